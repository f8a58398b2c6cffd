// The bottleneck product-residual quantiser of the rvq+swinT codec (RVQCodecs) in ONE launch per batch part
//   frame  ->  per-group down-projection  ->  S residual stages (normalise, codebook search, code, subtract the raw row, add it to the sum)
//   ->  up-projection of the SUM  ->  un-framed store into the decoder's input map
//                                   (quantization.py:139-431 ResidualVectorQuantize / ProductResidualVectorQuantize; codebook.py:20-55)
//
// Every phase that decides a code index is pvq_fused_kernel's own code: the shared device functions of fused_pvq.h, called from both kernels.
//   P1 / P2  pvq_down_slice, pvq_sum_slices: wave z is split-K slice z of the down-projection (partials in LDS), the slices are added in slice order,
//            so the projected vector is bit for bit what ESC's stream-0 quantiser computes for the same weights.  It is the stage-0 residual.
//   P3       a loop over the stages s < S_b (S_b = the clip's own count: a per-clip device array, or one uniform S).  Each stage normalises the
//            residual (pvq_normalise), searches the stage's normalised codebooks (pvq_search_group, pvq_combine_waves: tie -> lowest index, NaN
//            semantics of torch.min), writes the code, gathers the RAW row (codebook.py:52-53), subtracts it from the residual and adds it to the
//            running sum (quantization.py:180-186: residual - z_q_i, z_q + z_q_i, the sum starting from 0).  The optional per-vector commitment
//            term mse(z_q_i, residual_i) goes to a per-stage slot loss[s][g][m], reduced per clip afterwards by loss_reduce (fixed order, no
//            atomics).  Slots S_b .. Smax-1 get code -1 and loss 0.
//   P4       (forward) pvq_up_mfma with the summed vector as the operand instead of one codebook row
//            (quantization.py:320: proj_up of the SUM, not the sum of up-projections); no residual map is added.
// DECODE = true is the codes-in form of the same kernel (escx_decode): P1-P3 are replaced by the gather-sum of the raw rows in stage order from
// 0.f, and P4 is the same code - so eval forward's audio equals decode(encode(x)) bit for bit.
// Covered geometries: (Np / 16, dt / 4) = (2, 2) (the ablation yaml: 3 groups of d = 8) and (1, 1) (d <= 4, up to 4 groups); anything else is
// refused when the handle is created (prvq_geometry_ok).
#pragma once
#include <hip/hip_runtime.h>
#include "gemm_engine.h"
#include "kernels.h"
#include "fused_pvq.h"

namespace escx {

struct PrvqArgs {
    const float* enc;                               // bottleneck map (B, Hq, Wd, Cp): the frames are read in place, as pvq_fused_kernel does
    const float* wd;                                // down-projection in MFMA fragment order (Quant::wdf), k = (o, h, c)
    const float* cbn; const float* c2; const float* cbraw;      // [S][G][Ksz][dt] normalised, [S][G][Ksz] squared norms, [S][G][Ksz][dt] raw
    const float* wup;                               // [Kq][Np] up-projection
    float* out;                                     // decoder input map (B, Hq, Wd, Cp), un-framed; nullptr: codes only
    long long* codes; const long long* codes_in; long long bstride;      // codes[b * bstride + (s * G + g) * Tq + t]; codes_in: DECODE form
    const int* clip_S; int S, Smax;                 // per-clip stage counts (indexed by clip, nullptr = S for every clip); Smax = slots per clip
    float* loss; long long lslot; float loss_scale; // optional per-vector commitment terms, loss[s * lslot + g * M + m]
    int M, Tq, Hq, Wd, Cp, ov, Kq, k_per_z, splits;
    int G, Ksz, d, l2norm;
};

template <int NT, int STEPS, bool DECODE>
__global__ __launch_bounds__(64 * PVQF_WAVES) void prvq_fused_kernel(PrvqArgs a) {
#pragma clang fp contract(off)
    ESCX_SET_PRIO_SMALL();
    constexpr int NP = 16 * NT, DT = 4 * STEPS, KC = NT;
    extern __shared__ __attribute__((aligned(16))) float prvq_part[];           // [16 slices][16 rows][NP + 4] (encode form only)
    __shared__ float res[16][NP + 1];               // residual entering the current stage
    __shared__ float zsum[16][NP + 1];              // running sum of the raw rows (the operand of the up-projection)
    __shared__ float zn2[PVQF_GMAX][16][DT];
    __shared__ float asum[PVQF_GMAX][16];
    __shared__ float bestd[PVQF_WAVES][PVQF_GMAX][16];
    __shared__ int besti[PVQF_WAVES][PVQF_GMAX][16];
    __shared__ int nst[16];                         // stages of every row (0 for rows past M)
    const int tid = threadIdx.x;
    const int lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * 16;
    const int m = m0 + l15;
    const bool live = m < a.M;
    const int b = live ? m / a.Tq : 0, t = live ? m - b * a.Tq : 0;                 // rows past M alias vector 0: valid memory, their values are discarded
    const size_t vecbase = ((size_t)b * a.Hq * a.Wd + (size_t)a.ov * t) * a.Cp + 4 * lg;
    const size_t GT = (size_t)a.G * a.Tq;

    if (tid < 16) {
        const int mm = m0 + tid;
        int sb = 0;
        if (mm < a.M) { sb = a.clip_S ? a.clip_S[mm / a.Tq] : a.S; sb = sb < 0 ? 0 : (sb > a.Smax ? a.Smax : sb); }
        nst[tid] = sb;
    }
    for (int e = tid; e < 16 * (NP + 1); e += 64 * PVQF_WAVES) (&zsum[0][0])[e] = 0.f;
    __syncthreads();

    if constexpr (DECODE) {
        // ---- codes in: z_q = ((0 + e_0) + e_1) + ... in stage order (quantization.py:283-289), the sum the encode form accumulates ----
        if (tid < 16 * a.G) {
            const int g = tid >> 4, vi = tid & 15, mm = m0 + vi;
            if (mm < a.M) {
                const int bb = mm / a.Tq, tt = mm - bb * a.Tq;
                float acc[DT];
#pragma unroll
                for (int j = 0; j < DT; ++j) acc[j] = 0.f;
                for (int s = 0; s < nst[vi]; ++s) {
                    long long code = a.codes_in[(size_t)bb * a.bstride + (size_t)s * GT + (size_t)g * a.Tq + tt];
                    code = code < 0 ? 0 : (code >= a.Ksz ? a.Ksz - 1 : code);       // a corrupt index must not read outside the codebook (F.embedding would raise)
                    const float* q = a.cbraw + (((size_t)s * a.G + g) * a.Ksz + (size_t)code) * DT;
#pragma unroll
                    for (int j = 0; j < DT; ++j) acc[j] = acc[j] + q[j];
                }
#pragma unroll
                for (int j = 0; j < DT; ++j) zsum[vi][g * DT + j] = acc[j];
            }
        }
        __syncthreads();
    } else {
        pvq_down_slice<NT, false>(a.enc, nullptr, a.wd, vecbase, live, lane, wave, a.Kq, a.k_per_z, a.splits, a.Hq, a.Wd, a.Cp, prvq_part);      // P1
        __syncthreads();
        pvq_sum_slices<NT>(prvq_part, a.splits, tid, res);                                                                                        // P2: the stage-0 residual
        __syncthreads();

        // ---- P3: the residual stages ----
        int s_hi = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s_hi = max(s_hi, nst[i]);
        for (int s = 0; s < s_hi; ++s) {
            pvq_normalise<NT, STEPS>(res, tid, a.G, a.d, a.l2norm, zn2, asum);
            __syncthreads();
            for (int g = 0; g < a.G; ++g)
                pvq_search_group<STEPS>(a.cbn + ((size_t)s * a.G + g) * a.Ksz * DT, a.c2 + ((size_t)s * a.G + g) * a.Ksz, a.Ksz, g, wave, l15, lg, zn2, asum, bestd, besti);
            __syncthreads();
            if (tid < 16 * a.G) {           // cross-wave argmin, code, commitment term, residual update, running sum
                const int g = tid >> 4, vi = tid & 15;
                int i0 = pvq_combine_waves(bestd, besti, g, vi);
                const int mm = m0 + vi;
                if (mm < a.M && s < nst[vi]) {
                    i0 = i0 < 0 ? 0 : (i0 >= a.Ksz ? a.Ksz - 1 : i0);        // a NaN-only row keeps the lowest index; never outside the codebook
                    const int bb = mm / a.Tq, tt = mm - bb * a.Tq;
                    a.codes[(size_t)bb * a.bstride + (size_t)s * GT + (size_t)g * a.Tq + tt] = (long long)i0;
                    const float* q = a.cbraw + (((size_t)s * a.G + g) * a.Ksz + i0) * DT;
                    float qv[DT];
#pragma unroll
                    for (int j = 0; j < DT; ++j) qv[j] = q[j];
                    if (a.loss) {           // eval-mode commitment term: mse(z_q_i, residual_i).mean([1,2]) / groups (codebook.py:72-73, quantization.py:337-338)
                        float e = 0.f;
                        for (int j = 0; j < a.d; ++j) { const float df = qv[j] - res[vi][g * DT + j]; e = __builtin_fmaf(df, df, e); }
                        a.loss[(size_t)s * a.lslot + (size_t)g * a.M + mm] = e * a.loss_scale;
                    }
#pragma unroll
                    for (int j = 0; j < DT; ++j) {
                        res[vi][g * DT + j] = res[vi][g * DT + j] - qv[j];
                        zsum[vi][g * DT + j] = zsum[vi][g * DT + j] + qv[j];
                    }
                }
            }
            __syncthreads();
        }
        if (tid < 16 * a.G) {               // slots past the clip's own count
            const int g = tid >> 4, vi = tid & 15, mm = m0 + vi;
            if (mm < a.M) {
                const int bb = mm / a.Tq, tt = mm - bb * a.Tq;
                for (int s = nst[vi]; s < a.Smax; ++s) {
                    a.codes[(size_t)bb * a.bstride + (size_t)s * GT + (size_t)g * a.Tq + tt] = -1;
                    if (a.loss) a.loss[(size_t)s * a.lslot + (size_t)g * a.M + mm] = 0.f;
                }
            }
        }
    }
    if (!a.out) return;

    // ---- P4: up-projection of the summed vector + un-framed store ----
    f32x4 zf[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) zf[c][r] = zsum[l15][16 * c + 4 * lg + r];       // padding elements of the sum are zero
    pvq_up_mfma<NT, false>(zf, a.wup, nullptr, a.out, vecbase, live, wave, l15, lg, a.Kq, a.Hq, a.Wd, a.Cp);
}

}  // namespace escx
