// The bottleneck product-residual quantiser of the rvq+swinT codec (RVQCodecs) in ONE launch per batch part
//   frame  ->  per-group down-projection  ->  S residual stages (normalise, codebook search, code, subtract the raw row, add it to the sum)
//   ->  up-projection of the SUM  ->  un-framed store into the decoder's input map
//                                   (quantization.py:139-431 ResidualVectorQuantize / ProductResidualVectorQuantize; codebook.py:20-55)
//
// It reuses the structure of pvq_fused_kernel (fused_pvq.h) phase for phase:
//   P1 / P2  identical: wave z is split-K slice z of the down-projection (partials in LDS), the slices are added in slice order, so the projected
//            vector is bit for bit what ESC's stream-0 quantiser computes for the same weights.  The projected vector is the stage-0 residual.
//   P3       a loop over the stages s < S_b (S_b = the clip's own count: a per-clip device array, or one uniform S).  Each stage normalises the
//            residual (same fmaf chain, IEEE sqrt and division as P2), searches the stage's normalised codebook with the same MFMA dot products,
//            running argmin and cross-wave combine (tie -> lowest index, NaN semantics of torch.min), writes the code, gathers the RAW row
//            (codebook.py:52-53), subtracts it from the residual and adds it to the running sum (quantization.py:180-186: residual - z_q_i,
//            z_q + z_q_i, the sum starting from 0).  The optional per-vector commitment term mse(z_q_i, residual_i) goes to a per-stage slot
//            loss[s][g][m], reduced per clip afterwards by loss_reduce (fixed order, no atomics).  Slots S_b .. Smax-1 get code -1 and loss 0.
//   P4       (forward) the MFMA up-projection of pvq_fused_kernel's P4, with the summed vector as the operand instead of one codebook row
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
    constexpr int NP = 16 * NT, NPS = NP + 4, DT = 4 * STEPS, KC = NT;
    extern __shared__ __attribute__((aligned(16))) float prvq_part[];           // [16 slices][16 rows][NPS] (encode form only)
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
        // ---- P1: split-K slice `wave` of the down-projection (pvq_fused_kernel's P1 without a residual map) ----
        {
            constexpr int PF = NT >= 6 ? 2 : (NT >= 4 ? 3 : (NT == 3 ? 4 : (NT == 2 ? 5 : 6)));
            const int kbeg = wave * a.k_per_z, kend = min(a.Kq, kbeg + a.k_per_z);
            if (wave < a.splits && kbeg < kend) {                  // wave-uniform
                const int nch = (kend - kbeg) >> 4;
                const float* wfrag = a.wd + (size_t)lane * 4;
                f32x4 er[PF], wr[PF][NT];
                auto issue = [&](int ci, f32x4& e, f32x4 (&wf)[NT]) {
                    const int k0 = kbeg + 16 * min(ci, nch - 1);                               // past the end: re-read the last chunk (never consumed)
                    const int oh = k0 / a.Cp, cc = k0 - oh * a.Cp, o = oh / a.Hq, h = oh - o * a.Hq;
                    e = ld4(a.enc + vecbase + (size_t)(h * a.Wd + o) * a.Cp + cc);
#pragma unroll
                    for (int n = 0; n < NT; ++n) wf[n] = ld4(wfrag + ((size_t)(k0 >> 4) * NT + n) * 256);
                };
                f32x4 acc[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) acc[n] = zero4();
                auto consume = [&](const f32x4& e, const f32x4 (&wf)[NT]) {
                    f32x4 af = e;
                    if (!live) af = zero4();
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int n = 0; n < NT; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[n][r], af[r], acc[n], 0, 0, 0);
                };
#pragma unroll
                for (int j = 0; j < PF; ++j) issue(j, er[j], wr[j]);
                const int rounds = nch / PF, tail = nch - rounds * PF;
                for (int rd = 0; rd < rounds; ++rd) {
#pragma unroll
                    for (int j = 0; j < PF; ++j) {
                        consume(er[j], wr[j]);
                        issue((rd + 1) * PF + j, er[j], wr[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < PF - 1; ++j)
                    if (j < tail) consume(er[j], wr[j]);
                float* pr = prvq_part + ((size_t)wave * 16 + l15) * NPS + 4 * lg;
#pragma unroll
                for (int n = 0; n < NT; ++n) st4(pr + 16 * n, acc[n]);
            }
        }
        __syncthreads();
        // ---- P2: slices added in slice order: the stage-0 residual ----
        for (int e = tid; e < 16 * NP; e += 64 * PVQF_WAVES) {
            const int r = e / NP, n = e - r * NP;
            float z = 0.f;
#pragma unroll
            for (int s = 0; s < 16; ++s) z += (s < a.splits) ? prvq_part[((size_t)s * 16 + r) * NPS + n] : 0.f;
            res[r][n] = z;
        }
        __syncthreads();

        // ---- P3: the residual stages ----
        int s_hi = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) s_hi = max(s_hi, nst[i]);
        for (int s = 0; s < s_hi; ++s) {
            if (tid < 16 * a.G) {           // F.normalize and sum(zn^2) of the residual (P2's arithmetic)
                const int g = tid >> 4, vi = tid & 15;
                float zr[DT];
#pragma unroll
                for (int j = 0; j < DT; ++j) zr[j] = res[vi][g * DT + j];
                float ss = 0.f;
#pragma unroll
                for (int j = 0; j < DT; ++j) ss = (j < a.d) ? __builtin_fmaf(zr[j], zr[j], ss) : ss;
                const float den = a.l2norm ? fmaxf(sqrtf(ss), 1e-12f) : 1.0f;
                float s2 = 0.f;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    const float zn = (j < a.d) ? zr[j] / den : 0.f;
                    s2 = __builtin_fmaf(zn, zn, s2);
                    zn2[g][vi][j] = 2.0f * zn;
                }
                asum[g][vi] = s2;
            }
            __syncthreads();
            {                               // distances + running argmin (pvq_fused_kernel's P3 on stage s's codebooks)
                constexpr int TB = 4;
                const int per_wave = ((a.Ksz + PVQF_WAVES - 1) / PVQF_WAVES + 15) & ~15;
                const int cbeg = wave * per_wave, cend = min(a.Ksz, cbeg + per_wave);
                for (int g = 0; g < a.G; ++g) {
                    float zf[STEPS];
#pragma unroll
                    for (int r = 0; r < STEPS; ++r) zf[r] = zn2[g][l15][STEPS * lg + r];
                    const float av = asum[g][l15];
                    const float* cb = a.cbn + ((size_t)s * a.G + g) * a.Ksz * DT;
                    const float* c2 = a.c2 + ((size_t)s * a.G + g) * a.Ksz;
                    float bd = __builtin_inff();
                    int bi = 0x7fffffff;
                    bool have = false;
                    for (int cb0 = cbeg; cb0 < cend; cb0 += 16 * TB) {
                        float cf[TB][STEPS], c2v[TB][4];
#pragma unroll
                        for (int u = 0; u < TB; ++u) {
                            const int c0 = cb0 + 16 * u;
                            const float* p = cb + (size_t)min(c0 + l15, a.Ksz - 1) * DT + STEPS * lg;
#pragma unroll
                            for (int r = 0; r < STEPS; ++r) cf[u][r] = p[r];
#pragma unroll
                            for (int r = 0; r < 4; ++r) c2v[u][r] = c2[min(c0 + 4 * lg + r, a.Ksz - 1)];
                        }
#pragma unroll
                        for (int u = 0; u < TB; ++u) {
                            const int c0 = cb0 + 16 * u;
                            f32x4 dot = zero4();
#pragma unroll
                            for (int r = 0; r < STEPS; ++r) dot = __builtin_amdgcn_mfma_f32_16x16x4f32(cf[u][r], zf[r], dot, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int code = c0 + 4 * lg + r;
                                const float dist = (av - dot[r]) + c2v[u][r];
                                const bool in = code < cend;
                                const bool take = in & (!have | (!(dist >= bd) & (bd == bd)));
                                bd = take ? dist : bd; bi = take ? code : bi; have = have | in;
                            }
                        }
                    }
#pragma unroll
                    for (int o = 16; o <= 32; o <<= 1) {
                        const float od = __shfl_xor(bd, o);
                        const int oi = __shfl_xor(bi, o);
                        const bool n1 = od != od, n2 = bd != bd;
                        const bool better = (n1 | n2) ? (n1 & (!n2 | (oi < bi))) : ((od < bd) | ((od == bd) & (oi < bi)));
                        bd = better ? od : bd; bi = better ? oi : bi;
                    }
                    if (lg == 0) { bestd[wave][g][l15] = bd; besti[wave][g][l15] = bi; }
                }
            }
            __syncthreads();
            if (tid < 16 * a.G) {           // cross-wave argmin, code, commitment term, residual update, running sum
                const int g = tid >> 4, vi = tid & 15;
                float wd_[PVQF_WAVES]; int wi_[PVQF_WAVES];
#pragma unroll
                for (int w = 0; w < PVQF_WAVES; ++w) { wd_[w] = bestd[w][g][vi]; wi_[w] = besti[w][g][vi]; }
                float d0 = wd_[0]; int i0 = wi_[0];
#pragma unroll
                for (int w = 1; w < PVQF_WAVES; ++w) {
                    const bool n1 = wd_[w] != wd_[w], n2 = d0 != d0;
                    const bool better = (n1 | n2) ? (n1 & (!n2 | (wi_[w] < i0))) : ((wd_[w] < d0) | ((wd_[w] == d0) & (wi_[w] < i0)));
                    d0 = better ? wd_[w] : d0; i0 = better ? wi_[w] : i0;
                }
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

    // ---- P4: up-projection of the summed vector + un-framed store (pvq_fused_kernel's MFMA form of P4, no residual map) ----
    {
        constexpr int UNR = KC >= 6 ? 2 : (KC >= 4 ? 3 : (KC == 3 ? 4 : 6));
        f32x4 zf[KC];
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) zf[c][r] = zsum[l15][16 * c + 4 * lg + r];       // padding elements of the sum are zero
        const int NTo = a.Kq / 16;
        const float* wrow = a.wup + (size_t)l15 * NP + 4 * lg;
        for (int nt0 = wave * UNR; nt0 < NTo; nt0 += PVQF_WAVES * UNR) {
            f32x4 wf[UNR][KC];
            size_t idx[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int nt = min(nt0 + u, NTo - 1);                              // ragged tail: a duplicate tile, not stored
#pragma unroll
                for (int c = 0; c < KC; ++c) wf[u][c] = ld4(wrow + (size_t)(16 * nt) * NP + 16 * c);
                const int n0 = 16 * nt, oh = n0 / a.Cp, c0 = n0 - oh * a.Cp, o = oh / a.Hq, h = oh - o * a.Hq;      // wave-uniform
                idx[u] = vecbase + (size_t)(h * a.Wd + o) * a.Cp + c0;
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                f32x4 acc = zero4();
#pragma unroll
                for (int c = 0; c < KC; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u][c][r], zf[c][r], acc, 0, 0, 0);
                if (live && nt0 + u < NTo) st4(a.out + idx[u], acc);
            }
        }
    }
}

}  // namespace escx
