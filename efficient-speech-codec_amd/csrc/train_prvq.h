// Training form of the bottleneck product-residual quantiser of the rvq+swinT codec (RVQCodecs): forward in ONE launch per batch part, backward in ONE
// launch (+ the deterministic codebook scatter of train_kernels.h per live stage).
//                                   (quantization.py:167-196 residual_vector_quantization, 298-335 ProductResidualVectorQuantize.forward; codebook.py:57-75)
//
// Forward (prvq_train_fwd_kernel).  P1 / P2 / the search of every stage are prvq_fused_kernel's: the shared device functions of fused_pvq.h, so every decision
// that picks a code is the eval kernel's code.  What differs is what training mode does around the search:
//   * ALL num_rvqs stages run whatever num_streams is (quantization.py:178-187: the break is eval-only); codes has num_rvqs slots.
//   * the straight-through arithmetic is stated literally, in fp32 and in this order (codebook.py:70, quantization.py:184-189):
//         z_i = r_i + (q_i - r_i)        (NOT q_i bit for bit)
//         r_i+1 = r_i - z_i              (NOT r_i - q_i bit for bit)
//         i >= S:  z_i = z_i * 0,  term_i = 0
//         z_q = z_q + z_i                (from 0., stage order)
//     with contraction off - residuals and later codes would otherwise drift from the reference's training forward in the last bit.
//   * term_i = sum_j (q_i - r_i)^2 / (Tq d G) goes to terms[i][g][m] (commitment == codebook loss numerically), reduced per clip by loss_reduce: no atomics.
//   * freeze_vq (quantization.py:319-321): the operand of the up-projection is z_e + z_q * 0 and every term is 0.
//   * the tape gets the projected vectors z_e (M, Nz) and the up-projection's operand (M, Nz): the masked sum, or z_e when frozen.
// Rows past M in the last 16-row tile write nothing (codes, terms, tape, map).
//
// Backward (prvq_train_bwd_kernel, in train_kernels.h beside the cross-scale quantiser's and the codebook scatter).  One thread per (vector, group) replays the residual chain from z_e and the codes in the forward's exact arithmetic.
//   d z_e = g + (2 / (Tq d G)) d_cm[b] (r_0 - q_0)        g = d L / d z_q_m from the up-projection;  frozen: d z_e = g
//   gq_i  = (2 / (Tq d G)) d_cb[b] (q_i - r_i),  i < S    the per-vector contribution to codebook row code_i of (stage i, group); summed per row, in a fixed
//                                                         order, by codebook_grad_kernel
// The residual chain itself carries no gradient: d r_{i+1} / d r_i = 1 - 1, so the commitment terms of the stages i >= 1 cancel exactly and those stages
// reach the encoder through g alone.  Stages i >= S and the frozen form contribute exact zeros (their codebook regions stay at the memset).
#pragma once
#include <hip/hip_runtime.h>
#include "gemm_engine.h"
#include "kernels.h"
#include "fused_pvq.h"

namespace escx {

struct PrvqTrainArgs {
    const float* enc;                               // bottleneck map (B, Hq, Wd, Cp), frames read in place
    const float* wd;                                // down-projection in MFMA fragment order (Quant::wdf)
    const float* cbn; const float* c2; const float* cbraw;      // [R][G][Ksz][dt] normalised, [R][G][Ksz] squared norms, [R][G][Ksz][dt] raw
    const float* wup;                               // [Kq][Np] up-projection
    float* out;                                     // decoder input map (B, Hq, Wd, Cp), un-framed
    long long* codes; long long bstride;            // codes[b * bstride + (i * G + g) * Tq + t], all R stages
    float* ze; float* zq;                           // tape: projected vectors and the up-projection's operand, (M, Np) each
    float* terms; long long lslot; float loss_scale;      // terms[i * lslot + g * M + m]
    int S, R, freeze;
    int M, Tq, Hq, Wd, Cp, ov, Kq, k_per_z, splits;
    int G, Ksz, d, l2norm;
};

template <int NT, int STEPS>
__global__ __launch_bounds__(64 * PVQF_WAVES) void prvq_train_fwd_kernel(PrvqTrainArgs a) {
#pragma clang fp contract(off)
    ESCX_SET_PRIO_SMALL();
    constexpr int NP = 16 * NT, DT = 4 * STEPS, KC = NT;
    extern __shared__ __attribute__((aligned(16))) float prvq_tpart[];          // [16 slices][16 rows][NP + 4]
    __shared__ float res[16][NP + 1];               // residual entering the current stage (stage 0: z_e)
    __shared__ float zsum[16][NP + 1];              // the masked sum, then the operand of the up-projection
    __shared__ float zn2[PVQF_GMAX][16][DT];
    __shared__ float asum[PVQF_GMAX][16];
    __shared__ float bestd[PVQF_WAVES][PVQF_GMAX][16];
    __shared__ int besti[PVQF_WAVES][PVQF_GMAX][16];
    const int tid = threadIdx.x;
    const int lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * 16;
    const int m = m0 + l15;
    const bool live = m < a.M;
    const int b = live ? m / a.Tq : 0, t = live ? m - b * a.Tq : 0;                 // rows past M alias vector 0: valid memory, their values are discarded
    const size_t vecbase = ((size_t)b * a.Hq * a.Wd + (size_t)a.ov * t) * a.Cp + 4 * lg;
    const size_t GT = (size_t)a.G * a.Tq;

    for (int e = tid; e < 16 * (NP + 1); e += 64 * PVQF_WAVES) (&zsum[0][0])[e] = 0.f;
    pvq_down_slice<NT, false>(a.enc, nullptr, a.wd, vecbase, live, lane, wave, a.Kq, a.k_per_z, a.splits, a.Hq, a.Wd, a.Cp, prvq_tpart);         // P1
    __syncthreads();
    pvq_sum_slices<NT>(prvq_tpart, a.splits, tid, res);                                                                                          // P2: z_e = the stage-0 residual
    __syncthreads();
    for (int e = tid; e < 16 * NP; e += 64 * PVQF_WAVES) {                          // tape: z_e (the padding columns are the zero rows of the projection)
        const int r = e / NP, n = e - r * NP;
        if (m0 + r < a.M) a.ze[(size_t)(m0 + r) * NP + n] = res[r][n];
    }
    float zev[DT];                                  // z_e of this thread's (vector, group): the frozen form's operand
    if (tid < 16 * a.G) {
        const int g = tid >> 4, vi = tid & 15;
#pragma unroll
        for (int j = 0; j < DT; ++j) zev[j] = res[vi][g * DT + j];
    }

    // ---- the residual stages: every one runs (training mode) ----
    for (int s = 0; s < a.R; ++s) {
        pvq_normalise<NT, STEPS>(res, tid, a.G, a.d, a.l2norm, zn2, asum);
        __syncthreads();
        for (int g = 0; g < a.G; ++g)
            pvq_search_group<STEPS>(a.cbn + ((size_t)s * a.G + g) * a.Ksz * DT, a.c2 + ((size_t)s * a.G + g) * a.Ksz, a.Ksz, g, wave, l15, lg, zn2, asum, bestd, besti);
        __syncthreads();
        if (tid < 16 * a.G) {
            const int g = tid >> 4, vi = tid & 15;
            int i0 = pvq_combine_waves(bestd, besti, g, vi);
            const int mm = m0 + vi;
            if (mm < a.M) {
                i0 = i0 < 0 ? 0 : (i0 >= a.Ksz ? a.Ksz - 1 : i0);        // a NaN-only row keeps the lowest index; never outside the codebook
                const int bb = mm / a.Tq, tt = mm - bb * a.Tq;
                a.codes[(size_t)bb * a.bstride + (size_t)s * GT + (size_t)g * a.Tq + tt] = (long long)i0;
                const float* q = a.cbraw + (((size_t)s * a.G + g) * a.Ksz + i0) * DT;
                float qv[DT];
#pragma unroll
                for (int j = 0; j < DT; ++j) qv[j] = q[j];
                const bool on = s < a.S;
                float e = 0.f;
                for (int j = 0; j < a.d; ++j) { const float df = qv[j] - res[vi][g * DT + j]; e = __builtin_fmaf(df, df, e); }
                a.terms[(size_t)s * a.lslot + (size_t)g * a.M + mm] = (on && !a.freeze) ? e * a.loss_scale : 0.f;
#pragma unroll
                for (int j = 0; j < DT; ++j) {
                    const float r = res[vi][g * DT + j];
                    const float dq = qv[j] - r;
                    float z = r + dq;                           // z_e + (z_q - z_e).detach()
                    res[vi][g * DT + j] = r - z;                // residual - z_q_i, with the STE value
                    if (!on) z = z * 0.f;
                    zsum[vi][g * DT + j] = zsum[vi][g * DT + j] + z;
                }
            }
        }
        __syncthreads();
    }
    if (a.freeze && tid < 16 * a.G) {               // z_q_m = z_e_m + z_q_m * 0.
        const int g = tid >> 4, vi = tid & 15;
#pragma unroll
        for (int j = 0; j < DT; ++j) zsum[vi][g * DT + j] = zev[j] + zsum[vi][g * DT + j] * 0.f;
    }
    __syncthreads();
    for (int e = tid; e < 16 * NP; e += 64 * PVQF_WAVES) {                          // tape: the operand of the up-projection
        const int r = e / NP, n = e - r * NP;
        if (m0 + r < a.M) a.zq[(size_t)(m0 + r) * NP + n] = zsum[r][n];
    }

    // ---- up-projection of the operand + un-framed store (prvq_fused_kernel's P4) ----
    f32x4 zf[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) zf[c][r] = zsum[l15][16 * c + 4 * lg + r];
    pvq_up_mfma<NT, false>(zf, a.wup, nullptr, a.out, vecbase, live, wave, l15, lg, a.Kq, a.Hq, a.Wd, a.Cp);
}

}  // namespace escx
