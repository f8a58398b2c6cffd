// Device code of the multi-scale discriminator (MSD; reference esc/models/discriminator.py:69-99): the FIR resampler in front of it and the four
// grouped, stride-4, 41-tap Conv1d layers (16 -> 64 -> 256 -> 1024 -> 1024 channels in 4 / 16 / 64 / 256 groups).  The three dense layers
// (convs.0, convs.5, conv_post) are ordinary implicit GEMMs of disc_kernels.h.  DESIGN.md section 14.
//
// Every group has 4 input channels, so one tap of one group is exactly one K step of v_mfma_f32_16x16x4_f32: per group the contraction is
// 41 taps x 4 channels = 164.  Maps are channels-last [B][T][C] (C = Cp: 16, 64, 256, 1024), weights are the packed image wn_pack_kernel writes
// with Cin = CinP = 4:  Wf[co][t * 4 + ci], row stride Kf = 176 (= 11 column tiles of 16; columns 164.. stay zero).
//   GPT (groups per 16-channel output tile) = 1: a group has 16 outputs, the tile is one group.
//   GPT = 4 (convs.4: 4 outputs per group): the tile spans 4 groups; each tap takes 4 MFMAs, one per group, with the weights of the other
//   groups' output channels masked to zero (4x the MFMA issue of a 16-output group on a layer that holds 1/6 of the grouped FLOPs).
// One wave owns one 16 x 16 accumulator tile D[row = 4 * (lane >> 4) + e][col = lane & 15] with channels along the rows, so a lane stores four
// consecutive channels of one position with one 16-byte store.  No LDS, no atomics; every sum runs in an order fixed by the geometry.
#pragma once
#include <hip/hip_runtime.h>
#include "disc_kernels.h"

namespace escx {

constexpr int MSD_TAPS = 41, MSD_STRIDE = 4, MSD_PAD = 20, MSD_KF = 176;

// ------------------------------------------------------------------------------------------------
// Resampler: out(b, n) = sum_j k[j] * y(b, clamp(n * old + j - width, 0, L - 1)), n < Lr = L / old; written as the
// 4-channel-padded input map [B][Lr][4] = (value, 0, 0, 0) of convs.0.  rate 1: ntaps = 1, k = {1}, width = 0.
// ------------------------------------------------------------------------------------------------
__global__ void msd_resample_kernel(const float* __restrict__ y, const float* __restrict__ k, float* __restrict__ out, int B, int L, int Lr, int old, int width,
                                    int ntaps) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * Lr) return;
    const int n = (int)(idx % Lr), b = (int)(idx / Lr);
    const float* yr = y + (size_t)b * L;
    const int base = n * old - width;
    float s = 0.f;
    for (int j = 0; j < ntaps; ++j) {
        int i = base + j; i = i < 0 ? 0 : (i > L - 1 ? L - 1 : i);
        s += k[j] * yr[i];
    }
    st4(out + idx * 4, f32x4{s, 0.f, 0.f, 0.f});
}
// adjoint: dy(b, i) += sum over (n, j) with clamp(n * old + j - width) == i of k[j] * din(b, n); the two end samples also collect the replicate padding
__global__ void msd_resample_bwd_kernel(const float* __restrict__ din, const float* __restrict__ k, float* __restrict__ dy, int B, int L, int Lr, int old, int width,
                                        int ntaps) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * L) return;
    const int i = (int)(idx % L), b = (int)(idx / L);
    const float* g = din + (size_t)b * Lr * 4;
    // padded positions q = n * old + j that map onto sample i: [qlo, qhi]
    const int qlo = i == 0 ? 0 : i + width, qhi = i == L - 1 ? (Lr - 1) * old + ntaps - 1 : i + width;
    int nlo = (qlo - ntaps + 1 + old - 1) / old; if (qlo - ntaps + 1 <= 0) nlo = 0;
    int nhi = qhi / old; if (nhi > Lr - 1) nhi = Lr - 1;
    float s = 0.f;
    for (int n = nlo; n <= nhi; ++n) {
        const int jlo = qlo - n * old > 0 ? qlo - n * old : 0, jhi = qhi - n * old < ntaps - 1 ? qhi - n * old : ntaps - 1;
        const float gn = g[(size_t)n * 4];
        for (int j = jlo; j <= jhi; ++j) s += k[j] * gn;
    }
    dy[idx] += s;
}

// ------------------------------------------------------------------------------------------------
// forward: y(b, o, co) = LeakyReLU(bias[co] + sum_{t, ci} x(b, 4 o + t - 20, 4 g + ci) * Wf[co][4 t + ci]), g = group of co.  M = B * O rows.
// The K slots of an MFMA are four TAPS (slot s of step (u, e): tap 4 u + s, channel e), so a lane reads the 4 channels of its tap with one
// 16-byte load and its weights Wf[co][16 u + 4 s ..] with another, then issues 4 MFMAs: 11 steps cover the 176 columns (taps 41 .. 43 are
// the zero padding of Wf and read x as zero).
// ------------------------------------------------------------------------------------------------
template <int GPT>
__global__ __launch_bounds__(256) void msd_gconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                            float* __restrict__ y, int M, int O, int T, int Cin, int Cout) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int ntiles = Cout >> 4;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nt = (int)(wid % ntiles); const long long mt = wid / ntiles;
    if (mt * 16 >= M) return;                                   // wave-uniform
    const long long m = mt * 16 + l15;
    const bool valid = m < M;
    const int b = valid ? (int)(m / O) : 0, o = valid ? (int)(m - (long long)b * O) : 0;
    const int i0 = o * MSD_STRIDE - MSD_PAD + lg;
    const float* xr = x + (size_t)b * T * Cin + nt * GPT * 4;
    const float* wr = W + (size_t)(nt * 16 + l15) * MSD_KF + 4 * lg;
    f32x4 acc0 = zero4(), acc1 = zero4();                       // two accumulator chains (the MFMA's dependent latency exceeds its issue interval)
#pragma unroll 2
    for (int u = 0; u < MSD_KF / 16; ++u) {
        const int i = i0 + 4 * u;
        const bool ok = valid && 4 * u + lg < MSD_TAPS && (unsigned)i < (unsigned)T;
        const f32x4 wv = ld4(wr + 16 * u);
#pragma unroll
        for (int kk = 0; kk < GPT; ++kk) {
            const f32x4 xv = ok ? ld4(xr + (size_t)i * Cin + kk * 4) : zero4();
            const f32x4 wm = (GPT == 1 || (l15 >> 2) == kk) ? wv : zero4();
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wm[0], xv[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wm[1], xv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wm[2], xv[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wm[3], xv[3], acc1, 0, 0, 0);
        }
    }
    if (!valid) return;
    f32x4 v = acc0 + acc1 + ld4(bias + nt * 16 + 4 * lg);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.1f * v[e];
    st4(y + (size_t)m * Cout + nt * 16 + 4 * lg, v);
}

// ------------------------------------------------------------------------------------------------
// dX: input position i = 4 q + r receives, from output position o = q + 5 - a through tap t = r + 4 a (a < 11),
//   dx(b, 4 q + r, 4 g + ci) = sum_{a, co in group g} dy(b, q + 5 - a, co) * Wf[co][16 a + (4 r + ci)]
// - the SAME dy row for the four residues r, and 16 consecutive columns of Wf (columns 164 .. 175 are its zero padding: the taps 41 .. 43 that
// a = 10 would reach for r > 0).  So one wave owns (group g, 16 values of q) = 64 positions x 4 channels: D[row = 4 r + ci][col = q], the
// contraction runs over (a, co) = 11 x CPG, and lane (q, r = lane >> 4) stores the 4 channels of position 4 q + r with one 16-byte store.
//   CPG = 16: per a, K slot s of MFMA e is output channel 4 s + e (a lane reads its 4 channels of dy with one 16-byte load).
//   CPG = 4:  K slot s of MFMA e is (a = 4 u + s, output channel e), u < 3; a = 11 is masked.
// Every position of the input map is written exactly once (GradOut: accumulate, or the final (init + v) * LeakyReLU' form).  M = B * ceil(T / 4).
// ------------------------------------------------------------------------------------------------
template <int CPG>
__global__ __launch_bounds__(256) void msd_gconv_dx_kernel(const float* __restrict__ dy, const float* __restrict__ W, GradOut go, int B, int O, int T, int Cin,
                                                           int Cout) {
    constexpr int NA = (MSD_TAPS + MSD_STRIDE - 1) / MSD_STRIDE;           // 11
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int Q = (T + MSD_STRIDE - 1) / MSD_STRIDE;
    const long long M = (long long)B * Q;
    const int G = Cin >> 2;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int g = (int)(wid % G); const long long mt = wid / G;
    if (mt * 16 >= M) return;                                   // wave-uniform
    const long long m = mt * 16 + l15;
    const bool valid = m < M;
    const int b = valid ? (int)(m / Q) : 0, q = valid ? (int)(m - (long long)b * Q) : 0;
    const float* dyr = dy + (size_t)b * O * Cout + g * CPG;
    const float* wr = W + (size_t)g * CPG * MSD_KF + l15;
    f32x4 acc0 = zero4(), acc1 = zero4();
    if constexpr (CPG == 16) {
#pragma unroll 2
        for (int a = 0; a < NA; ++a) {
            const int o = q + MSD_PAD / MSD_STRIDE - a;
            const bool ok = valid && (unsigned)o < (unsigned)O;
            const f32x4 gv = ok ? ld4(dyr + (size_t)o * Cout + 4 * lg) : zero4();
            const float* wa = wr + (size_t)(4 * lg) * MSD_KF + 16 * a;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0], gv[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[MSD_KF], gv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[2 * MSD_KF], gv[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[3 * MSD_KF], gv[3], acc1, 0, 0, 0);
        }
    } else {
        static_assert(CPG == 4, "4 or 16 output channels per group");
#pragma unroll
        for (int u = 0; u < (NA + 3) / 4; ++u) {
            const int a = 4 * u + lg;
            const bool aok = a < NA;
            const int o = q + MSD_PAD / MSD_STRIDE - a;
            const bool ok = valid && aok && (unsigned)o < (unsigned)O;
            const f32x4 gv = ok ? ld4(dyr + (size_t)o * Cout) : zero4();
            const float* wa = wr + 16 * (aok ? a : 0);          // (a = 11 lies behind the row: its dy reads as zero, the weight read is redirected)
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[0], gv[0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[MSD_KF], gv[1], acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[2 * MSD_KF], gv[2], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[3 * MSD_KF], gv[3], acc1, 0, 0, 0);
        }
    }
    const int i = MSD_STRIDE * q + lg;
    if (!valid || i >= T) return;
    go.put(((size_t)b * T + i) * Cin + g * 4, acc0 + acc1);
}

// ------------------------------------------------------------------------------------------------
// dW, dbias: part[slice][co][c], c = 4 t + ci < 164: sum over the slice's rows m = (b, o) of dy(m, co) * x(b, 4 o + t - 20, 4 g + ci); the rows
// are the K dimension (4 per MFMA).  Column 164 reads a constant 1, so it holds the bias gradient, which goes to bpart[slice][co].
// A wave owns (16 output channels, one row slice) and all 11 column tiles: the dy operand and the row's (b, o) are fetched once per 4 rows
// and serve 11 MFMAs (11 independent accumulators).  reduce_partials_kernel adds the slices in increasing order.
// ------------------------------------------------------------------------------------------------
template <int GPT>
__global__ __launch_bounds__(256) void msd_gconv_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ part,
                                                           float* __restrict__ bpart, int M, int O, int T, int Cin, int Cout, int mps) {
    constexpr int NCT = MSD_KF / 16;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int nt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (nt >= (Cout >> 4)) return;                              // wave-uniform
    const int slice = blockIdx.y;
    const int m0 = slice * mps, m1 = min(M, m0 + mps);
    const int tl = l15 >> 2, ci = l15 & 3;                      // this lane's column of B in column tile ct: tap 4 ct + tl, channel ci
    f32x4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) acc[ct] = zero4();
    for (int mb = m0; mb < m1; mb += 4) {                       // rows behind m1 read as zero
        const int m = mb + lg;
        const bool valid = m < m1;
        const int b = valid ? m / O : 0, o = valid ? m - b * O : 0;
        const int i0 = o * MSD_STRIDE - MSD_PAD + tl;
        const float gv = valid ? dy[(size_t)m * Cout + nt * 16 + l15] : 0.f;
        const float* xr = x + (size_t)b * T * Cin + nt * GPT * 4 + ci;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int i = i0 + 4 * ct;
            const bool ok = valid && 4 * ct + tl < MSD_TAPS && (unsigned)i < (unsigned)T;
            const bool one = ct == NCT - 1 && l15 == 4;         // column 164
#pragma unroll
            for (int kk = 0; kk < GPT; ++kk) {
                float xv = ok ? xr[(size_t)i * Cin + kk * 4] : 0.f;
                if (one && valid) xv = 1.f;
                const float gm = (GPT == 1 || (l15 >> 2) == kk) ? gv : 0.f;
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(gm, xv, acc[ct], 0, 0, 0);
            }
        }
    }
    float* pr = part + ((size_t)slice * Cout + nt * 16 + 4 * lg) * MSD_KF + l15;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e) pr[(size_t)e * MSD_KF + ct * 16] = acc[ct][e];
    if (l15 == 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bpart[(size_t)slice * Cout + nt * 16 + 4 * lg + e] = acc[NCT - 1][e];
    }
}

}  // namespace escx
