// Device code of the parameter gradients through the DAC baseline's decoder (reference: baselines/descript/dac/model/dac.py:249-266 DAC.decode,
// dac.py:24-41 ResidualUnit, dac.py:94-145 DecoderBlock / Decoder, nn/layers.py:5-33 weight-normalised layers and Snake1d), eval mode, padding on.
// DESIGN.md section 13.5.
//
// The weight gradient of every convolution is gemm_dw_kernel of train_kernels.h (fp32 MFMA over row slices, the slices' partial tiles added in
// increasing order; under escx_dac_set_param_grad_precision(ESCX_PRECISION_BF16X3) gemm_dw_bf16_kernel<.., 3> of gemm_bf16.h, the same contraction
// with split operands and 128 x 128 tiles) with DacConvA on both sides, over the layer's output gradient dY and its forward operand s (the Snaked saved map, or the
// staged latent for the first convolution), both channels-last:
//   Conv1d (K taps, dilation d, padding p)         rows (b, t) of dY:  A = dY rows (one tap),  B[(b, t)][tap * CinP + ci] = s(b, t - p + tap d, ci)
//                                                  dW[co][tap * CinP + ci]
//   ConvTranspose1d (stride st, 2 st taps, p)      rows (b, t) of s:   A = s rows (one tap),   B[(b, t)][tap * CoutP + co] = dY(b, t st - p + tap, co)
//                                                  dW[ci][tap * CoutP + co]
// Either way the staged gradient is dW[i][tap * JP + j] for the weight_v element (i, j, tap): i is the dimension the weight norm keeps (Cout of a
// Conv1d, Cin of a ConvTranspose1d; nn/layers.py:5-10), and dac_wn_bwd_kernel takes it back to weight_g and weight_v.
// The bias gradient is the column sums of dY (dac_colsum_kernel).  The Snake gradient needs v = conv^T(dY), the value DacGradEpi multiplies by
// snake'(x): DacGradEpiV is DacGradEpi's map form with v also stored to a second map, and dac_colsum_kernel sums v * d snake / d alpha over the rows.
// The column sums and the weight norm's two dot products are accumulated in fp64 (a few adds per element read; the terms are fp32).  No atomics;
// every sum runs in an order fixed by the geometry.
#pragma once
#include "dac_grad_kernels.h"

namespace escx {

// d/d alpha (x + sin(alpha x)^2 / (alpha + 1e-9)) = x sin(2 alpha x) / (alpha + 1e-9) - sin(alpha x)^2 / (alpha + 1e-9)^2, with the forward's inv
// table, the accurate sinf and no contraction into fma
__device__ __forceinline__ float dac_snake_grad_alpha(float x, float a, float inv) {
#pragma clang fp contract(off)
    const float ax = a * x;
    const float s2 = sinf(2.0f * ax), s = sinf(ax);
    return (x * s2) * inv - ((s * s) * inv) * inv;
}

struct DacGradEpiV {
    static constexpr bool CHUNKED_K = true;     // as DacGradEpi: the same kernel up to the extra store, so `out` has the same bits
    float* out; const float* res; const float* xs; const float* alpha; const float* inv; float* vout;      // vout aliases none of the others
    int Cp;
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (n >= Cp) return;
        const size_t idx = (size_t)m * Cp + n;
        st4(vout + idx, v);
        const f32x4 x = ld4(xs + idx), a = ld4(alpha + n), r = ld4(inv + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * dac_snake_grad(x[e], a[e], r[e]);
        if (res) v = ld4(res + idx) + v;
        st4(out + idx, v);
    }
};

__device__ __forceinline__ double block_sum256d(double s, double* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k]; __syncthreads(); }
    const double r = red[0];
    __syncthreads();
    return r;
}

// Column sums of a channels-last (M, Cp) map over a row range per workgroup:  part[block][c] = sum_m v(m, c) * f(m, c), in fp64
//   ALPHA false: f = 1 (a bias gradient);  true: f = d snake / d alpha at the saved input xs(m, c), evaluated in fp32
// Workgroup (x, y) owns rows [x * rows, (x + 1) * rows) of the columns [y * cw, (y + 1) * cw), cw = min(Cp, 256); its 256 threads are
// nph = 256 / cw row phases of cw columns, a thread adds rows ph, ph + nph, ... of its column in order and the phases are added in the order
// 0..nph-1.  dac_reduce_cols_kernel adds the row ranges.
template <bool ALPHA>
__global__ __launch_bounds__(256) void dac_colsum_kernel(const float* __restrict__ v, const float* __restrict__ xs, const float* __restrict__ alpha,
                                                         const float* __restrict__ inv, long long M, int Cp, int rows, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int cw = min(Cp, 256), nph = 256 / cw;
    const int ph = threadIdx.x / cw, cx = threadIdx.x - ph * cw;
    const int c = blockIdx.y * cw + cx;
    const long long m0 = (long long)blockIdx.x * rows, m1 = min(M, m0 + rows);
    double s = 0.0;
    if (ph < nph && c < Cp) {
        float a = 0.f, r = 0.f;
        if (ALPHA) { a = alpha[c]; r = inv[c]; }
#pragma unroll 4
        for (long long m = m0 + ph; m < m1; m += nph) {
            const size_t idx = (size_t)m * Cp + c;
            s = s + (ALPHA ? (double)v[idx] * (double)dac_snake_grad_alpha(xs[idx], a, r) : (double)v[idx]);
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (ph == 0 && c < Cp) {
        double t = red[cx];
        for (int p = 1; p < nph; ++p) t = t + red[p * cw + cx];
        part[(size_t)blockIdx.x * Cp + c] = t;
    }
}

// out[i] = sum_k part[k * stride + i] for i < n: the row ranges' partial rows (a row is stride >= n values wide), rounded to fp32 once.  16 columns
// x 16 lanes per workgroup: lane (q, j) adds the ranges q, q + 16, ... of column j in order, lane q = 0 then adds the 16 sums in the order 0..15
// (a thread per column would walk up to 1024 partials as one chain of loads).
__global__ __launch_bounds__(256) void dac_reduce_cols_kernel(const double* __restrict__ part, int count, int stride, int n, float* __restrict__ out) {
    __shared__ double red[16][17];
    const int j = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int i = blockIdx.x * 16 + j;
    double s = 0.0;
    if (i < n) for (int k = q; k < count; k += 16) s += part[(size_t)k * stride + i];
    red[q][j] = s;
    __syncthreads();
    if (q == 0 && i < n) {
        double t = red[0][j];
#pragma unroll
        for (int r = 1; r < 16; ++r) t += red[r][j];
        out[i] = (float)t;
    }
}

// Weight norm backward (torch.nn.utils.weight_norm over every dimension but the first, nn/layers.py:5-10) from the staged gradient of the
// normalised weight, dW[i][tap * JP + j] with row stride Kp, to the raw parameters v (I, J, K) and g (I): one workgroup per i.
//   dg = <dW, v> / |v|        dv = g / |v| * (dW - <dW, v> v / |v|^2)
// <dW, v> and |v|^2 are summed in fp64 and rounded once; the elementwise part is fp32.
__global__ __launch_bounds__(256) void dac_wn_bwd_kernel(const float* __restrict__ dW, const float* __restrict__ v, const float* __restrict__ g,
                                                         float* __restrict__ dv, float* __restrict__ dg, int J, int K, int JP, int Kp) {
    const int i = blockIdx.x;
    __shared__ double red[256];
    const float* vr = v + (size_t)i * J * K;
    const float* dr = dW + (size_t)i * Kp;
    double s = 0.0, q = 0.0;
    for (int e = threadIdx.x; e < J * K; e += 256) {
        const int j = e / K, t = e - j * K;
        s += (double)vr[e] * (double)vr[e];
        q += (double)dr[t * JP + j] * (double)vr[e];
    }
    const double n2 = block_sum256d(s, red), dot = block_sum256d(q, red);
    const double nrm = sqrt(n2);
    if (threadIdx.x == 0) dg[i] = (float)(dot / nrm);
    const float sc = (float)((double)g[i] / nrm), c = (float)(dot / n2);
    for (int e = threadIdx.x; e < J * K; e += 256) {
        const int j = e / K, t = e - j * K;
        dv[(size_t)i * J * K + e] = sc * (dr[t * JP + j] - c * vr[e]);
    }
}

// ---- parameter gradients through the encoder and the quantiser (dac.py:24-91 ResidualUnit / EncoderBlock / Encoder, nn/quantize.py:58-70, 173-198,
// nn/layers.py:5-33), eval mode, padding on.  DESIGN.md section 13.7. --------------------------------------------------------------------------------
//
// DacGradPhaseEpi with v = conv^T(dY) also stored to a second map, as DacGradEpiV is to DacGradEpi: `out` has DacGradPhaseEpi's bits, and every
// input row lies in exactly one phase, so every row of vout is written too.
struct DacGradPhaseEpiV {
    static constexpr bool CHUNKED_K = true;
    float* out; const float* xs; const float* alpha; const float* inv; float* vout;            // vout aliases none of the others
    int Cp, Trows, Tmap, os, o0; FastDiv dT;
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (n >= Cp) return;
        const int b = dT.div(m), q = m - b * Trows;
        const size_t idx = ((size_t)b * Tmap + (size_t)q * os + o0) * Cp + n;
        st4(vout + idx, v);
        const f32x4 x = ld4(xs + idx), a = ld4(alpha + n), r = ld4(inv + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * dac_snake_grad(x[e], a[e], r[e]);
        st4(out + idx, v);
    }
};

// One stage of the quantiser's parameter backward, the row part: dac_rvq_grad_kernel's walk cut into one launch per stage, i = n - 1 .. 0, with
// g_r (the cotangent of the residual) carried between the launches in a (M, Dp) map that starts as zeros.  One wave per latent row (b, t); lane l
// owns the channels c = l + 64 j.  For a row whose clip runs stage i (i < n_b) the launch
//   rebuilds r_i = z_enc - sum_{k < i} (W_out_k q_k + b_out_k) with the forward's own operations (dac_rvq_kernel: the straight-through value
//   q_k = z_e_k + (C_k[code_k] - z_e_k), one fma chain over d, the stages subtracted in order), so r_i has the forward's bits;
//   forms u_i = g_z - g_r and e_i = W_out_i^T u_i + g_lat_i + g_cm 2 (z_e_i - C_i[code_i]) / (B d T) exactly as dac_rvq_grad_kernel does;
//   stores u_i and r_i as rows of the channels-last maps U and R (M, Dp), e_i and q_i as rows of E and Q (M, dp), pad channels zero;
//   advances g_r += W_in_i^T e_i.
// A row whose clip does not run stage i stores zero rows and leaves g_r alone.  u_i and r_i are formed directly, never as differences of sums
// over rows.  The contractions dW_out_i = U^T Q, dW_in_i = E^T R and the column sums db_out_i, db_in_i then go through gemm_dw_kernel and
// dac_colsum_kernel with one-tap operands.  Every sum runs in one fixed order; no atomics.
struct DacQParamArgs {
    const float* win; const float* wout; const float* bout; const float* cbraw;     // DacQTables: [S][d][D] [S][D][d] [S][D] [S][K][d]
    const float* g_z; const float* g_lat; const float* g_cm;
    const float* latents; const long long* codes; const int* clip_n;               // the tape's: (B, n d, T), (B, n, T), [B]
    const float* zmap;                                                              // z_enc (M, Dp)
    float* gr; float* U; float* R;                                                  // (M, Dp)
    float* E; float* Q;                                                             // (M, dp)
    int M, T, D, Dp, d, dp, K, n, B, stage;
};

template <int J>
__global__ __launch_bounds__(256) void dac_rvq_param_rows_kernel(DacQParamArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.M) return;                                     // wave-uniform
    const int b = row / a.T, t = row - b * a.T;
    const int D = a.D, d = a.d, K = a.K, i = a.stage;
    const size_t mrow = (size_t)row * a.Dp, drow = (size_t)row * a.dp;
    const int nb = max(0, min(a.clip_n[b], a.n));               // stages of this row
    if (i >= nb) {                                              // wave-uniform
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            if (c < a.Dp) { a.U[mrow + c] = 0.f; a.R[mrow + c] = 0.f; }
        }
        if (lane < a.dp) { a.E[drow + lane] = 0.f; a.Q[drow + lane] = 0.f; }
        return;
    }
    float res[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { const int c = lane + 64 * j; res[j] = c < D ? a.zmap[mrow + c] : 0.f; }
    float q[DAC_DMAX], ze[DAC_DMAX], raw[DAC_DMAX];
    for (int k = 0; k <= i; ++k) {
        long long code = a.codes[((size_t)b * a.n + k) * a.T + t];
        code = code < 0 ? 0 : (code >= K ? K - 1 : code);       // the tape is caller memory: never read outside the codebook
        const float* rw = a.cbraw + ((size_t)k * K + (size_t)code) * d;
        _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) {
            ze[jd] = a.latents[((size_t)b * a.n * d + (size_t)k * d + jd) * a.T + t];
            raw[jd] = rw[jd];
            q[jd] = ze[jd] + (raw[jd] - ze[jd]);
        }
        if (k == i) break;
        const float* wo = a.wout + (size_t)k * D * d;
        const float* bo = a.bout + (size_t)k * D;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            if (c >= D) continue;
            float s = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) s = fmaf(wo[(size_t)c * d + jd], q[jd], s);
            const float o = s + bo[c];
            res[j] = res[j] - o;
        }
    }
    const float gcm = a.g_cm ? a.g_cm[0] : 0.f;
    const float cms = 2.0f / ((float)a.B * (float)(d * a.T));
    const float* wo = a.wout + (size_t)i * D * d;
    const float* wi = a.win + (size_t)i * d * D;
    float u[J], gr[J], e[DAC_DMAX];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        gr[j] = c < D ? a.gr[mrow + c] : 0.f;
        const float gz = (a.g_z && c < D) ? a.g_z[((size_t)b * D + c) * a.T + t] : 0.f;
        u[j] = gz - gr[j];
    }
    _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) { const int c = lane + 64 * j; if (c < D) s = fmaf(wo[(size_t)c * d + jd], u[j], s); }
        s = wave_sum(s);
        const size_t li = ((size_t)b * a.n * d + (size_t)i * d + jd) * a.T + t;
        if (a.g_lat) s = s + a.g_lat[li];
        if (a.g_cm) s = s + (gcm * cms) * (ze[jd] - raw[jd]);
        e[jd] = s;
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c < D) {
            float s = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) s = fmaf(wi[(size_t)jd * D + c], e[jd], s);
            a.gr[mrow + c] = gr[j] + s;
        }
        if (c < a.Dp) { a.U[mrow + c] = c < D ? u[j] : 0.f; a.R[mrow + c] = c < D ? res[j] : 0.f; }
    }
    float el = 0.f, ql = 0.f;                                   // e[lane], q[lane] without a dynamic register index
#pragma unroll
    for (int jd = 0; jd < DAC_DMAX; ++jd) { el = (jd == lane && jd < d) ? e[jd] : el; ql = (jd == lane && jd < d) ? q[jd] : ql; }
    if (lane < a.dp) { a.E[drow + lane] = el; a.Q[drow + lane] = ql; }
}

// Codebook gradient (quantize.py:66, the codebook loss mse(z_q, z_e.detach()) summed over the stages and meaned over the clips):
//   dC_i[c] = g_cb * 2 / (B d T) * sum over the rows (b, t) with code_i = c and i < n_b of (C_i[c] - z_e_i(b, t))
// One wave per (stage, code).  The wave walks the code column of its stage 64 rows at a time; the rows that chose the code are added in increasing
// row order, lane jd < d owning component jd: the fp32 difference, accumulated in fp64 and rounded once after the scale.  A code no row chose gets
// exactly zero, and so does everything when g_cb is NULL.  No atomics.
__global__ __launch_bounds__(256) void dac_codebook_grad_kernel(const float* __restrict__ cbraw, const float* __restrict__ latents,
                                                                const long long* __restrict__ codes, const int* __restrict__ clip_n,
                                                                const float* __restrict__ g_cb, const long long* __restrict__ cb_offs, int M, int T, int d,
                                                                int K, int n, int B, float* __restrict__ grad) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)n * K) return;                          // wave-uniform
    const int i = (int)(w / K), c = (int)(w - (long long)i * K);
    float* out = grad + cb_offs[i] + (size_t)c * d;
    if (!g_cb) { if (lane < d) out[lane] = 0.f; return; }
    const float raw = lane < d ? cbraw[((size_t)i * K + c) * d + lane] : 0.f;
    double acc = 0.0;
    for (int m0 = 0; m0 < M; m0 += 64) {
        const int row = m0 + lane;
        bool hit = false;
        if (row < M) {
            const int b = row / T, t = row - b * T;
            long long code = codes[((size_t)b * n + i) * T + t];
            code = code < 0 ? 0 : (code >= K ? K - 1 : code);
            hit = i < max(0, min(clip_n[b], n)) && code == c;
        }
        unsigned long long mask = __ballot(hit);
        while (mask) {                                          // wave-uniform: the set bits in increasing order
            const int k = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int r = m0 + k, b = r / T, t = r - b * T;
            if (lane < d) acc += (double)(raw - latents[((size_t)b * n * d + (size_t)i * d + lane) * T + t]);
        }
    }
    if (lane < d) out[lane] = (float)(acc * ((double)g_cb[0] * 2.0 / ((double)B * (double)d * (double)T)));
}

}  // namespace escx
