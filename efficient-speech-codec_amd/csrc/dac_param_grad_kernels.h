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

}  // namespace escx
