// Device code of the latent gradient through the DAC baseline's decoder (reference: baselines/descript/dac/model/dac.py:249-266 DAC.decode,
// dac.py:24-41 ResidualUnit, dac.py:94-145 DecoderBlock / Decoder, nn/layers.py:9-33), eval mode, padding on.  DESIGN.md section 13.3.
//
// The backward of every convolution is an implicit GEMM on the fp32 MFMA engine with the forward's loader (DacConvA, no Snake) over the
// output gradient dY, a channels-last (B, Tout, CoutP) map:
//   dX of Conv1d (K taps, dilation d, padding p, stride 1)   A[(b, t)][k = tap * CoutP + co] = dY(b, t + p - tap * d, co):  rs = 1, r0 = p, td = -d
//   dX of ConvTranspose1d (stride s, 2s taps, padding p)     A[(b, t)][k = tap * CoutP + co] = dY(b, t * s - p + tap, co):  rs = s, r0 = -p, td = 1
// against the transposed weight image Wt[ci][tap * CoutP + co] that dac_wt_pack_kernel derives from the forward's packed, weight-normalised image
// (the same fp32 values, moved).  One output element is summed in one fixed order whatever the tile (gemm_engine.h CHUNKED_K: one fma chain per
// BK step, the steps added in order): no atomics, no split K.
//   DacGradEpi   out(b, t, n..n+3) = [res +] v * snake'(x_saved(b, t, n..n+3))      the Snake in front of the differentiated convolution
//                d_z(b, n + r, t) = v[r]   (xs == nullptr)                            the first convolution: (B, D, T) layout, no Snake in front
#pragma once
#include "dac_kernels.h"

namespace escx {

// d/dx (x + inv * sin(alpha x)^2) = 1 + inv * alpha * sin(2 alpha x), with the forward's inv table, the accurate sinf and no contraction into fma
__device__ __forceinline__ float dac_snake_grad(float x, float a, float inv) {
#pragma clang fp contract(off)
    const float s = sinf(2.0f * (a * x));
    return 1.0f + (inv * a) * s;
}
// d tanh / d v from the output y = tanh(v): 1 - y^2, one rounding (y^2 is within half an ulp of 1 where it matters)
__device__ __forceinline__ float dac_tanh_grad(float y) { return fmaf(-y, y, 1.0f); }

struct DacGradEpi {
    static constexpr bool CHUNKED_K = true;     // gemm_engine.h: the contractions here run to 7 * decoder_dim and 16 * decoder_dim / 2 terms
    float* out; const float* res; const float* xs; const float* alpha; const float* inv;       // res may alias out (same element read then written by one lane)
    int Cp, D, T; FastDiv dT;                                                                   // D, T, dT: the d_z form only
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (!xs) {
            const int b = dT.div(m), t = m - b * T;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < D) out[((size_t)b * D + n + r) * T + t] = v[r];
            return;
        }
        if (n >= Cp) return;
        const size_t idx = (size_t)m * Cp + n;                  // rows (b, t) of a (B, T, Cp) map are consecutive
        const f32x4 x = ld4(xs + idx), a = ld4(alpha + n), r = ld4(inv + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * dac_snake_grad(x[e], a[e], r[e]);
        if (res) v = ld4(res + idx) + v;
        st4(out + idx, v);
    }
};

// g_pre = d_audio * (1 - audio^2) as a (B, L, 4) map with zero pad channels: the output gradient of the one-channel last convolution
__global__ void dac_tanh_grad_in_kernel(const float* __restrict__ d_audio, const float* __restrict__ audio, float* __restrict__ out, long long n) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st4(out + 4 * i, f32x4{d_audio[i] * dac_tanh_grad(audio[i]), 0.f, 0.f, 0.f});
}

// Transposed image of one layer from its packed forward image W (dac_wn_conv_kernel: W[co][tap * CinP + ci];  dac_wn_convt_kernel:
// Wp[r][co][a * CinP + ci] with tap = a * s + k0, r = (k0 - p) mod s):  Wt[ci][tap * CoutP + co], row stride KpT, one thread per (ci, tap, co).
// The pad rows and columns of Wt are never written: they stay the zeros the buffer was allocated with.
__global__ void dac_wt_pack_kernel(const float* __restrict__ W, float* __restrict__ Wt, int kind, int Cin, int Cout, int K, int s, int p, int CinP,
                                   int CoutP, int Np, int Kp, int KpT) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)Cin * K * Cout) return;
    const int co = (int)(i % Cout); const long long ct = i / Cout;
    const int tap = (int)(ct % K), ci = (int)(ct / K);
    size_t src;
    if (kind == 0) src = (size_t)co * Kp + (size_t)tap * CinP + ci;
    else {
        const int a = tap / s, r = (((tap % s) - p) % s + s) % s;
        src = ((size_t)r * Np + co) * Kp + (size_t)a * CinP + ci;
    }
    Wt[(size_t)ci * KpT + (size_t)tap * CoutP + co] = W[src];
}

// The tape's header: what escx_dac_decode_backward checks before it launches anything
constexpr long long DAC_TAPE_MAGIC = 0x4553435844414354ll;      // "ESCXDACT"
constexpr int DAC_TAPE_HEADER = 64;                             // floats
__global__ void dac_tape_header_kernel(long long* __restrict__ hdr, long long version, long long B, long long T, long long floats) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { hdr[0] = DAC_TAPE_MAGIC; hdr[1] = version; hdr[2] = B; hdr[3] = T; hdr[4] = floats; }
}

// escx_dac_test_grad_math: the backward's Snake derivative (mode 0) and tanh derivative from the output (mode 1), elementwise
__global__ void dac_test_grad_math_kernel(const float* __restrict__ x, const float* __restrict__ alpha, float* __restrict__ out, long long n, int mode) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) { const float a = alpha[i]; out[i] = dac_snake_grad(x[i], a, 1.0f / (a + 1e-9f)); }
    else out[i] = dac_tanh_grad(x[i]);
}

}  // namespace escx
