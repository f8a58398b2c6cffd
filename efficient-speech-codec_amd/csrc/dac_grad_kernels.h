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

// ---- audio gradient through the encoder and the quantiser (dac.py:209-247 DAC.encode, dac.py:44-91 EncoderBlock / Encoder, nn/quantize.py:58-70,
// 173-198), eval mode, padding on.  DESIGN.md section 13.4. -----------------------------------------------------------------------------------------
//
// dX of the EncoderBlock's strided Conv1d (2s taps, stride s, padding p) is a transposed convolution: input row t = q s + r collects output rows
// q + c_r and q + c_r - 1 (c_r = floor((r + p) / s)) through the taps k0 = (r + p) mod s and k0 + s.  One GEMM per input phase r with two taps,
// the forward ConvTranspose1d's scheme: DacConvA over dY with rs = 1, r0 = c_r, td = -1 against the phase image below, and
//   DacGradPhaseEpi   out(b, q * os + o0, n..n+3) = v * snake'(x_saved(b, q * os + o0, n..n+3))
// Every input row lies in exactly one phase, so a row that no output tap covers is written too: its operand is zero and so is the product.
struct DacGradPhaseEpi {
    static constexpr bool CHUNKED_K = true;     // gemm_engine.h: contractions of 2 * 2 encoder_dim 2^i terms
    float* out; const float* xs; const float* alpha; const float* inv;
    int Cp, Trows, Tmap, os, o0; FastDiv dT;
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (n >= Cp) return;
        const int b = dT.div(m), q = m - b * Trows;
        const size_t idx = ((size_t)b * Tmap + (size_t)q * os + o0) * Cp + n;
        const f32x4 x = ld4(xs + idx), a = ld4(alpha + n), r = ld4(inv + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * dac_snake_grad(x[e], a[e], r[e]);
        st4(out + idx, v);
    }
};

// Transposed phase image of a strided Conv1d from its packed forward image W[co][tap * CinP + ci] (dac_wn_conv_kernel):
//   Wph[r][ci][a * CoutP + co] = W[co][(k0_r + a s) * CinP + ci],  k0_r = (r + p) mod s,  a in {0, 1};  row stride KpT, NpT rows per phase.
// One thread per (r, ci, a, co); the pad rows and columns stay the zeros the buffer was allocated with.
__global__ void dac_wt_phase_pack_kernel(const float* __restrict__ W, float* __restrict__ Wph, int Cin, int Cout, int s, int p, int CinP, int CoutP,
                                         int Kp, int NpT, int KpT) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)s * Cin * 2 * Cout) return;
    const int co = (int)(i % Cout); long long q = i / Cout;
    const int a = (int)(q % 2); q /= 2;
    const int ci = (int)(q % Cin), r = (int)(q / Cin);
    const int tap = (r + p) % s + a * s;
    Wph[((size_t)r * NpT + ci) * KpT + (size_t)a * CoutP + co] = W[(size_t)co * Kp + (size_t)tap * CinP + ci];
}

// Backward of the fused residual quantiser (quantize.py:58-70, 173-198 under autograd; forward: dac_rvq_kernel of dac_kernels.h), one launch.
// One wave per latent row (b, t); lane l owns the channels c = l + 64 j of g_r, the cotangent of the residual, in registers.  The stages run in
// reverse, i = n_b - 1 .. 0, from g_r = 0:
//   u   = g_z - g_r                                      cotangent of z_q_i (the straight-through estimator passes it to z_e_i unchanged)
//   e   = W_out_i^T u                                    lane-partial dot products, butterfly-summed across the wave
//   e  += g_lat_i + g_cm * 2 (z_e_i - raw_i[code]) / (B d T)        the commitment term of dac_loss_kernel's sum_i mean_b mean_{d,t}
//   g_r = g_r + W_in_i^T e                               rank-d update of the lane's channels
// The codebook loss detaches z_e and the codes are integers: neither contributes.  z_e_i, the codes and the per-clip stage counts come from the
// tape (a clip runs its own n_b stages; the slots past them gave zero latents and no loss term, so they get no gradient).  g_z (B, D, T) and
// g_lat (B, n d, T) may be NULL (zero); g_cm is a DEVICE scalar or NULL.  d_z_enc goes out channels-last (B, T, Dp) with zero pad channels: the dY
// of the encoder's last convolution.  Every sum runs in one fixed order; no atomics.
struct DacQGradArgs {
    const float* win; const float* wout; const float* cbraw;    // DacQTables: [S][d][D] [S][D][d] [S][K][d]
    const float* g_z; const float* g_lat; const float* g_cm;
    const float* latents; const long long* codes; const int* clip_n;   // the tape's: (B, n d, T), (B, n, T), [B]
    float* out;                                                 // (B, T, Dp)
    int M, T, D, Dp, d, K, n, B;
};

template <int J>
__global__ __launch_bounds__(256) void dac_rvq_grad_kernel(DacQGradArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.M) return;                                     // wave-uniform
    const int b = row / a.T, t = row - b * a.T;
    const int D = a.D, d = a.d, K = a.K;
    float gz[J], gr[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        gr[j] = 0.f;
        gz[j] = (a.g_z && c < D) ? a.g_z[((size_t)b * D + c) * a.T + t] : 0.f;
    }
    const float gcm = a.g_cm ? a.g_cm[0] : 0.f;
    const float cms = 2.0f / ((float)a.B * (float)(d * a.T));   // dac_loss_kernel: s / (d T), then the mean over the B clips of the call
    const int nb = max(0, min(a.clip_n[b], a.n));               // stages of this row
    for (int i = nb - 1; i >= 0; --i) {
        long long code = a.codes[((size_t)b * a.n + i) * a.T + t];
        code = code < 0 ? 0 : (code >= K ? K - 1 : code);       // the tape is caller memory: never read outside the codebook
        const float* raw = a.cbraw + ((size_t)i * K + (size_t)code) * d;
        const float* wo = a.wout + (size_t)i * D * d;
        const float* wi = a.win + (size_t)i * d * D;
        float u[J], e[DAC_DMAX];
#pragma unroll
        for (int j = 0; j < J; ++j) u[j] = gz[j] - gr[j];
        _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) { const int c = lane + 64 * j; if (c < D) s = fmaf(wo[(size_t)c * d + jd], u[j], s); }
            s = wave_sum(s);
            const size_t li = ((size_t)b * a.n * d + (size_t)i * d + jd) * a.T + t;
            if (a.g_lat) s = s + a.g_lat[li];
            if (a.g_cm) s = s + (gcm * cms) * (a.latents[li] - raw[jd]);
            e[jd] = s;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            if (c >= D) continue;
            float s = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) s = fmaf(wi[(size_t)jd * D + c], e[jd], s);
            gr[j] = gr[j] + s;
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c < a.Dp) a.out[((size_t)b * a.T + t) * a.Dp + c] = c < D ? gr[j] : 0.f;
    }
}

// The encode tape's header and its per-clip stage counts (clip_n == nullptr: every clip runs n stages)
constexpr long long DAC_ENC_TAPE_MAGIC = 0x4553435844414345ll;  // "ESCXDACE"
__global__ void dac_enc_tape_header_kernel(long long* __restrict__ hdr, long long version, long long B, long long L, long long floats, long long n,
                                           const int* __restrict__ clip_n, int* __restrict__ counts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { hdr[0] = DAC_ENC_TAPE_MAGIC; hdr[1] = version; hdr[2] = B; hdr[3] = L; hdr[4] = floats; hdr[5] = n; }
    if (i < B) counts[i] = clip_n ? clip_n[i] : (int)n;
}

// escx_dac_test_grad_math: the backward's Snake derivative (mode 0) and tanh derivative from the output (mode 1), elementwise
__global__ void dac_test_grad_math_kernel(const float* __restrict__ x, const float* __restrict__ alpha, float* __restrict__ out, long long n, int mode) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) { const float a = alpha[i]; out[i] = dac_snake_grad(x[i], a, 1.0f / (a + 1e-9f)); }
    else out[i] = dac_tanh_grad(x[i]);
}

// The stand-alone quantiser's d_z (quantize.py:127-198 under autograd, differentiated in its input): dac_rvq_grad_kernel's channels-last
// (B, T, Dp) gradient map stored in the caller's (B, D, T) layout.  The mirror of dac_z_in_kernel: one thread per output element, the stores
// coalesced along t; a copy, so no arithmetic and no order to fix.
__global__ void dac_z_out_kernel(const float* __restrict__ g, float* __restrict__ out, int B, int D, int Dp, int T) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * D * T) return;
    const int t = (int)(i % T); const long long bc = i / T; const int c = (int)(bc % D), b = (int)(bc / D);
    out[i] = g[((size_t)b * T + t) * Dp + c];
}

}  // namespace escx
