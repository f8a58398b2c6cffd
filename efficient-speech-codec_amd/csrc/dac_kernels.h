// Device code of the DAC baseline codec's inference path (reference: baselines/descript/dac/model/dac.py, nn/layers.py, nn/quantize.py).
//
// Feature maps are channels-last (B, T, Cp) fp32 buffers, Cp = rup(C, 4) with zero pad channels.  Every convolution is an implicit GEMM on the
// fp32 MFMA engine of gemm_engine.h:
//   DacConvA   A[(b, t)][k = tap * Cp + c] = snake?(X(b, t * rs + r0 + tap * td, c))     zero outside [0, Tin)
//              Conv1d:           rs = stride, r0 = -padding, td = dilation
//              ConvTranspose1d:  one GEMM per output phase r (t_out = q * s + r): rs = 1, r0 = floor((r + p) / s), td = -1, two taps
//              (p is the padding in effect: the layer's own, or 0 for every layer when the handle's padding is off)
//   DacEpi     out(b, t * os + o0, n..n+3) = [res +] (v + bias)   or   audio(b, t) = tanh(v + bias) for the one-channel last layer
//   DacEpiCrop out(b, t, n..n+3) = res(b, t + off, n..n+3) + (v + bias): the ResidualUnit's cropped skip when the padding is off
//   DacConvALen / DacEpiLen: the same two for a batch with per-clip lengths (a table of rows per clip instead of one Tin / Tout); DESIGN.md section 13.6
// Snake (nn/layers.py:19-24) is applied to the operand while it is staged: x + inv * sin(alpha * x)^2 with inv = 1 / (alpha + 1e-9) derived
// once per parameter version, in the reference's operation order, with the accurate sinf and no contraction into fma.
#pragma once
#include <hip/hip_runtime.h>
#include "gemm_engine.h"

namespace escx {

__device__ __forceinline__ float dac_snake(float x, float a, float inv) {
#pragma clang fp contract(off)
    const float s = sinf(a * x);
    return x + inv * (s * s);
}

struct DacConvA {
    const float* x; const float* alpha; const float* inv;      // alpha == nullptr: no Snake on this operand
    int Tin, Cp, Trows, rs, r0, td, ntaps, M; FastDiv dT, dCp;
    struct Ctx { int ok, tb; unsigned base; };
    __device__ __forceinline__ Ctx make_ctx(int m) const {
        Ctx c; c.ok = 0; c.tb = 0; c.base = 0;
        if (m < M) { const int b = dT.div(m); const int t = m - b * Trows; c.ok = 1; c.tb = t * rs + r0; c.base = (unsigned)b * (unsigned)Tin * (unsigned)Cp; }
        return c;
    }
    __device__ __forceinline__ f32x4 load4(const Ctx& c, int k0, int kin) const {
        const int k = k0 + kin;                 // Cp is a multiple of 4: the four values share one tap
        const int tap = dCp.div(k), cc = k - tap * Cp;
        const int ti = c.tb + tap * td;
        if (!c.ok || tap >= ntaps || (unsigned)ti >= (unsigned)Tin) return zero4();
        f32x4 v = ld4(x + c.base + (unsigned)ti * (unsigned)Cp + (unsigned)cc);
        if (alpha) {
            const f32x4 a = ld4(alpha + cc), r = ld4(inv + cc);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = dac_snake(v[e], a[e], r[e]);
        }
        return v;
    }
};

struct DacEpi {
    float* out; const float* bias; const float* res;           // res may alias out (same element read then written by one lane)
    int Cp, Trows, Tmap, os, o0, tanh_out; FastDiv dT;
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (n >= Cp) return;
        const int b = dT.div(m), t = m - b * Trows;
        const int to = t * os + o0;
        if (tanh_out) {                                         // one output channel: audio (B, Tmap)
            if (n == 0) out[(size_t)b * Tmap + to] = tanhf(v[0] + bias[0]);
            return;
        }
        v += ld4(bias + n);
        const size_t idx = ((size_t)b * Tmap + to) * Cp + n;
        if (res) v = ld4(res + idx) + v;
        st4(out + idx, v);
    }
};

// The residual add of a ResidualUnit whose convolutions run without padding (CodecMixin.padding = False, dac.py:35-40): the 7-tap convolution at
// dilation d loses 6d rows, so the skip input is read `off` = 3d rows further in, from a map with its own rows-per-clip count:
//   out(b, t, n..n+3) = res(b, t + off, n..n+3) + (v + bias)        t < Trows, t + off < Tres
// A type of its own: DacEpi, and with it every kernel of the padded path, stays what it is.  `res` must NOT alias `out`: a lane reads row t + off
// of a map of which another workgroup writes row t.  The host writes into the free map and swaps (dac.hip run_res).
struct DacEpiCrop {
    float* out; const float* bias; const float* res;
    int Cp, Trows, Tres, off; FastDiv dT;
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (n >= Cp) return;
        const int b = dT.div(m), t = m - b * Trows;
        v += ld4(bias + n);
        v = ld4(res + ((size_t)b * Tres + t + off) * Cp + n) + v;
        st4(out + ((size_t)b * Trows + t) * Cp + n, v);
    }
};

// Mixed-length batches (escx_dac_encode_lengths / escx_dac_decode_lengths; padding on): the maps keep their padded (B, Tmax, Cp) layout and clip b
// owns the rows t < tin[b] of the input map and t_out < tout[b] of the output map.  A row of the GEMM is live when its output row
// t_out = t * os + o0 lies inside its clip (os = 1, o0 = 0 for a Conv1d; os = stride, o0 = phase for a ConvTranspose1d phase GEMM, whose rows per clip
// Q_b = ceil((tout[b] - phase) / stride) are exactly the t with t * os + o0 < tout[b]).  A live row zero-fills outside [0, tin[b]): what DacConvA does
// for that clip alone with Tin = tin[b], tap for tap, so a live row sees the operands, and the MFMA sequence, of the call on its clip alone.  A dead
// row is staged as zeros and never stored; the rows past a clip's length hold stale scratch that no loader reads.  Types of their own: DacConvA and
// DacEpi, and with them every kernel of the uniform paths, stay what they are.
struct DacConvALen {
    static constexpr bool SKIPS_DEAD_TILES = true;             // gemm_engine.h: a workgroup without a live row returns before its first load
    const float* x; const float* alpha; const float* inv;      // alpha == nullptr: no Snake on this operand
    const int* tin; const int* tout;                           // [B] rows of clip b in the input map / in the layer's output map
    int Tin, Cp, Trows, rs, r0, td, ntaps, M, os, o0;          // Tin, Trows: the padded maps' rows per clip
    int keep_dead;                                             // the tanh layer: its epilogue zeroes the audio past a clip's length, so no tile is skipped
    FastDiv dT, dCp;
    struct Ctx { int tb, tin; unsigned base; };                // tin == 0: a dead row (or one behind M); every tap then fails the bounds test
    __device__ __forceinline__ Ctx make_ctx(int m) const {
        Ctx c; c.tb = 0; c.tin = 0; c.base = 0;
        if (m < M) {
            const int b = dT.div(m); const int t = m - b * Trows;
            if (t * os + o0 < tout[b]) { c.tb = t * rs + r0; c.tin = tin[b]; c.base = (unsigned)b * (unsigned)Tin * (unsigned)Cp; }
        }
        return c;
    }
    __device__ __forceinline__ int row_live(const Ctx& c) const { return c.tin | keep_dead; }
    __device__ __forceinline__ f32x4 load4(const Ctx& c, int k0, int kin) const {
        const int k = k0 + kin;                 // Cp is a multiple of 4: the four values share one tap
        const int tap = dCp.div(k), cc = k - tap * Cp;
        const int ti = c.tb + tap * td;
        if (tap >= ntaps || (unsigned)ti >= (unsigned)c.tin) return zero4();
        f32x4 v = ld4(x + c.base + (unsigned)ti * (unsigned)Cp + (unsigned)cc);
        if (alpha) {
            const f32x4 a = ld4(alpha + cc), r = ld4(inv + cc);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = dac_snake(v[e], a[e], r[e]);
        }
        return v;
    }
};

// DacEpi for the live rows only; the one-channel tanh layer writes 0 to the audio past a clip's length (its launch keeps the dead tiles).
struct DacEpiLen {
    float* out; const float* bias; const float* res;           // res may alias out (same element read then written by one lane)
    const int* tout;                                           // [B] rows of clip b in the output map
    int Cp, Trows, Tmap, os, o0, tanh_out; FastDiv dT;
    __device__ __forceinline__ void store(int m, int n, f32x4 v, int) const {
#pragma clang fp contract(off)
        if (n >= Cp) return;
        const int b = dT.div(m), t = m - b * Trows;
        const int to = t * os + o0;
        const bool live = to < tout[b];
        if (tanh_out) {                                         // one output channel: audio (B, Tmap)
            if (n == 0) out[(size_t)b * Tmap + to] = live ? tanhf(v[0] + bias[0]) : 0.f;
            return;
        }
        if (!live) return;
        v += ld4(bias + n);
        const size_t idx = ((size_t)b * Tmap + to) * Cp + n;
        if (res) v = ld4(res + idx) + v;
        st4(out + idx, v);
    }
};

// ------------------------------------------------------------------------------------------------
// Weight normalisation (torch.nn.utils.weight_norm: w = v * (g / ||v||), the norm over every dim but `dim`), packed for the engine.
// Conv1d (dim 0 = output channels): one workgroup per output channel, W[co][tap * CinP + ci].
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum256(float s, float* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k]; __syncthreads(); }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void dac_wn_conv_kernel(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ b,
                                                          float* __restrict__ W, float* __restrict__ bias, int Cin, int K, int CinP, int Kp) {
    const int co = blockIdx.x;
    __shared__ float red[256];
    const float* vr = v + (size_t)co * Cin * K;
    float s = 0.f;
    for (int i = threadIdx.x; i < Cin * K; i += 256) s += vr[i] * vr[i];
    const float sc = g[co] / sqrtf(block_sum256(s, red));
    if (threadIdx.x == 0) bias[co] = b[co];
    for (int i = threadIdx.x; i < Cin * K; i += 256) {
        const int ci = i / K, t = i - ci * K;
        W[(size_t)co * Kp + t * CinP + ci] = vr[i] * sc;
    }
}

// ConvTranspose1d (weight (Cin, Cout, 2s), dim 0 = INPUT channels): one workgroup per input channel.  Phase r of the output takes taps
// k0 = (r + p) mod s (a = 0, input q + c_r) and k0 + s (a = 1, input q + c_r - 1):  Wp[r][co][a * CinP + ci], Kp per phase.
__global__ __launch_bounds__(256) void dac_wn_convt_kernel(const float* __restrict__ v, const float* __restrict__ g, float* __restrict__ Wp,
                                                           int Cout, int s, int p, int CinP, int CoutN, int Kp) {
    const int ci = blockIdx.x;
    __shared__ float red[256];
    const int K = 2 * s;
    const float* vr = v + (size_t)ci * Cout * K;
    float sum = 0.f;
    for (int i = threadIdx.x; i < Cout * K; i += 256) sum += vr[i] * vr[i];
    const float sc = g[ci] / sqrtf(block_sum256(sum, red));
    for (int i = threadIdx.x; i < Cout * K; i += 256) {
        const int co = i / K, kk = i - co * K;
        const int a = kk / s, r = (((kk % s) - p) % s + s) % s;
        Wp[((size_t)r * CoutN + co) * Kp + a * CinP + ci] = vr[i] * sc;
    }
}

__global__ void dac_snake_pack_kernel(const float* __restrict__ alpha, float* __restrict__ a, float* __restrict__ inv, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) { const float x = alpha[c]; a[c] = x; inv[c] = 1.0f / (x + 1e-9f); }
}

// ------------------------------------------------------------------------------------------------
// Quantiser tables, per stage i: in_proj (d x D), out_proj (D x d) weight-normalised; codebook raw, F.normalize'd, and its squared norms.
// ------------------------------------------------------------------------------------------------
struct DacQTables {
    float* win; float* bin; float* wout; float* bout; float* cbraw; float* cbn; float* c2;      // [S][d][D] [S][d] [S][D][d] [S][D] [S][K][d] [S][K][d] [S][K]
};

// in_proj: one workgroup per (stage, output row j < d): norm over D
// offs: per stage the flat-buffer offsets of in_proj (bias, weight_g, weight_v), out_proj (bias, weight_g, weight_v), then one codebook per stage
__global__ __launch_bounds__(256) void dac_wn_inproj_kernel(const float* __restrict__ flat, const long long* __restrict__ offs, DacQTables t, int D, int d) {
    const int i = blockIdx.x / d, j = blockIdx.x - i * d;
    const float* bias = flat + offs[6 * i + 0]; const float* g = flat + offs[6 * i + 1]; const float* v = flat + offs[6 * i + 2];
    __shared__ float red[256];
    float s = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) s += v[(size_t)j * D + c] * v[(size_t)j * D + c];
    const float sc = g[j] / sqrtf(block_sum256(s, red));
    for (int c = threadIdx.x; c < D; c += 256) t.win[((size_t)i * d + j) * D + c] = v[(size_t)j * D + c] * sc;
    if (threadIdx.x == 0) t.bin[i * d + j] = bias[j];
}

// out_proj (norm over d per output row), codebook normalisation: one thread per (stage, row)
__global__ void dac_qtables_kernel(const float* __restrict__ flat, const long long* __restrict__ offs, DacQTables t, int S, int D, int d, int K) {
#pragma clang fp contract(off)
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long nout = (long long)S * D;
    if (idx < nout) {
        const int i = (int)(idx / D), c = (int)(idx - (long long)i * D);
        const float* bias = flat + offs[6 * i + 3]; const float* g = flat + offs[6 * i + 4]; const float* v = flat + offs[6 * i + 5];
        float s = 0.f;
        for (int j = 0; j < d; ++j) s += v[(size_t)c * d + j] * v[(size_t)c * d + j];
        const float sc = g[c] / sqrtf(s);
        for (int j = 0; j < d; ++j) t.wout[((size_t)i * D + c) * d + j] = v[(size_t)c * d + j] * sc;
        t.bout[(size_t)i * D + c] = bias[c];
        return;
    }
    const long long r = idx - nout;
    if (r >= (long long)S * K) return;
    const int i = (int)(r / K), k = (int)(r - (long long)i * K);
    const float* row = flat + offs[6 * S + i] + (size_t)k * d;
    float s = 0.f;
    for (int j = 0; j < d; ++j) s += row[j] * row[j];
    const float den = fmaxf(sqrtf(s), 1e-12f);                  // F.normalize: x / max(||x||, eps)
    float s2 = 0.f;
    for (int j = 0; j < d; ++j) {
        const float q = row[j] / den;
        t.cbraw[((size_t)i * K + k) * d + j] = row[j];
        t.cbn[((size_t)i * K + k) * d + j] = q;
        s2 += q * q;
    }
    t.c2[(size_t)i * K + k] = s2;
}

// ------------------------------------------------------------------------------------------------
// Fused residual vector quantiser (quantize.py:127-198, eval): one wave per latent row (b, t), all n stages in one launch.
// Lane l owns the latent channels c = l + 64 j (j < J) of the running sum z_q and the residual, in registers.  Per stage:
//   z_e = in_proj(residual)      lane-partial dot products, butterfly-summed across the wave; written to `latents`
//   e = z_e / max(||z_e||, 1e-12);  dist_k = (sum e^2 - 2 e.c_k) + sum c_k^2 over the normalised codebook; first minimal index wins
//   q = z_e + (raw_k - z_e)      the straight-through value of quantize.py:64-68 (not bitwise raw_k)
//   o = out_proj(q);  z_q += o;  residual -= o;  sum_j (z_e - raw_k)^2 goes to the per-(stage, row) loss slot
// The codebook-dimension loops run to DAC_DMAX with a guard, so ze / e / q stay in registers (the order of the operations is that of the d-loop).
// FROM_CODES: z_q = sum over stages, in stage order from 0, of out_proj(raw_{code}) (quantize.py:200-220); z_p gets the raw rows.
// EXT selects one optional input (never both); DAC_Q_PLAIN is the kernel without either, instruction for instruction:
//   DAC_Q_CLIPS  clip_n[b] stages for the rows of clip b (the per-item mask of quantize.py:181-190; wave-uniform, a wave owns one row).  The
//                slots clip_n[b] <= i < n get code -1, zero latents and a zero loss term, so dac_loss_kernel's sum_i mean_b is the reference's
//                masked mean.  FROM_CODES never reads those slots and writes zero z_p there.
//   DAC_Q_SNAPS  after stage i with i + 1 == snap_n[r] the running sum goes to zsnap[r] (B, D, T) with the store pattern of the final z:
//                the same registers at the same point of the same sum as a call that stops at n = snap_n[r].
//   DAC_Q_LEN    a flag on top of DAC_Q_PLAIN or DAC_Q_CLIPS (EXT = DAC_Q_LEN | DAC_Q_CLIPS): frame_len[b] frames of clip b.  A row at or past its
//                clip's length is a row with zero stages: nothing of it is read (not zmap, not codes_in), z and latents / z_p get 0 and codes -1
//                in every slot.  Without the flag the kernels are what they were, name and instructions.
// ------------------------------------------------------------------------------------------------
constexpr int DAC_DMAX = 8;
constexpr int DAC_Q_PLAIN = 0, DAC_Q_CLIPS = 1, DAC_Q_SNAPS = 2, DAC_Q_LEN = 4;

struct DacQArgs {
    DacQTables t;
    const float* zmap;              // encoder output (B, T, Dp) channels-last (encode form)
    const long long* codes_in;      // (B, n, T) (from_codes form)
    float* z;                       // (B, D, T)
    long long* codes;               // (B, n, T)
    float* latents;                 // (B, n * d, T)  (from_codes form: z_p)
    float* loss;                    // [n][M] squared-error sums
    int M, T, D, Dp, d, K, n;
    const int* clip_n;              // DAC_Q_CLIPS: [B] stage counts, each in [1, n]
    const int* snap_n;              // DAC_Q_SNAPS: [n_snaps] strictly increasing stage counts in [1, n]
    float* zsnap;                   // DAC_Q_SNAPS: (n_snaps, B, D, T)
    int n_snaps;
    const int* frame_len;           // DAC_Q_LEN: [B] frames per clip, each in [1, T]
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int J, bool FROM_CODES, int EXT_ = DAC_Q_PLAIN>
__global__ __launch_bounds__(256) void dac_rvq_kernel(DacQArgs a) {
#pragma clang fp contract(off)
    constexpr int EXT = EXT_ & ~DAC_Q_LEN;
    constexpr bool LEN = (EXT_ & DAC_Q_LEN) != 0;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.M) return;                                     // wave-uniform
    const int b = row / a.T, t = row - b * a.T;
    const int D = a.D, d = a.d, K = a.K;
    [[maybe_unused]] bool live = true;                          // wave-uniform
    if constexpr (LEN) live = t < a.frame_len[b];
    float zq[J], res[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        zq[j] = 0.f;
        if constexpr (LEN) res[j] = (!FROM_CODES && c < D && live) ? a.zmap[((size_t)b * a.T + t) * a.Dp + c] : 0.f;
        else res[j] = (!FROM_CODES && c < D) ? a.zmap[((size_t)b * a.T + t) * a.Dp + c] : 0.f;
    }
    int nb = a.n;                                               // stages of this row
    if constexpr (EXT == DAC_Q_CLIPS) nb = max(0, min(a.clip_n[b], a.n));
    if constexpr (LEN) nb = live ? nb : 0;
    [[maybe_unused]] int snap = 0;
    for (int i = 0; i < nb; ++i) {
        float q[DAC_DMAX];
        int best = 0;
        if constexpr (FROM_CODES) {
            long long code = a.codes_in[((size_t)b * a.n + i) * a.T + t];
            best = (int)(code < 0 ? 0 : (code >= K ? K - 1 : code));       // a corrupt index must not read outside the codebook
            const float* raw = a.t.cbraw + ((size_t)i * K + best) * d;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) q[jd] = raw[jd];
            if (lane < d) a.latents[((size_t)b * a.n * d + (size_t)i * d + lane) * a.T + t] = raw[lane];
        } else {
            float ze[DAC_DMAX];
            const float* w = a.t.win + (size_t)i * d * D;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < J; ++j) { const int c = lane + 64 * j; if (c < D) s = fmaf(w[(size_t)jd * D + c], res[j], s); }
                ze[jd] = wave_sum(s) + a.t.bin[i * d + jd];
            }
            float nn = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) nn += ze[jd] * ze[jd];
            const float den = fmaxf(sqrtf(nn), 1e-12f);
            float e[DAC_DMAX], e2 = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) { e[jd] = ze[jd] / den; e2 += e[jd] * e[jd]; }
            float bd = INFINITY; best = 0x7fffffff;
            const float* cbn = a.t.cbn + (size_t)i * K * d;
            const float* c2 = a.t.c2 + (size_t)i * K;
            for (int k = lane; k < K; k += 64) {
                float dot = 0.f;
                _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) dot = fmaf(e[jd], cbn[(size_t)k * d + jd], dot);
                const float dist = (e2 - 2.f * dot) + c2[k];
                if (dist < bd) { bd = dist; best = k; }                          // k rises per lane: the first minimum stays
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float od = __shfl_xor(bd, o, 64); const int ok = __shfl_xor(best, o, 64);
                if (od < bd || (od == bd && ok < best)) { bd = od; best = ok; }
            }
            if (best == 0x7fffffff) best = 0;                                   // every distance NaN
            const float* raw = a.t.cbraw + ((size_t)i * K + best) * d;
            float se = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) {
                const float r = raw[jd];
                const float df = ze[jd] - r;
                se += df * df;
                q[jd] = ze[jd] + (r - ze[jd]);
            }
            float zl = 0.f;                                                     // ze[lane] without a dynamic register index
#pragma unroll
            for (int jd = 0; jd < DAC_DMAX; ++jd) zl = jd == lane ? ze[jd] : zl;
            if (lane < d) a.latents[((size_t)b * a.n * d + (size_t)i * d + lane) * a.T + t] = zl;
            if (lane == 0) { a.codes[((size_t)b * a.n + i) * a.T + t] = best; a.loss[(size_t)i * a.M + row] = se; }
        }
        const float* wo = a.t.wout + (size_t)i * D * d;
        const float* bo = a.t.bout + (size_t)i * D;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = lane + 64 * j;
            if (c >= D) continue;
            float s = 0.f;
            _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) s = fmaf(wo[(size_t)c * d + jd], q[jd], s);
            const float o = s + bo[c];
            zq[j] = zq[j] + o;
            res[j] = res[j] - o;
        }
        if constexpr (EXT == DAC_Q_SNAPS) {
            if (snap < a.n_snaps && i + 1 == a.snap_n[snap]) {                  // wave-uniform
                float* zs = a.zsnap + (size_t)snap * a.M * D;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const int c = lane + 64 * j;
                    if (c < D) zs[((size_t)b * D + c) * a.T + t] = zq[j];
                }
                ++snap;
            }
        }
    }
    if constexpr (EXT == DAC_Q_CLIPS || LEN) {
        for (int i = nb; i < a.n; ++i) {                                        // the slots past this clip's count (LEN: every slot of a dead row)
            if (lane < d) a.latents[((size_t)b * a.n * d + (size_t)i * d + lane) * a.T + t] = 0.f;
            if constexpr (!FROM_CODES) if (lane == 0) { a.codes[((size_t)b * a.n + i) * a.T + t] = -1; a.loss[(size_t)i * a.M + row] = 0.f; }
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = lane + 64 * j;
        if (c < D) a.z[((size_t)b * D + c) * a.T + t] = zq[j];
    }
}

// losses: out[0] = commitment, out[1] = codebook = sum_i mean_b (sum_t loss[i][b, t] / (d T))   (both MSE terms are the same values in eval).
// One workgroup: per-(stage, clip) means into perclip, then one lane adds them in the reference's order.
__global__ __launch_bounds__(256) void dac_loss_kernel(const float* __restrict__ loss, float* __restrict__ perclip, float* __restrict__ out, int B, int T, int n, int d) {
    for (int p = threadIdx.x; p < n * B; p += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += loss[(size_t)p * T + t];
        perclip[p] = s / (float)(d * T);
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    float tot = 0.f;
    for (int i = 0; i < n; ++i) {
        float mb = 0.f;
        for (int b = 0; b < B; ++b) mb += perclip[i * B + b];
        tot += mb / (float)B;
    }
    out[0] = tot; out[1] = tot;
}

// dac_loss_kernel for a batch with per-clip lengths: clip b's mean runs over its own frames t < tl[b], in the order and with the divisor of the call
// on that clip alone; the slots of the rows past them are never read.
__global__ __launch_bounds__(256) void dac_loss_len_kernel(const float* __restrict__ loss, float* __restrict__ perclip, float* __restrict__ out, int B, int T, int n,
                                                           int d, const int* __restrict__ tl) {
    for (int p = threadIdx.x; p < n * B; p += 256) {
        const int Tb = tl[p % B];
        float s = 0.f;
        for (int t = 0; t < Tb; ++t) s += loss[(size_t)p * T + t];
        perclip[p] = s / (float)(d * Tb);
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    float tot = 0.f;
    for (int i = 0; i < n; ++i) {
        float mb = 0.f;
        for (int b = 0; b < B; ++b) mb += perclip[i * B + b];
        tot += mb / (float)B;
    }
    out[0] = tot; out[1] = tot;
}

// Snaked copy of a (rows, Cp) map: the same dac_snake per element as the on-load form, so the GEMM reads bitwise the same operand
__global__ void dac_snake_map_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ inv, float* __restrict__ out,
                                     long long n4, int cp4) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const int c = 4 * (int)(i % cp4);
    f32x4 v = ld4(x + 4 * i);
    const f32x4 a = ld4(alpha + c), r = ld4(inv + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = dac_snake(v[e], a[e], r[e]);
    st4(out + 4 * i, v);
}

// escx_dac_test_math: the device Snake (mode 0) and tanh (mode 1) of the kernels, elementwise
__global__ void dac_test_math_kernel(const float* __restrict__ x, const float* __restrict__ alpha, float* __restrict__ out, long long n, int mode) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (mode == 0) { const float a = alpha[i]; out[i] = dac_snake(x[i], a, 1.0f / (a + 1e-9f)); }
    else out[i] = tanhf(x[i]);
}

// (B, 1, L) audio -> (B, L, 4) map with zero pad channels;  (B, D, T) -> (B, T, Dp)
__global__ void dac_wave_in_kernel(const float* __restrict__ x, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) st4(out + 4 * i, f32x4{x[i], 0.f, 0.f, 0.f});
}
// Mixed-length batch: (B, 1, Lsrc) audio -> (B, Lmap, 4) map; sample s of clip b is read only for s < len[b] and staged as 0 from there on (the clip's
// right-pad to a multiple of the hop, dac.py:198-207, and everything behind it: nothing at or past a clip's length is read, whatever it holds)
__global__ void dac_wave_in_len_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, int Lsrc, int Lmap, const int* __restrict__ len) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = (int)(i / Lmap), s = (int)(i - (long long)b * Lmap);
    const float v = s < len[b] ? x[(size_t)b * Lsrc + s] : 0.f;
    st4(out + 4 * i, f32x4{v, 0.f, 0.f, 0.f});
}
// Chunked compress (base.py:197, 206-208) without the host's copies: the (rows * n_chunks, n_samples, 4) map of overlapping windows straight from
// the (rows, n_signal) signal.  Sample j of chunk c of row r is signal[r][c * hop + j - lead], zero outside [0, n_signal): the reference's
// zero_pad(delay, delay), its slice [c hop, c hop + n_samples) and the right zero-pad of a short last slice, with lead = delay.
__global__ void dac_chunk_in_kernel(const float* __restrict__ sig, float* __restrict__ out, long long n, long long n_signal, int n_chunks, int n_samples,
                                    int hop, long long lead) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long rc = i / n_samples;
    const int j = (int)(i - rc * n_samples);
    const long long r = rc / n_chunks, c = rc - r * n_chunks;
    const long long src = c * hop + j - lead;
    const float v = (src >= 0 && src < n_signal) ? sig[r * n_signal + src] : 0.f;
    st4(out + 4 * i, f32x4{v, 0.f, 0.f, 0.f});
}
__global__ void dac_z_in_kernel(const float* __restrict__ z, float* __restrict__ out, int B, int D, int Dp, int T) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * T * Dp) return;
    const int c = (int)(i % Dp); const long long bt = i / Dp; const int t = (int)(bt % T), b = (int)(bt / T);
    out[i] = c < D ? z[((size_t)b * D + c) * T + t] : 0.f;
}
// dac_z_in_kernel for a mixed-length batch: frame t of clip b is read only for t < tl[b] and staged as 0 from there on
__global__ void dac_z_in_len_kernel(const float* __restrict__ z, float* __restrict__ out, int B, int D, int Dp, int T, const int* __restrict__ tl) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * T * Dp) return;
    const int c = (int)(i % Dp); const long long bt = i / Dp; const int t = (int)(bt % T), b = (int)(bt / T);
    out[i] = (c < D && t < tl[b]) ? z[((size_t)b * D + c) * T + t] : 0.f;
}

// ------------------------------------------------------------------------------------------------
// Independent codebook search of ResidualVectorQuantize.from_latents (quantize.py:222-255 over VectorQuantize.decode_latents, quantize.py:78-94):
// stage i looks up its own d channels of per-codebook latents (B, C, T) that something else predicted; there is no residual chain, so the n stages
// of a row are n independent searches.  One wave per (stage, latent row) pair, stage-major (wave w: stage w / M, row w % M), so the four waves of
// a workgroup and its neighbours scan the same codebook.  Every lane reads the row's d channels straight from the (B, C, T) layout (one address
// per channel across the wave: a broadcast), then repeats dac_rvq_kernel's search on them operation for operation: the normalisation
// e = z_e / max(||z_e||, 1e-12), dist_k = (sum e^2 - 2 e.c_k) + sum c_k^2 with the dot product as one fma chain over d, the lane-strided scan
// in which the first minimum stays, the butterfly that prefers the lower index, code 0 when every distance is NaN.  No contraction into fma
// outside the explicit chain, so the codes are bitwise the ones dac_rvq_kernel emits for the same latents.  No LDS, no atomics.
// clip_n / frame_len ([B] or nullptr): a slot at or past its clip's stage count, and every slot of a row at or past its clip's frame count, is a
// wave-uniform early exit that writes -1 and reads nothing.  Only the codes are written: z_p and z_q come from dac_rvq_kernel<.., FROM_CODES>.
// ------------------------------------------------------------------------------------------------
struct DacSearchArgs {
    const float* cbn; const float* c2;      // DacQTables: [S][K][d] normalised rows, [S][K] their squared norms
    const float* latents;                   // (B, C, T), stage i in the channels [i d, (i + 1) d)
    long long* codes;                       // (B, n, T)
    const int* clip_n;                      // [B] stage counts, each in [1, n], or nullptr
    const int* frame_len;                   // [B] frames per clip, each in [1, T], or nullptr
    int M, T, C, d, K, n;
};

__global__ __launch_bounds__(256) void dac_latent_search_kernel(DacSearchArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= (long long)a.M * a.n) return;                      // wave-uniform
    const int i = (int)(w / a.M), row = (int)(w - (long long)i * a.M);
    const int b = row / a.T, t = row - b * a.T;
    const int d = a.d, K = a.K;
    int nb = a.n;                                               // stages of this row (wave-uniform)
    if (a.clip_n) nb = max(0, min(a.clip_n[b], a.n));
    if (a.frame_len && t >= a.frame_len[b]) nb = 0;
    long long* out = a.codes + ((size_t)b * a.n + i) * a.T + t;
    if (i >= nb) { if (lane == 0) *out = -1; return; }
    float ze[DAC_DMAX];
    _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) ze[jd] = a.latents[((size_t)b * a.C + (size_t)i * d + jd) * a.T + t];
    float nn = 0.f;
    _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) nn += ze[jd] * ze[jd];
    const float den = fmaxf(sqrtf(nn), 1e-12f);
    float e[DAC_DMAX], e2 = 0.f;
    _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) { e[jd] = ze[jd] / den; e2 += e[jd] * e[jd]; }
    float bd = INFINITY; int best = 0x7fffffff;
    const float* cbn = a.cbn + (size_t)i * K * d;
    const float* c2 = a.c2 + (size_t)i * K;
    for (int k = lane; k < K; k += 64) {
        float dot = 0.f;
        _Pragma("unroll") for (int jd = 0; jd < DAC_DMAX; ++jd) if (jd < d) dot = fmaf(e[jd], cbn[(size_t)k * d + jd], dot);
        const float dist = (e2 - 2.f * dot) + c2[k];
        if (dist < bd) { bd = dist; best = k; }                              // k rises per lane: the first minimum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o, 64); const int ok = __shfl_xor(best, o, 64);
        if (od < bd || (od == bd && ok < best)) { bd = od; best = ok; }
    }
    if (best == 0x7fffffff) best = 0;                                       // every distance NaN
    if (lane == 0) *out = best;
}

}  // namespace escx
