// Mixed-length batches of ESC (escx_encode_lengths / escx_decode_lengths / escx_forward_lengths): the length-aware forms of the kernels that are
// coupled along time.  The batch keeps the padded batch-major layout [B][H * Wmax][Cp]; clip b owns the first W_b latent columns (T_b = 1 + L_b / hop
// frames, pt * W_b de-embedded frames).  Every row-wise kernel runs unchanged on the padded maps: the tokens past a clip's columns ("dead" tokens)
// hold whatever they hold and feed nothing.  What reads ACROSS time gets a per-clip table here:
//   FrameALen                    STFT framing that reflects about L_b - 1 and skips the frames past T_b
//   zero_dead_cols_kernel        the composed de-embedding zero-pads at W_b: the dead columns of its input are stored as zeros
//   deembed_border_len_kernel    the border variants of the composed 7x7 at the clip's own last column
//   istft_ola_len_kernel         overlap-add over the clip's own frames, its own envelope at the end, zeros past its output
//   loss_reduce_len_kernel       the VQ losses over the clip's own frames
//   codes_mask_len_kernel        -1 (encode) / 0 (decode: the dead slots of the caller's tensor are not read) past the clip's code frames
//   unpad_rows_len_kernel        spectra in the reference's layout with zero rows past the clip's frames
//   window_attention_len_kernel  the attention core of the unfused sequence with per-window flags
// The fused window attention's length form is an instantiation of attn_fused_kernel (fused_attn.h, LEN).
#pragma once
#include <hip/hip_runtime.h>
#include "gemm_engine.h"

namespace escx {

struct FrameALen {              // FrameA with a per-clip sample count: A[(b,f)][k] = wave[b][reflect_b(f*hop + k + off)], rows f >= 1 + len[b] / hop are dead
    static constexpr bool SKIPS_DEAD_TILES = true;
    const float* wave; const int* len; int L, T, hop, off, M; FastDiv dT;      // L: row stride of `wave`, T: frames per clip of the padded spectrum
    struct Ctx { const float* w; int start; int n; };
    __device__ __forceinline__ Ctx make_ctx(int m) const {
        Ctx c; c.w = nullptr; c.start = 0; c.n = 0;
        if (m < M) {
            const int b = dT.div(m), f = m - b * T, n = len[b];
            if (f < 1 + n / hop) { c.w = wave + (size_t)b * L; c.start = f * hop + off; c.n = n; }
        }
        return c;
    }
    __device__ __forceinline__ int row_live(const Ctx& c) const { return c.w != nullptr; }
    __device__ __forceinline__ float at(const Ctx& c, int p) const {
        if (p < 0) p = -p;
        if (p >= c.n) p = 2 * (c.n - 1) - p;
        return c.w[p];
    }
    __device__ __forceinline__ f32x4 load4(const Ctx& c, int k0, int kin) const {
        if (!c.w) return zero4();
        const int p = c.start + k0 + kin;
        f32x4 v; v[0] = at(c, p); v[1] = at(c, p + 1); v[2] = at(c, p + 2); v[3] = at(c, p + 3);
        return v;
    }
};

// window_attention_kernel (kernels.h; the attention core of the UNFUSED sequence, for widths without a fused attention mode) on the windows of a mixed-length
// batch: the same arithmetic, with the window's place in its clip read from the flag table of the batch-wide slot map (bit 0: last window row, bit 1:
// last window column of its clip) instead of being derived from a uniform grid.  The gather before it (ln_rows, mode 1) and the scatter after it
// (gemm_proj_scatter) take the batch-wide map as it is: one "clip" of n_windows * 16 slots whose entries are absolute token rows.
template <int STEPS>
__global__ __launch_bounds__(256) void window_attention_len_kernel(const float* __restrict__ qkv, const float* __restrict__ bias, float* __restrict__ out,
                                                                   int total_pairs, int nH, int ldq, int ldo, const int* __restrict__ flags, int shifted) {
    constexpr int HDP = 4 * STEPS;
    constexpr int DT = (HDP + 15) / 16;
    const int lane = threadIdx.x & 63;
    const int i = lane & 15, g = lane >> 4;
    const int wave_global = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * 256) >> 6;
    const int kOff = nH * HDP, vOff = 2 * nH * HDP;
    for (int pair = wave_global; pair < total_pairs; pair += nwaves) {
        const int win = pair / nH, h = pair - win * nH;
        const float* base = qkv + (size_t)win * 16 * ldq + h * HDP;
        const float* rowp = base + (size_t)i * ldq + STEPS * g;
        float kf[STEPS], qf[STEPS];
#pragma unroll
        for (int r = 0; r < STEPS; ++r) { qf[r] = rowp[r]; kf[r] = rowp[kOff + r]; }
        f32x4 s = zero4();
#pragma unroll
        for (int r = 0; r < STEPS; ++r) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[r], qf[r], s, 0, 0, 0);
        s += ld4(bias + ((size_t)h * 16 + i) * 16 + 4 * g);
        if (shifted) {                          // attention.py:56-75 regions
            const int fl = flags[win];
            const bool lastH = (fl & 1) != 0, lastW = (fl & 2) != 0;
            const int qh = i >> 2, qw = i & 3;
            const int labq = 3 * (lastH ? (qh < 2 ? 1 : 2) : 0) + (lastW ? (qw < 2 ? 1 : 2) : 0);
            const int labkh = 3 * (lastH ? (g < 2 ? 1 : 2) : 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int labk = labkh + (lastW ? (r < 2 ? 1 : 2) : 0);
                s[r] += (labk != labq) ? -100.0f : 0.0f;
            }
        }
        float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        f32x4 p;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = expf(s[r] - mx);
        float den = (p[0] + p[1]) + (p[2] + p[3]);
        den += __shfl_xor(den, 16);
        den += __shfl_xor(den, 32);
        const float inv = 1.0f / den;
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] *= inv;
        float* orow = out + ((size_t)win * 16 + i) * ldo + h * HDP;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const int d = t * 16 + i;
            f32x4 o = zero4();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float vv = (d < HDP) ? base[(size_t)(4 * g + r) * ldq + vOff + d] : 0.f;
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(vv, p[r], o, 0, 0, 0);
            }
            if (t * 16 + 4 * g < HDP) st4(orow + t * 16 + 4 * g, o);
        }
        if (h == 0 && nH * HDP < ldo) {         // keep the K padding of the projection GEMM at exact zero
            for (int c = nH * HDP + g; c < ldo; c += 4) out[((size_t)win * 16 + i) * ldo + c] = 0.f;
        }
    }
}

// x: [B][H][W][Cp]; columns w >= wlen[b] become zero rows.  One thread per float4 of a dead token.
__global__ void zero_dead_cols_kernel(float* __restrict__ x, const int* __restrict__ wlen, int B, int H, int W, int Cp) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int V = Cp / 4;
    if (idx >= (long long)B * H * W * V) return;
    const long long tok = idx / V;
    const int w = (int)(tok % W), b = (int)(tok / ((long long)H * W));
    if (w >= wlen[b]) st4(x + idx * 4, zero4());
}

// deembed_border_kernel (kernels.h) with the clip's own width: the border pixels of clip b are rows 0 and H - 1 up to column wlen[b] - 1 and the
// columns 0 and wlen[b] - 1; taps past wlen[b] fall outside.  Rows of the maps keep the padded stride W.
template <int NO>
__global__ __launch_bounds__(256) void deembed_border_len_kernel(const float* __restrict__ x, const float* __restrict__ wv, const float* __restrict__ bv,
                                                                 float* __restrict__ out, const int* __restrict__ wlen, int B, int H, int W, int C, int Cp,
                                                                 int pf, int pt, int in_dim, int Fp) {
    const int per_clip = 2 * W + 2 * (H > 2 ? H - 2 : 0);          // slots of the padded width; the ones past the clip's own border return
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= B * per_clip) return;
    const int b = wave / per_clip; int i = wave - b * per_clip;
    const int Wb = wlen[b];
    int h, w;
    if (i < W) { h = 0; w = i; }
    else if (i < 2 * W) { h = H - 1; w = i - W; }
    else { i -= 2 * W; h = 1 + (i >> 1); w = (i & 1) ? Wb - 1 : 0; }
    if (w >= Wb) return;
    if (H == 1 && i >= W && i < 2 * W) return;                       // the single row was already handled
    if (Wb == 1 && i >= 2 * W && (i & 1)) return;
    const int eh = (h == 0 ? 1 : 0) | (h == H - 1 ? 2 : 0), ew = (w == 0 ? 1 : 0) | (w == Wb - 1 ? 2 : 0);
    const int K = 49 * C;
    const float* wvar = wv + (size_t)(4 * eh + ew) * NO * K;
    float acc[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) acc[o] = 0.f;
    for (int k = lane; k < K; k += 64) {
        const int tap = k / C, ci = k - tap * C;
        const int hh = h + tap / 7 - 3, ww = w + tap % 7 - 3;
        if (hh < 0 || hh >= H || ww < 0 || ww >= Wb) continue;
        const float xv = x[((size_t)(b * H + hh) * W + ww) * Cp + ci];
#pragma unroll
        for (int o = 0; o < NO; ++o) acc[o] = fmaf(wvar[(size_t)o * K + k], xv, acc[o]);
    }
#pragma unroll
    for (int o = 0; o < NO; ++o) {
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) acc[o] += __shfl_xor(acc[o], sft);
    }
    if (lane == 0) {
        const int Q = pf * pt;
        for (int o = 0; o < NO; ++o) {
            const int co = o / Q, q = o - co * Q, s1 = q / pt, s2 = q - s1 * pt;
            out[((size_t)(b * (pt * W) + pt * w + s2) * in_dim + co) * Fp + pf * h + s1] = acc[o] + bv[(4 * eh + ew) * NO + o];
        }
    }
}

// istft_ola_kernel (kernels.h) over the clip's own pt * wlen[b] frames: frames [B*T][ldf] with T frames per clip in the padded map, wave [B][out_len]
// with out_len the padded output length; samples at or past hop * (T_b - 1) are zeros.
__global__ void istft_ola_len_kernel(const float* __restrict__ frames, const float* __restrict__ win2, float* __restrict__ wave, const int* __restrict__ wlen,
                                     int pt, int B, int T, int ldf, int win, int hop, int left, int half, int out_len) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * out_len) return;
    const int b = idx / out_len, s = idx - b * out_len;
    const int Tb = pt * wlen[b];
    if (s >= hop * (Tb - 1)) { wave[idx] = 0.f; return; }
    const int p = s + half - left;
    int t_hi = p / hop; if (t_hi > Tb - 1) t_hi = Tb - 1;
    float acc = 0.f, env = 0.f;
    for (int t = t_hi; t >= 0; --t) {
        const int j = p - t * hop;
        if (j >= win) break;
        acc += frames[((size_t)b * T + t) * ldf + j];
        env += win2[j];
    }
    wave[idx] = acc / env;
}

// loss_reduce_kernel (kernels.h) over the clip's own code frames: terms [n_slots][G][B * Tq] hold sum_j (q - z)^2 / (d G) per vector (no 1 / Tq: the
// frame count is the clip's); out[b] = (sum over slot, group and t < wlen[b] / ov) / (wlen[b] / ov), the lanes' partial sums joined by the same butterfly.
__global__ __launch_bounds__(64) void loss_reduce_len_kernel(const float* __restrict__ terms, const int* __restrict__ wlen, int ov, int n_slots, int G, int M,
                                                             int Tq, float* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int Tb = wlen[b] / ov;
    const int per = n_slots * G * Tb;
    float acc = 0.f;
    for (int i = lane; i < per; i += 64) {
        const int sg = i / Tb, t = i - sg * Tb;
        acc += terms[(size_t)sg * M + (size_t)b * Tq + t];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[b] = acc / (float)Tb;
}

// codes (B, S * G, Tq) int64: dst[b][r][t] = t < wlen[b] / ov ? src[b][r][t] : fill.  src == dst masks in place; the dead slots of src are not read.
__global__ void codes_mask_len_kernel(const long long* __restrict__ src, long long* __restrict__ dst, const int* __restrict__ wlen, int ov, int B, int rows,
                                      int Tq, long long fill) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * rows * Tq) return;
    const int t = (int)(idx % Tq), b = (int)(idx / ((long long)rows * Tq));
    const bool live = t < wlen[b] / ov;
    if (live) { if (src != dst) dst[idx] = src[idx]; }
    else dst[idx] = fill;
}

// unpad_rows_kernel (kernels.h) on [B][T] frames of `segs` rows each (in_dim rows of Fp floats per frame): the frames at or past the clip's own count
// are written as zeros.  n_b = per_w ? pt * len[b] : 1 + len[b] / hop  (len = latent widths, or sample counts).
__global__ void unpad_rows_len_kernel(const float* __restrict__ src, float* __restrict__ dst, const int* __restrict__ len, int per_w, int pt, int hop, int B,
                                      int T, int segs, int C, int Cp) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * T * segs * C) return;
    const long long r = idx / C; const int c = (int)(idx - r * C);
    const long long fr = r / segs; const int t = (int)(fr % T), b = (int)(fr / T);
    const int n = per_w ? pt * len[b] : 1 + len[b] / hop;
    dst[idx] = t < n ? src[r * Cp + c] : 0.f;
}

}  // namespace escx
