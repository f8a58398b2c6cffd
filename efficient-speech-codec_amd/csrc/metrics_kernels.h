// Kernels of the evaluation metrics (metrics.hip): the reference's scripts/metrics.py:12-171 with a per-clip sample count, so that a zero-padded
// batch of clips of different lengths gets, clip by clip, the numbers of the call on the clip alone.
//   FramePairLenA        STFT framing of BOTH signals in one GEMM (rows [0, B T): raw, [B T, 2 B T): reconstruction) with the clip's own reflect point
//   MagRowsLenA          A-side loader of the mel projection: |S| of a spectrum row, formed while the row is staged (no magnitude buffer, no launch)
//   met_mel_log_kernel   sum over the clip's own frames of |log10(clamp(x)^2) - log10(clamp(y)^2)|, fp64 partial sums with one owner each
//   met_mel_finish_kernel  the seven resolutions' means, added in resolution order
//   met_sisdr_kernel     SI-SDR of one clip per workgroup, three fp64 passes over the clip's own samples
//   met_hist_kernel      code histogram of one (stream, group) slot per workgroup, integer counts in LDS
// No floating-point atomics; every sum has one owner and one order, which depends on (batch, n_samples) alone.  Nothing at or past a clip's own length is
// read: rows past its frame count are dead (their tiles return before the first load), and the reflected index is clamped to the clip.
#pragma once
#include <hip/hip_runtime.h>

#include "dac_loss_kernels.h"
#include "gemm_engine.h"

namespace escx {

struct FramePairLenA {          // len_kernels.h FrameALen over two signals: A[(c, f)][k] = wave_c[reflect_b(f * hop + k + off)], b = c mod B, rows f >= 1 + len[b] / hop dead
    static constexpr bool SKIPS_DEAD_TILES = true;
    const float* raw; const float* rec; const int* len; int B, L, T, hop, off, M; FastDiv dT;      // L: row stride of both signals, T: frames per clip of the padded spectrum
    struct Ctx { const float* w; int start; int n; };
    __device__ __forceinline__ Ctx make_ctx(int m) const {
        Ctx c; c.w = nullptr; c.start = 0; c.n = 0;
        if (m < M) {
            const int clip = dT.div(m), f = m - clip * T, b = clip < B ? clip : clip - B, n = len[b];
            if (f < 1 + n / hop) { c.w = (clip < B ? raw : rec) + (size_t)b * L; c.start = f * hop + off; c.n = n; }
        }
        return c;
    }
    __device__ __forceinline__ int row_live(const Ctx& c) const { return c.w != nullptr; }
    __device__ __forceinline__ float at(const Ctx& c, int p) const {
        if (p < 0) p = -p;
        if (p >= c.n) p = 2 * (c.n - 1) - p;
        p = p < 0 ? 0 : (p >= c.n ? c.n - 1 : p);          // never taken for len > window / 2 and K = window; keeps every read inside the clip
        return c.w[p];
    }
    __device__ __forceinline__ f32x4 load4(const Ctx& c, int k0, int kin) const {
        if (!c.w) return zero4();
        const int p = c.start + k0 + kin;
        f32x4 v; v[0] = at(c, p); v[1] = at(c, p + 1); v[2] = at(c, p + 2); v[3] = at(c, p + 3);
        return v;
    }
};

struct MagRowsLenA {            // A[m][k] = |spec[m][k] + i spec[m][Fq + k]| of the live rows of a [2 B T][2 Fq] spectrum (pad bins are exact zeros: zero DFT rows)
    static constexpr bool SKIPS_DEAD_TILES = true;
    const float* spec; const int* len; int B, T, hop, Fq, M; FastDiv dT;
    struct Ctx { const float* p; };
    __device__ __forceinline__ Ctx make_ctx(int m) const {
        Ctx c; c.p = nullptr;
        if (m < M) {
            const int clip = dT.div(m), f = m - clip * T, b = clip < B ? clip : clip - B;
            if (f < 1 + len[b] / hop) c.p = spec + (size_t)m * 2 * Fq;
        }
        return c;
    }
    __device__ __forceinline__ int row_live(const Ctx& c) const { return c.p != nullptr; }
    __device__ __forceinline__ f32x4 load4(const Ctx& c, int k0, int kin) const {
        if (!c.p) return zero4();
        const f32x4 re = ld4(c.p + k0 + kin), im = ld4(c.p + Fq + k0 + kin);
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = sqrtf(re[r] * re[r] + im[r] * im[r]);
        return v;
    }
};

// mel: [2 B T][Mp] (raw clips, then reconstructions).  part[b * bpc + k] = sum over the cells (f < 1 + len[b] / hop, c < n_mels) that block k of clip b owns.
static __global__ __launch_bounds__(256) void met_mel_log_kernel(const float* __restrict__ mel, const int* __restrict__ len, double* __restrict__ part, int B,
                                                                 int T, int hop, int n_mels, int Mp, int bpc, float clamp_eps) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    const long long per = (long long)(1 + len[b] / hop) * n_mels;
    const float* x = mel + (size_t)b * T * Mp;
    const float* y = mel + (size_t)(B + b) * T * Mp;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long long)bpc * 256) {
        const long long f = i / n_mels; const int c = (int)(i - f * n_mels);
        const float xc = fmaxf(x[f * Mp + c], clamp_eps), yc = fmaxf(y[f * Mp + c], clamp_eps);
        acc += fabs(log10((double)xc * (double)xc) - log10((double)yc * (double)yc));
    }
    acc = dl_block_sum64(acc, red);
    if (threadIdx.x == 0) part[(size_t)b * bpc + blockIdx.x] = acc;
}

struct MetMelScales { int hop[7]; int n_mels[7]; };
// out[b] = sum_i (sum_k part[i][b][k]) / (n_mels_i * (1 + len[b] / hop_i)), resolutions and blocks in index order
static __global__ void met_mel_finish_kernel(const double* __restrict__ part, const int* __restrict__ len, MetMelScales sc, int B, int bpc, float* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double total = 0.0;
    for (int i = 0; i < 7; ++i) {
        double s = 0.0;
        for (int k = 0; k < bpc; ++k) s += part[((size_t)i * B + b) * bpc + k];
        total += s / ((double)sc.n_mels[i] * (double)(1 + len[b] / sc.hop[i]));
    }
    out[b] = (float)total;
}

// SISDR.forward (metrics.py:123-171) on ref[b][:n], est[b][:n], n = len[b] (L when len is null): eps = 1e-8 on the projection, the cross term and inside the log10.
static __global__ __launch_bounds__(256) void met_sisdr_kernel(const float* __restrict__ ref, const float* __restrict__ est, const int* __restrict__ len, long long L,
                                                               int scaling, int zero_mean, float* __restrict__ out) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    const long long n = len ? (long long)len[b] : L;
    const float* r = ref + (size_t)b * L;
    const float* e = est + (size_t)b * L;
    const double eps = 1e-8;
    double mr = 0.0, me = 0.0;
    if (zero_mean) {
        double sr = 0.0, se = 0.0;
        for (long long i = threadIdx.x; i < n; i += 256) { sr += (double)r[i]; se += (double)e[i]; }
        mr = dl_block_sum64(sr, red) / (double)n; me = dl_block_sum64(se, red) / (double)n;
    }
    double srr = 0.0, ser = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) { const double rv = (double)r[i] - mr, ev = (double)e[i] - me; srr += rv * rv; ser += ev * rv; }
    srr = dl_block_sum64(srr, red); ser = dl_block_sum64(ser, red);
    const double alpha = scaling ? (ser + eps) / (srr + eps) : 1.0;
    double sig = 0.0, res = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
        const double t = alpha * ((double)r[i] - mr), d = ((double)e[i] - me) - t;
        sig += t * t; res += d * d;
    }
    sig = dl_block_sum64(sig, red); res = dl_block_sum64(res, red);
    if (threadIdx.x == 0) out[b] = (float)(10.0 * log10(sig / res + eps));
}

// EntropyCounter.update (metrics.py:37-51): codes (B, SG, T) int64, one workgroup per slot sg; counts[sg * K + k] += #{codes == k}.  K is walked in chunks of
// MET_HIST_BINS LDS counters (one chunk for the codecs' 1024 entries).  Negative codes are skipped, codes >= K add to overflow[0] and nothing else.
constexpr int MET_HIST_BINS = 8192;
static __global__ __launch_bounds__(256) void met_hist_kernel(const long long* __restrict__ codes, int B, int SG, int T, int K, long long* __restrict__ counts,
                                                              unsigned long long* __restrict__ overflow) {
    __shared__ int hist[MET_HIST_BINS];
    __shared__ int over;
    const int sg = blockIdx.x;
    const long long n = (long long)B * T;
    if (threadIdx.x == 0) over = 0;
    for (int k0 = 0; k0 < K; k0 += MET_HIST_BINS) {
        const int nb = min(MET_HIST_BINS, K - k0);
        for (int k = threadIdx.x; k < nb; k += 256) hist[k] = 0;
        __syncthreads();
        for (long long i = threadIdx.x; i < n; i += 256) {
            const long long b = i / T, t = i - b * T;
            const long long c = codes[((size_t)b * SG + sg) * T + t];
            if (c >= k0 && c < k0 + nb) atomicAdd(&hist[(int)(c - k0)], 1);
            else if (k0 == 0 && c >= K) atomicAdd(&over, 1);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < nb; k += 256)
            if (hist[k]) counts[(size_t)sg * K + k0 + k] += hist[k];
        __syncthreads();
    }
    if (threadIdx.x == 0 && over) atomicAdd(overflow, (unsigned long long)over);
}

}  // namespace escx
