// Kernels of the DAC training losses (dac_loss.hip): what the DAC form of the spectral losses needs and ESC's mel loss (train_kernels.h) lacks, and the two
// waveform losses.  Reference: baselines/descript/dac/nn/loss.py:11-327.  No atomics; every partial sum has one owner and is added in a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm_engine.h"

namespace escx {

// ------------------------------------------------------------------------------------------------
// STFT framing of TWO signals in one GEMM: rows [0, B T) are the frames of `est`, rows [B T, 2 B T) those of `ref` (they share the windowed-DFT matrix).
// A[(c, f)][k] = wave_c[reflect(f * hop + k + off)].  The reflected index is clamped as well: the K tail past the window (zero weights) may reach
// further than one reflection covers on the shortest clips.
// ------------------------------------------------------------------------------------------------
struct FramePairA {
    const float* est; const float* ref; int B, L, T, hop, off, M; FastDiv dT;
    struct Ctx { const float* w; int start; };
    __device__ __forceinline__ Ctx make_ctx(int m) const {
        Ctx c; c.w = nullptr; c.start = 0;
        if (m < M) {
            const int clip = dT.div(m), f = m - clip * T;
            c.w = clip < B ? est + (size_t)clip * L : ref + (size_t)(clip - B) * L;
            c.start = f * hop + off;
        }
        return c;
    }
    __device__ __forceinline__ float at(const float* w, int p) const {
        if (p < 0) p = -p;
        if (p >= L) p = 2 * (L - 1) - p;
        p = p < 0 ? 0 : (p >= L ? L - 1 : p);
        return w[p];
    }
    __device__ __forceinline__ f32x4 load4(const Ctx& c, int k0, int kin) const {
        if (!c.w) return zero4();
        const int p = c.start + k0 + kin;
        f32x4 v; v[0] = at(c.w, p); v[1] = at(c.w, p + 1); v[2] = at(c.w, p + 2); v[3] = at(c.w, p + 3);
        return v;
    }
};

// ------------------------------------------------------------------------------------------------
// The same spectra with fp64 accumulation (the scales without a filterbank): spec[(c, t)][n] = fp32( sum_k wave_c[reflect(t hop + off + k)] W[k][n] ), W the
// windowed-DFT matrix in fp64 ([win][Np], pad columns zero).  The log term's 1 / |S| amplifies the rounding of a near-empty bin, and an fp32 chain of 2048
// products is further from the exact spectrum than an FFT is.  Form of stft_f64_kernel (train_kernels.h) for any window: the samples of DL_FR frames are staged
// in LDS one K chunk at a time and a thread owns DL_NC spectrum columns (256 apart: coalesced matrix rows), so one broadcast LDS read of a sample feeds DL_NC
// FMAs, and a matrix element read from memory feeds DL_FR of them: the kernel is bound by re-reading the fp64 matrix (34 MB at window 2048, once per
// workgroup), so the frames per workgroup decide its time.  16 frames x 4 columns where the grid still fills the chip, 8 x 1 otherwise; an output is one
// k-ordered chain either way, so its bits do not depend on the choice (nor on the batch).
// ------------------------------------------------------------------------------------------------
constexpr int DL_LDS_DOUBLES = 2048;      // samples staged per K chunk: DL_FR frames x (2048 / DL_FR) samples, 16 KB
template <int DL_FR, int DL_NC>
static __global__ __launch_bounds__(256) void dl_stft_f64_kernel(const float* __restrict__ est, const float* __restrict__ ref, const double* __restrict__ W,
                                                                 float* __restrict__ spec, int B, int L, int T, int hop, int off, int win, int Np) {
    constexpr int DL_KC = DL_LDS_DOUBLES / DL_FR;
    __shared__ double xs[DL_KC][DL_FR];
    const long long M = 2ll * B * T, m0 = (long long)blockIdx.x * DL_FR;
    const int n0 = blockIdx.y * 256 * DL_NC + threadIdx.x;
    int col[DL_NC];                       // clamped: a column past Np reads the last one and is not stored
#pragma unroll
    for (int c = 0; c < DL_NC; ++c) col[c] = min(n0 + c * 256, Np - 1);
    double acc[DL_NC][DL_FR];
#pragma unroll
    for (int c = 0; c < DL_NC; ++c)
#pragma unroll
        for (int j = 0; j < DL_FR; ++j) acc[c][j] = 0.0;
    for (int k0 = 0; k0 < win; k0 += DL_KC) {
        for (int e = threadIdx.x; e < DL_FR * DL_KC; e += 256) {
            const int j = e / DL_KC, k = e - j * DL_KC;
            const long long m = m0 + j;
            double v = 0.0;
            if (m < M && k0 + k < win) {
                const int clip = (int)(m / T), t = (int)(m - (long long)clip * T);
                const float* w = clip < B ? est + (size_t)clip * L : ref + (size_t)(clip - B) * L;
                int p = t * hop + off + k0 + k;
                if (p < 0) p = -p;
                if (p >= L) p = 2 * (L - 1) - p;
                p = p < 0 ? 0 : (p >= L ? L - 1 : p);
                v = (double)w[p];
            }
            xs[k][j] = v;
        }
        __syncthreads();
        if (n0 < Np) {
            const int kn = min(DL_KC, win - k0);
#pragma unroll 2
            for (int k = 0; k < kn; ++k) {
                double w[DL_NC];
#pragma unroll
                for (int c = 0; c < DL_NC; ++c) w[c] = W[(size_t)(k0 + k) * Np + col[c]];
#pragma unroll
                for (int j = 0; j < DL_FR; ++j) {
                    const double x = xs[k][j];
#pragma unroll
                    for (int c = 0; c < DL_NC; ++c) acc[c][j] += x * w[c];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int c = 0; c < DL_NC; ++c) {
        const int n = n0 + c * 256;
        if (n < Np) {
#pragma unroll
            for (int j = 0; j < DL_FR; ++j) if (m0 + j < M) spec[(size_t)(m0 + j) * Np + n] = (float)acc[c][j];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The generalised term (loss.py:223-227, 322-326) of one cell: wl |log10(clamp(x)^p) - log10(clamp(y)^p)| + wm |x - y| and its derivatives.
// A zero weight skips its term (and the transcendental work).  The log of the power is evaluated as the reference does, log10(pow(v, p)); p = 1 and p = 2 are
// the identity and v * v, as torch.pow gives them.  Autograd conventions: sign(0) = 0, clamp(min) passes the gradient where v >= clamp_eps.
// ------------------------------------------------------------------------------------------------
struct DlTerm { float clamp_eps, pw, wl, wm, dlog, inv_n; int pmode; };      // dlog = p / ln 10; pmode 1: p == 1, 2: p == 2, 0: powf
__device__ __forceinline__ float dl_sign(float a) { return a > 0.f ? 1.f : (a < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float dl_logpow(const DlTerm& t, float v) { return log10f(t.pmode == 1 ? v : (t.pmode == 2 ? v * v : powf(v, t.pw))); }
__device__ __forceinline__ float dl_cell(const DlTerm& t, float x, float y, float& gx, float& gy) {
    float acc = 0.f, gxv = 0.f, gyv = 0.f;
    if (t.wm != 0.f) {
        const float d = x - y;
        acc = t.wm * fabsf(d);
        gxv = t.wm * dl_sign(d); gyv = -gxv;
    }
    if (t.wl != 0.f) {
        const float xc = fmaxf(x, t.clamp_eps), yc = fmaxf(y, t.clamp_eps);
        const float d = dl_logpow(t, xc) - dl_logpow(t, yc);
        acc += t.wl * fabsf(d);
        const float s = dl_sign(d) * t.wl * t.dlog;
        if (x >= t.clamp_eps) gxv += s / xc;
        if (y >= t.clamp_eps) gyv -= s / yc;
    }
    gx = gxv * t.inv_n; gy = gyv * t.inv_n;
    return acc;
}
__device__ __forceinline__ void dl_block_sum(float acc, float* __restrict__ part, float scale) {
    __shared__ float red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] * scale;
}

// Filterbank scales: xm / ym are the [rows][ldm] mel maps of the estimate and the reference (all clips), gx / gy (optional) receive d loss / d mel.
static __global__ __launch_bounds__(256) void dl_mel_term_kernel(const float* __restrict__ xm, const float* __restrict__ ym, float* __restrict__ part,
                                                                 float* __restrict__ gx, float* __restrict__ gy, long long rows, int n_mels, int ldm, DlTerm t) {
    const long long total = rows * ldm;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % ldm);
        float a = 0.f, b = 0.f;
        if (c < n_mels) acc += dl_cell(t, xm[i], ym[i], a, b);
        if (gx) gx[i] = a;
        if (gy) gy[i] = b;
    }
    dl_block_sum(acc, part, t.inv_n);
}

// Scales without a filterbank (the STFT loss), ONE pass over the two spectra ([rows][2 Fq], re | im): |S| of both sides, the two terms and d spec of each side
// that wants one (|S| has zero gradient at S = 0).  No magnitude buffers, no separate magnitude backward.  Pad columns of d spec are written as zeros.
static __global__ __launch_bounds__(256) void dl_stft_term_kernel(const float* __restrict__ sx, const float* __restrict__ sy, float* __restrict__ part,
                                                                  float* __restrict__ dsx, float* __restrict__ dsy, long long rows, int F, int Fq, DlTerm t) {
    const long long total = rows * Fq;
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / Fq; const int f = (int)(i - r * Fq);
        const size_t o = (size_t)r * 2 * Fq + f;
        float gxr = 0.f, gxi = 0.f, gyr = 0.f, gyi = 0.f;
        if (f < F) {
            const float xr = sx[o], xi = sx[o + Fq], yr = sy[o], yi = sy[o + Fq];
            const float mx = sqrtf(xr * xr + xi * xi), my = sqrtf(yr * yr + yi * yi);
            float a, b;
            acc += dl_cell(t, mx, my, a, b);
            if (mx > 0.f) { const float g = a / mx; gxr = g * xr; gxi = g * xi; }
            if (my > 0.f) { const float g = b / my; gyr = g * yr; gyi = g * yi; }
        }
        if (dsx) { dsx[o] = gxr; dsx[o + Fq] = gxi; }
        if (dsy) { dsy[o] = gyr; dsy[o + Fq] = gyi; }
    }
    dl_block_sum(acc, part, t.inv_n);
}

// loss[0] = sum over scales and blocks of part[s][j], j-major tree then fixed order: one workgroup of 256 threads, part is [n_scales][256]
static __global__ __launch_bounds__(256) void dl_finish_kernel(const float* __restrict__ part, int n_scales, float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int k = 0; k < n_scales; ++k) s += (double)part[k * 256 + threadIdx.x];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h]; __syncthreads(); }
    if (threadIdx.x == 0) loss[0] = (float)red[0];
}

// ------------------------------------------------------------------------------------------------
// L1 on the waveform (loss.py:11-48): value, sign gradients and the partial sums in one kernel.  part[block] = sum |x - y| of the block's elements;
// gradients = +-scale * sign(x - y), sign(0) = 0.
// ------------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void dl_wave_l1_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ part,
                                                                float* __restrict__ gx, float* __restrict__ gy, long long n, float scale) {
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float d = x[i] - y[i];
        acc += fabsf(d);
        const float s = dl_sign(d) * scale;
        if (gx) gx[i] = s;
        if (gy) gy[i] = -s;
    }
    dl_block_sum(acc, part, 1.0f);
}
static __global__ __launch_bounds__(256) void dl_sum_scale_kernel(const float* __restrict__ part, int n, float scale, float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += (double)part[k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = (float)(red[0] * (double)scale);
}

// ------------------------------------------------------------------------------------------------
// SI-SDR (loss.py:51-139), per clip, in fp64 on the fp32 samples: stage 1 the two sums (means), stage 2 the three inner products of the centred
// signals, stage 3 the value and both gradients.  Partial sums are [B][bpc][k] doubles, added in block order by every consumer.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dl_block_sum64(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    const double r = red[0];
    __syncthreads();
    return r;
}
static __global__ __launch_bounds__(256) void dl_sisdr_sums_kernel(const float* __restrict__ ref, const float* __restrict__ est, double* __restrict__ p1, long long L,
                                                                   int bpc) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    double sr = 0.0, se = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < L; i += (long long)bpc * 256) { sr += (double)ref[(size_t)b * L + i]; se += (double)est[(size_t)b * L + i]; }
    sr = dl_block_sum64(sr, red); se = dl_block_sum64(se, red);
    if (threadIdx.x == 0) { p1[((size_t)b * bpc + blockIdx.x) * 2] = sr; p1[((size_t)b * bpc + blockIdx.x) * 2 + 1] = se; }
}
__device__ __forceinline__ void dl_sisdr_means(const double* __restrict__ p1, int b, int bpc, long long L, int zero_mean, double& mr, double& me) {
    double sr = 0.0, se = 0.0;
    if (zero_mean) for (int k = 0; k < bpc; ++k) { sr += p1[((size_t)b * bpc + k) * 2]; se += p1[((size_t)b * bpc + k) * 2 + 1]; }
    mr = sr / (double)L; me = se / (double)L;
}
static __global__ __launch_bounds__(256) void dl_sisdr_dots_kernel(const float* __restrict__ ref, const float* __restrict__ est, const double* __restrict__ p1,
                                                                   double* __restrict__ p2, long long L, int bpc, int zero_mean) {
    __shared__ double red[256];
    const int b = blockIdx.y;
    double mr, me;
    dl_sisdr_means(p1, b, bpc, L, zero_mean, mr, me);
    double srr = 0.0, ser = 0.0, see = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < L; i += (long long)bpc * 256) {
        const double r = (double)ref[(size_t)b * L + i] - mr, e = (double)est[(size_t)b * L + i] - me;
        srr += r * r; ser += e * r; see += e * e;
    }
    srr = dl_block_sum64(srr, red); ser = dl_block_sum64(ser, red); see = dl_block_sum64(see, red);
    if (threadIdx.x == 0) { double* o = p2 + ((size_t)b * bpc + blockIdx.x) * 3; o[0] = srr; o[1] = ser; o[2] = see; }
}
// value (block 0 of a clip) and gradients: with S = sum r^2, C = sum e r, E = sum e^2, P = S + eps, alpha = (C + eps) / P (1 without scaling),
// signal = alpha^2 S, noise N = E - 2 alpha C + alpha^2 S, q = signal / N + eps, sdr = -10 log10 q.  d sdr / d e_i = Ae e_i + Be r_i and d sdr / d r_i = Ar e_i + Br r_i
// on the centred signals; the centring itself adds nothing (the centred signals sum to zero).  clip_min cuts the gradient below it.
static __global__ __launch_bounds__(256) void dl_sisdr_grad_kernel(const float* __restrict__ ref, const float* __restrict__ est, const double* __restrict__ p1,
                                                                   const double* __restrict__ p2, float* __restrict__ loss, float* __restrict__ d_ref,
                                                                   float* __restrict__ d_est, long long L, int bpc, int zero_mean, int scaling, int has_clip,
                                                                   float clip_min) {
    const int b = blockIdx.y;
    const double eps = 1e-8;
    double mr, me;
    dl_sisdr_means(p1, b, bpc, L, zero_mean, mr, me);
    double S = 0.0, C = 0.0, E = 0.0;
    for (int k = 0; k < bpc; ++k) { const double* o = p2 + ((size_t)b * bpc + k) * 3; S += o[0]; C += o[1]; E += o[2]; }
    const double P = S + eps;
    const double alpha = scaling ? (C + eps) / P : 1.0;
    const double signal = alpha * alpha * S;
    const double N = E - 2.0 * alpha * C + alpha * alpha * S;
    const double q = signal / N + eps;
    double sdr = -10.0 * log10(q);
    double dq = -10.0 / (2.302585092994045684 * q);       // d sdr / d q
    if (has_clip && sdr < (double)clip_min) { sdr = (double)clip_min; dq = 0.0; }
    if (blockIdx.x == 0 && threadIdx.x == 0) loss[b] = (float)sdr;
    if (!d_ref && !d_est) return;
    // dq = ds / N - signal dN / N^2; residual res = e - alpha r, K = sum res r = C - alpha S
    const double K = C - alpha * S, cs = dq / N, cn = -dq * signal / (N * N);
    double Ae, Be, Ar, Br;
    if (scaling) {
        // d alpha / d e_i = r_i / P, d alpha / d r_i = e_i / P - 2 alpha r_i / P; d signal = 2 alpha S d alpha + 2 alpha^2 r_i dr_i; d N = 2 res de - 2 alpha res dr - 2 K d alpha
        const double ua = cs * 2.0 * alpha * S - cn * 2.0 * K;         // coefficient of d alpha
        Ae = cn * 2.0;                                                  // res_i = e_i - alpha r_i
        Be = -cn * 2.0 * alpha + ua / P;
        Ar = -cn * 2.0 * alpha + ua / P;
        Br = cn * 2.0 * alpha * alpha + cs * 2.0 * alpha * alpha - ua * 2.0 * alpha / P;
    } else {
        Ae = cn * 2.0; Be = -cn * 2.0;
        Ar = -cn * 2.0; Br = cn * 2.0 + cs * 2.0;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < L; i += (long long)bpc * 256) {
        const double r = (double)ref[(size_t)b * L + i] - mr, e = (double)est[(size_t)b * L + i] - me;
        if (d_est) d_est[(size_t)b * L + i] = (float)(Ae * e + Be * r);
        if (d_ref) d_ref[(size_t)b * L + i] = (float)(Ar * e + Br * r);
    }
}

}  // namespace escx
