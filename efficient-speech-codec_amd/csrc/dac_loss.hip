// Training losses of the DAC baseline on MI355X: MelSpectrogramLoss / MultiScaleSTFTLoss (one handle type, escx_spec_loss), L1Loss and SISDRLoss with
// their gradients.  Reference: baselines/descript/dac/nn/loss.py:11-327, used by baselines/descript/scripts/train_customize_no_adv.py:188-197, 257-263.
//
// A spectral-loss handle owns the windowed-DFT matrices of its scales and the filterbanks the caller computed (Slaney, any fmin / fmax / n_mels: they are data
// here).  ESC's own mel loss (train.hip escx_mel_loss*, one table per device) is a different loss and is not touched.  The launch sequence of one scale:
//   spectra of BOTH signals in one launch over 2B clips (framing GEMM with the FramePairA loader, or dl_stft_f64_kernel for a scale without a filterbank)
//   filterbank scale:  |S| (2B clips) -> mel GEMM (2B clips) -> dl_mel_term_kernel -> per side with a gradient: fbT GEMM, |S| backward, DT GEMM, framing adjoint
//   no filterbank:     dl_stft_term_kernel (|S|, both terms, d spec of each side in one pass)  -> per side with a gradient: DT GEMM, framing adjoint
// and one dl_finish_kernel at the end.  Scratch is the per-stream grow-only buffer (stream_scratch), as in escx_mel_loss_ex.  No atomics; fixed summation order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "escx_internal.h"
#include "launchers.h"
#include "train_kernels.h"
#include "dac_loss_kernels.h"

using namespace escx;

namespace {

inline unsigned dl_blocks(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }
constexpr int DL_PART = 256;             // partial sums per scale (= blocks of a term kernel)
constexpr int DL_MAX_WINDOW = 4096;

struct SpecScale {
    int w = 0, Wp = 0, hop = 0, F = 0, Fq = 0, n_mels = 0, Mp = 0;
    float *D = nullptr, *DT = nullptr, *fb = nullptr, *fbT = nullptr;
    double* D64 = nullptr;               // [w][2 Fq], scales whose spectra are accumulated in fp64
};

void dl_gemm_rows(const float* A, int lda, int M, const float* W, int Np, int Kp, float* out, int ldo, hipStream_t st) {
    launch_gemm_rows(PlainA{A, lda, M}, W, M, Np, Kp, EpiStore{out, ldo, nullptr}, st);
}

struct SpecLayout { size_t spec, mag, mel, g, dmg, dsp, dfr, part, total; };
size_t pad64(size_t n) { return (n + 63) / 64 * 64; }

}  // namespace

struct escx_spec_loss_s {
    int device = 0, n = 0, max_w = 0, min_hop = 0;
    SpecScale sc[ESCX_SPEC_LOSS_MAX_SCALES];
    float* base = nullptr; double* base64 = nullptr;
    float clamp_eps = 1e-5f, pw = 2.f, mag_w = 1.f, log_w = 1.f;
};

namespace {

SpecLayout spec_layout(const escx_spec_loss_s* h, int B, int L, int sides) {
    size_t spec = 0, mag = 0, mel = 0, dfr = 0;
    for (int i = 0; i < h->n; ++i) {
        const SpecScale& m = h->sc[i];
        const size_t rows = (size_t)B * (1 + L / m.hop);
        spec = std::max(spec, rows * 2 * m.Fq); dfr = std::max(dfr, rows * m.Wp);
        if (m.n_mels) { mag = std::max(mag, rows * m.Fq); mel = std::max(mel, rows * m.Mp); }
    }
    SpecLayout o;
    size_t at = 0;
    auto take = [&](size_t n) { const size_t a = at; at += pad64(n); return a; };
    o.spec = take(2 * spec); o.mag = take(2 * mag); o.mel = take(2 * mel); o.g = take(sides * mel); o.dmg = take(sides ? mag : 0);
    o.dsp = take(sides * spec); o.dfr = take(sides ? dfr : 0); o.part = take((size_t)ESCX_SPEC_LOSS_MAX_SCALES * DL_PART);
    o.total = at;
    return o;
}

int spec_eval_args(const escx_spec_loss_s* h, int B, int L) {
    if (!h) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null spectral-loss handle");
    if (B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d: at least one clip", B);
    if (L <= h->max_w / 2) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "n_samples=%d too short for the %d-sample window (reflect padding needs more than half a window)", L, h->max_w);
    const long long rows2 = 2ll * B * (1 + L / h->min_hop);
    if (rows2 >= (1ll << 31) || (long long)B * L >= (1ll << 31)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d x n_samples=%d: more frames than a launch indexes", B, L);
    return 0;
}

}  // namespace

extern "C" int escx_spec_loss_create(const escx_spec_loss_config* cfg, int device, escx_spec_loss* out) {
    if (!cfg || !out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (cfg->n_scales < 1 || cfg->n_scales > ESCX_SPEC_LOSS_MAX_SCALES) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "n_scales=%d: 1 .. %d", cfg->n_scales, ESCX_SPEC_LOSS_MAX_SCALES);
    if (!(cfg->clamp_eps > 0.f) || !(cfg->pow > 0.f) || !std::isfinite(cfg->pow) || !std::isfinite(cfg->mag_weight) || !std::isfinite(cfg->log_weight))
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "clamp_eps and pow must be positive, the weights finite");
    for (int i = 0; i < cfg->n_scales; ++i) {
        const int w = cfg->window[i];
        if (w < 4 || w % 4) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "window[%d]=%d: a positive multiple of 4 (hop = window / 4)", i, w);
        if (w > DL_MAX_WINDOW) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "window[%d]=%d: windows up to %d", i, w, DL_MAX_WINDOW);
        if (cfg->n_mels[i] < 0 || cfg->n_mels[i] > 4096) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "n_mels[%d]=%d", i, cfg->n_mels[i]);
        if (cfg->n_mels[i] > 0 && !cfg->filterbank[i]) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "filterbank[%d] is null for n_mels=%d", i, cfg->n_mels[i]);
    }
    int ndev = 0;
    ESCX_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "device %d of %d", device, ndev);
    int prev = 0;
    ESCX_HIP(hipGetDevice(&prev));
    ESCX_HIP(hipSetDevice(device));
    // ESCX_SPEC_LOSS_F32=1 (a debugging knob, include/escx.h): the fp32-MFMA framing GEMM for the scales without a filterbank too - the A/B of DESIGN.md 15.1
    const char* e = getenv("ESCX_SPEC_LOSS_F32");
    const bool all_f32 = e && e[0] == '1';
    escx_spec_loss_s* h = new escx_spec_loss_s();
    h->device = device; h->n = cfg->n_scales;
    h->clamp_eps = cfg->clamp_eps; h->pw = cfg->pow; h->mag_w = cfg->mag_weight; h->log_w = cfg->log_weight;
    std::vector<float> host;
    std::vector<double> host64;
    auto alloc = [&](size_t n) { const size_t o = pad64(host.size()); host.resize(o + n, 0.f); return o; };
    size_t oD[ESCX_SPEC_LOSS_MAX_SCALES], oDT[ESCX_SPEC_LOSS_MAX_SCALES], ofb[ESCX_SPEC_LOSS_MAX_SCALES], ofbT[ESCX_SPEC_LOSS_MAX_SCALES], oD64[ESCX_SPEC_LOSS_MAX_SCALES];
    h->min_hop = 1 << 30;
    for (int i = 0; i < h->n; ++i) {
        SpecScale& m = h->sc[i];
        m.w = cfg->window[i]; m.Wp = rup(m.w, 16); m.hop = m.w / 4; m.F = m.w / 2 + 1; m.Fq = rup(m.F, 16); m.n_mels = cfg->n_mels[i]; m.Mp = rup(std::max(m.n_mels, 1), 16);
        h->max_w = std::max(h->max_w, m.w); h->min_hop = std::min(h->min_hop, m.hop);
        const bool f64 = m.n_mels == 0 && !all_f32;
        oD[i] = f64 ? 0 : alloc((size_t)2 * m.Fq * m.Wp);          // the forward matrix of a scale is fp32 OR fp64, never both
        oDT[i] = alloc((size_t)m.Wp * 2 * m.Fq);
        oD64[i] = host64.size();
        if (f64) host64.resize(host64.size() + (size_t)m.w * 2 * m.Fq, 0.0);
        for (int f = 0; f < m.F; ++f) for (int k = 0; k < m.w; ++k) {
            const double win = 0.5 - 0.5 * std::cos(2.0 * M_PI * k / m.w);           // hann, periodic
            const double ang = 2.0 * M_PI * (double)((long long)f * k % m.w) / m.w;
            const double re = win * std::cos(ang), im = -win * std::sin(ang);
            if (!f64) { host[oD[i] + (size_t)f * m.Wp + k] = (float)re; host[oD[i] + (size_t)(m.Fq + f) * m.Wp + k] = (float)im; }
            host[oDT[i] + (size_t)k * 2 * m.Fq + f] = (float)re; host[oDT[i] + (size_t)k * 2 * m.Fq + m.Fq + f] = (float)im;
            if (f64) { host64[oD64[i] + (size_t)k * 2 * m.Fq + f] = re; host64[oD64[i] + (size_t)k * 2 * m.Fq + m.Fq + f] = im; }
        }
        if (m.n_mels) {
            ofb[i] = alloc((size_t)m.Mp * m.Fq); ofbT[i] = alloc((size_t)m.Fq * m.Mp);
            for (int j = 0; j < m.n_mels; ++j) for (int f = 0; f < m.F; ++f) {
                const float v = cfg->filterbank[i][(size_t)j * m.F + f];
                host[ofb[i] + (size_t)j * m.Fq + f] = v; host[ofbT[i] + (size_t)f * m.Mp + j] = v;
            }
        }
    }
    hipError_t er = hipMalloc((void**)&h->base, std::max<size_t>(host.size(), 1) * sizeof(float));
    if (er == hipSuccess) er = hipMemcpy(h->base, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
    if (er == hipSuccess && !host64.empty()) {
        er = hipMalloc((void**)&h->base64, host64.size() * sizeof(double));
        if (er == hipSuccess) er = hipMemcpy(h->base64, host64.data(), host64.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    (void)hipSetDevice(prev);
    if (er != hipSuccess) {
        if (h->base) (void)hipFree(h->base);
        if (h->base64) (void)hipFree(h->base64);
        delete h;
        ESCX_FAIL(ESCX_ERR_HIP, "spectral-loss matrices: %s", hipGetErrorString(er));
    }
    for (int i = 0; i < h->n; ++i) {
        SpecScale& m = h->sc[i];
        m.DT = h->base + oDT[i];
        if (m.n_mels) { m.fb = h->base + ofb[i]; m.fbT = h->base + ofbT[i]; }
        if (m.n_mels == 0 && !all_f32) m.D64 = h->base64 + oD64[i];
        else m.D = h->base + oD[i];
    }
    *out = h;
    return 0;
}

extern "C" void escx_spec_loss_destroy(escx_spec_loss h) {
    if (!h) return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->base) (void)hipFree(h->base);
    if (h->base64) (void)hipFree(h->base64);
    (void)hipSetDevice(prev);
    delete h;
}

extern "C" int64_t escx_spec_loss_workspace_floats(escx_spec_loss h, int B, int L, int want_d_est, int want_d_ref) {
    if (spec_eval_args(h, B, L)) return -1;
    return (int64_t)spec_layout(h, B, L, (want_d_est ? 1 : 0) + (want_d_ref ? 1 : 0)).total;
}

extern "C" int escx_spec_loss_eval(escx_spec_loss h, const float* est, const float* ref, int B, int L, float* loss, float* d_est, float* d_ref, void* stream) {
    int rc = spec_eval_args(h, B, L);
    if (rc) return rc;
    if (!est || !ref || !loss) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null signal or loss pointer");
    int dev = 0;
    ESCX_HIP(hipGetDevice(&dev));
    if (dev != h->device) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "the handle lives on device %d, the current device is %d", h->device, dev);
    hipStream_t st = (hipStream_t)stream;
    const int sides = (d_est ? 1 : 0) + (d_ref ? 1 : 0);
    const SpecLayout lay = spec_layout(h, B, L, sides);
    float* buf = stream_scratch(st, 3, lay.total);
    if (!buf) ESCX_FAIL(ESCX_ERR_HIP, "scratch allocation of %zu floats failed", lay.total);
    float* part = buf + lay.part;
    for (int i = 0; i < h->n; ++i) {
        const SpecScale& m = h->sc[i];
        const int T = 1 + L / m.hop;
        const long long rows = (long long)B * T;
        const int Np = 2 * m.Fq;
        float* spx = buf + lay.spec; float* spy = spx + (size_t)rows * Np;
        // spectra of the estimate (rows [0, B T)) and the reference (rows [B T, 2 B T)): one launch
        if (m.D64) {
            if ((long long)dl_blocks(2 * rows, 16) * dl_blocks(Np, 1024) >= 512)
                hipLaunchKernelGGL((dl_stft_f64_kernel<16, 4>), dim3(dl_blocks(2 * rows, 16), dl_blocks(Np, 1024)), dim3(256), 0, st, est, ref, m.D64, spx, B, L, T, m.hop, -m.w / 2, m.w, Np);
            else
                hipLaunchKernelGGL((dl_stft_f64_kernel<8, 1>), dim3(dl_blocks(2 * rows, 8), dl_blocks(Np, 256)), dim3(256), 0, st, est, ref, m.D64, spx, B, L, T, m.hop, -m.w / 2, m.w, Np);
        } else
            launch_gemm_rows(FramePairA{est, ref, B, L, T, m.hop, -m.w / 2, (int)(2 * rows), FastDiv(T)}, m.D, (int)(2 * rows), Np, m.Wp, EpiStore{spx, Np, nullptr}, st);
        DlTerm t;
        t.clamp_eps = h->clamp_eps; t.pw = h->pw; t.wl = h->log_w; t.wm = h->mag_w; t.dlog = (float)((double)h->pw / std::log(10.0));
        t.pmode = h->pw == 1.f ? 1 : (h->pw == 2.f ? 2 : 0);
        float* dfr = buf + lay.dfr;
        if (m.n_mels) {
            float* mgx = buf + lay.mag; float* mlx = buf + lay.mel; float* mly = mlx + (size_t)rows * m.Mp;
            float* gx = d_est ? buf + lay.g : nullptr; float* gy = d_ref ? buf + lay.g + (d_est ? (size_t)rows * m.Mp : 0) : nullptr;
            float* dmg = buf + lay.dmg; float* dsp = buf + lay.dsp;
            t.inv_n = 1.0f / ((float)rows * (float)m.n_mels);
            hipLaunchKernelGGL(complex_mag_kernel, dim3(dl_blocks(2 * rows * m.Fq)), dim3(256), 0, st, spx, mgx, 2 * rows, m.F, m.Fq, m.Fq);
            dl_gemm_rows(mgx, m.Fq, (int)(2 * rows), m.fb, m.Mp, m.Fq, mlx, m.Mp, st);
            hipLaunchKernelGGL(dl_mel_term_kernel, dim3(DL_PART), dim3(256), 0, st, mlx, mly, part + i * DL_PART, gx, gy, rows, m.n_mels, m.Mp, t);
            for (int side = 0; side < 2; ++side) {
                float* g = side ? gy : gx; float* d = side ? d_ref : d_est;
                if (!d) continue;
                dl_gemm_rows(g, m.Mp, (int)rows, m.fbT, m.Fq, m.Mp, dmg, m.Fq, st);
                hipLaunchKernelGGL(complex_mag_bwd_kernel, dim3(dl_blocks(rows * m.Fq)), dim3(256), 0, st, side ? spy : spx, dmg, dsp, rows, m.F, m.Fq, m.Fq);
                dl_gemm_rows(dsp, Np, (int)rows, m.DT, m.Wp, Np, dfr, m.Wp, st);
                hipLaunchKernelGGL(frames_bwd_kernel, dim3(dl_blocks((long long)B * L)), dim3(256), 0, st, dfr, d, B, L, T, m.hop, m.w, m.Wp, i > 0, -1);
            }
        } else {
            float* dsx = d_est ? buf + lay.dsp : nullptr; float* dsy = d_ref ? buf + lay.dsp + (d_est ? (size_t)rows * Np : 0) : nullptr;
            t.inv_n = 1.0f / ((float)rows * (float)m.F);
            hipLaunchKernelGGL(dl_stft_term_kernel, dim3(DL_PART), dim3(256), 0, st, spx, spy, part + i * DL_PART, dsx, dsy, rows, m.F, m.Fq, t);
            for (int side = 0; side < 2; ++side) {
                float* ds = side ? dsy : dsx; float* d = side ? d_ref : d_est;
                if (!d) continue;
                dl_gemm_rows(ds, Np, (int)rows, m.DT, m.Wp, Np, dfr, m.Wp, st);
                hipLaunchKernelGGL(frames_bwd_kernel, dim3(dl_blocks((long long)B * L)), dim3(256), 0, st, dfr, d, B, L, T, m.hop, m.w, m.Wp, i > 0, -1);
            }
        }
    }
    hipLaunchKernelGGL(dl_finish_kernel, dim3(1), dim3(256), 0, st, part, h->n, loss);
    return launch_ok("spec_loss_eval");
}

// L1Loss (loss.py:11-48) over n values: loss[0] = scale * sum |est - ref| (scale = 1 / n: the mean), d_est = scale * sign(est - ref), d_ref = -d_est (both optional).
extern "C" int escx_wave_l1(const float* est, const float* ref, int64_t n, float scale, float* loss, float* d_est, float* d_ref, void* stream) {
    if (!est || !ref || !loss || n < 1 || !std::isfinite(scale)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = (int)std::min<long long>(1024, ((long long)n + 255) / 256);
    float* part = stream_scratch(st, 4, 1024);
    if (!part) ESCX_FAIL(ESCX_ERR_HIP, "scratch allocation failed");
    hipLaunchKernelGGL(dl_wave_l1_kernel, dim3(blocks), dim3(256), 0, st, est, ref, part, d_est, d_ref, (long long)n, scale);
    hipLaunchKernelGGL(dl_sum_scale_kernel, dim3(1), dim3(256), 0, st, part, blocks, scale, loss);
    return launch_ok("wave_l1");
}

// SISDRLoss (loss.py:51-139) per clip: loss (B,) and the unit gradients d loss_b / d references, d loss_b / d estimates (both optional).  The reduction over the
// batch is the caller's.  has_clip_min = 0: no clip_min.
extern "C" int escx_sisdr(const float* references, const float* estimates, int B, int64_t L, int scaling, int zero_mean, int has_clip_min, float clip_min,
                          float* loss, float* d_references, float* d_estimates, void* stream) {
    if (!references || !estimates || !loss || B < 1 || L < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (B > 65535 || (long long)B * L >= (1ll << 40)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d x n_samples=%lld too large", B, (long long)L);
    hipStream_t st = (hipStream_t)stream;
    const int bpc = (int)std::min<long long>(64, ((long long)L + 255) / 256);
    double* p1 = reinterpret_cast<double*>(stream_scratch(st, 4, (size_t)2 * 5 * B * bpc));
    if (!p1) ESCX_FAIL(ESCX_ERR_HIP, "scratch allocation failed");
    double* p2 = p1 + (size_t)2 * B * bpc;
    if (zero_mean) hipLaunchKernelGGL(dl_sisdr_sums_kernel, dim3(bpc, B), dim3(256), 0, st, references, estimates, p1, (long long)L, bpc);
    hipLaunchKernelGGL(dl_sisdr_dots_kernel, dim3(bpc, B), dim3(256), 0, st, references, estimates, p1, p2, (long long)L, bpc, zero_mean ? 1 : 0);
    const bool grads = d_references || d_estimates;
    hipLaunchKernelGGL(dl_sisdr_grad_kernel, dim3(grads ? bpc : 1, B), dim3(256), 0, st, references, estimates, p1, p2, loss, d_references, d_estimates, (long long)L, bpc,
                       zero_mean ? 1 : 0, scaling ? 1 : 0, has_clip_min ? 1 : 0, clip_min);
    return launch_ok("sisdr");
}
