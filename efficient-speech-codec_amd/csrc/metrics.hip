// Evaluation metrics on MI355X (the reference's scripts/metrics.py:12-171) with per-clip lengths: mel-spectrogram distance, SI-SDR, code histogram.
// A batch of whole utterances is zero-padded to its longest clip; every clip gets the number the reference's batch-size-1 loop gives it.
//
// Mel distance, per resolution (window w, hop w / 4), on the tables of the mel loss (build_mel, train.hip):
//   1. spectra of BOTH signals in one framing GEMM over 2B clips (FramePairLenA: two base pointers, the clip's own reflect point, dead tiles skipped)
//   2. mel projection, a second GEMM whose A-side loader (MagRowsLenA) forms |S| from the spectrum row while staging it
//   3. met_mel_log_kernel: the log term over the clip's own frames, fp64 partial sums
// and one met_mel_finish_kernel after the seven resolutions.  No gradient buffers and no magnitude-L1 term (that is the training loss, escx_mel_loss_ex).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "escx_internal.h"
#include "metrics_kernels.h"

using namespace escx;

namespace {
constexpr int MET_SLOT = 5;             // stream_scratch slot of the metrics
constexpr int MET_BPC = 64;             // partial sums per (resolution, clip)
size_t met_pad64(size_t n) { return (n + 63) / 64 * 64; }

// NULL: every clip has n_samples.  Otherwise lo < len[b] <= n_samples, or the message names the clip.
int met_lengths(const int32_t* lengths_host, int B, long long L, int lo, std::vector<int32_t>* out) {
    out->assign(B, (int32_t)L);
    if (!lengths_host) return 0;
    for (int b = 0; b < B; ++b) {
        const long long n = lengths_host[b];
        if (n <= lo || n > L) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "lengths[%d]=%lld outside (%d, %lld]", b, n, lo, L);
        (*out)[b] = (int32_t)n;
    }
    return 0;
}
}  // namespace

extern "C" int escx_mel_distance(const float* raw, const float* recon, int B, int L, const int32_t* lengths_host, int sample_rate, float* out, void* stream) {
    if (!raw || !recon || !out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null signal or output pointer");
    if (B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d: at least one clip", B);
    if (sample_rate < 2) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "sample_rate=%d", sample_rate);
    if (L <= 1024) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "n_samples=%d too short for the 2048-sample mel window (reflect padding)", L);
    if (2ll * B * (1 + L / 8) >= (1ll << 31) || (long long)B * L >= (1ll << 31)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d x n_samples=%d: more frames than a launch indexes", B, L);
    std::vector<int32_t> lens;
    int rc = met_lengths(lengths_host, B, L, 1024, &lens);
    if (rc) return rc;
    int dev = 0;
    ESCX_HIP(hipGetDevice(&dev));
    MelState* msp = nullptr;
    if ((rc = build_mel(dev, sample_rate, &msp))) return rc;
    const MelState& ms = *msp;
    hipStream_t st = (hipStream_t)stream;
    size_t spec_max = 0, mel_max = 0;
    MetMelScales sc;
    for (int i = 0; i < 7; ++i) {
        const MelScale& m = ms.sc[i];
        const size_t rows2 = (size_t)2 * B * (1 + L / m.hop);
        spec_max = std::max(spec_max, rows2 * 2 * m.Fq); mel_max = std::max(mel_max, rows2 * m.Mp);
        sc.hop[i] = m.hop; sc.n_mels[i] = m.n_mels;
    }
    // scratch: [lengths | fp64 partial sums | spectra of the widest resolution | mels of the widest]
    const size_t o_part = met_pad64(B), o_spec = o_part + met_pad64((size_t)2 * 7 * B * MET_BPC), o_mel = o_spec + met_pad64(spec_max);
    float* buf = stream_scratch(st, MET_SLOT, o_mel + met_pad64(mel_max));
    if (!buf) ESCX_FAIL(ESCX_ERR_HIP, "scratch allocation of %zu floats failed", o_mel + met_pad64(mel_max));
    int* d_len = reinterpret_cast<int*>(buf);
    double* part = reinterpret_cast<double*>(buf + o_part);
    float* spec = buf + o_spec; float* mel = buf + o_mel;
    ESCX_HIP(hipMemcpyAsync(d_len, lens.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    for (int i = 0; i < 7; ++i) {
        const MelScale& m = ms.sc[i];
        const int T = 1 + L / m.hop, M = 2 * B * T;
        launch_gemm_rows(FramePairLenA{raw, recon, d_len, B, L, T, m.hop, -m.w / 2, M, FastDiv(T)}, m.D, M, 2 * m.Fq, m.w, EpiStore{spec, 2 * m.Fq, nullptr}, st);
        launch_gemm_rows(MagRowsLenA{spec, d_len, B, T, m.hop, m.Fq, M, FastDiv(T)}, m.fb, M, m.Mp, m.Fq, EpiStore{mel, m.Mp, nullptr}, st);
        hipLaunchKernelGGL(met_mel_log_kernel, dim3(MET_BPC, B), dim3(256), 0, st, mel, d_len, part + (size_t)i * B * MET_BPC, B, T, m.hop, m.n_mels, m.Mp, MET_BPC, 1e-5f);
    }
    hipLaunchKernelGGL(met_mel_finish_kernel, dim3((B + 63) / 64), dim3(64), 0, st, part, d_len, sc, B, MET_BPC, out);
    return launch_ok("mel_distance");
}

extern "C" int escx_sisdr_metric(const float* ref, const float* est, int B, int64_t L, const int32_t* lengths_host, int scaling, int zero_mean, float* out, void* stream) {
    if (!ref || !est || !out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null signal or output pointer");
    if (B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d: at least one clip", B);
    if (L < 1 || (long long)B * L >= (1ll << 40)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d x n_samples=%lld: 1 <= n_samples, fewer than 2^40 samples in all", B, (long long)L);
    hipStream_t st = (hipStream_t)stream;
    int* d_len = nullptr;
    if (lengths_host) {
        std::vector<int32_t> lens;
        int rc = met_lengths(lengths_host, B, L, 0, &lens);
        if (rc) return rc;
        float* buf = stream_scratch(st, MET_SLOT, met_pad64(B));
        if (!buf) ESCX_FAIL(ESCX_ERR_HIP, "scratch allocation failed");
        d_len = reinterpret_cast<int*>(buf);
        ESCX_HIP(hipMemcpyAsync(d_len, lens.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(met_sisdr_kernel, dim3(B), dim3(256), 0, st, ref, est, d_len, (long long)L, scaling ? 1 : 0, zero_mean ? 1 : 0, out);
    return launch_ok("sisdr_metric");
}

extern "C" int escx_code_histogram(const int64_t* codes, int B, int S, int G, int T, int K, int64_t* counts, int64_t* overflow, void* stream) {
    if (!codes || !counts || !overflow) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null codes, counts or overflow pointer");
    if (B < 1 || S < 1 || G < 1 || T < 0 || K < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "codes (%d, %d, %d, %d) with %d entries per codebook", B, S, G, T, K);
    if ((long long)B * T >= (1ll << 31) || (long long)S * G >= (1ll << 31) || (long long)S * G * K >= (1ll << 40))
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "codes (%d, %d, %d, %d) x %d entries: more than a launch indexes", B, S, G, T, K);
    if (T == 0) return ESCX_OK;
    hipLaunchKernelGGL(met_hist_kernel, dim3(S * G), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const long long*>(codes), B, S * G, T, K,
                       reinterpret_cast<long long*>(counts), reinterpret_cast<unsigned long long*>(overflow));
    return launch_ok("code_histogram");
}
