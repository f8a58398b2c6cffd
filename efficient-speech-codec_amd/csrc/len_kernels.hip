// Launchers of the length-aware kernels of ESC's mixed-length batches (len_kernels.h).
#include "len_kernels.h"
#include "launchers.h"

namespace escx {

void gemm_frames_len(const float* wave, const int* len, int B, int L, int T, int hop, int off, const float* W, int Np, int Kp, float* out, hipStream_t s) {
    FrameALen ld{wave, len, L, T, hop, off, B * T, FastDiv(T)};
    launch_gemm<64>(ld, W, B * T, Np, Kp, EpiStore{out, Np, nullptr}, s);
}

int window_attention_len(const float* qkv, const float* bias, float* out, int total_windows, int nH, int hdp, int ldq, int ldo, const int* flags, int shifted,
                         hipStream_t s) {
    const long long pairs = (long long)total_windows * nH;
    long long g = (pairs + 3) / 4;
    const int grid = (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
#define ESCX_ATT(S) case S: ESCX_LAUNCH((window_attention_len_kernel<S>), dim3(grid), dim3(256), 0, s, qkv, bias, out, (int)pairs, nH, ldq, ldo, flags, shifted); return 0;
    switch (hdp / 4) {
        ESCX_ATT(1) ESCX_ATT(2) ESCX_ATT(3) ESCX_ATT(4) ESCX_ATT(5) ESCX_ATT(6) ESCX_ATT(7) ESCX_ATT(8)
        ESCX_ATT(12) ESCX_ATT(16)
        default: return -1;
    }
#undef ESCX_ATT
}

void zero_dead_cols(float* x, const int* wlen, int B, int H, int W, int Cp, hipStream_t s) {
    const long long n = (long long)B * H * W * (Cp / 4);
    ESCX_LAUNCH(zero_dead_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, wlen, B, H, W, Cp);
}

int deembed_border_len(const float* x, const float* wv, const float* bv, float* out, const int* wlen, int B, int H, int W, int C, int Cp, int pf, int pt,
                       int in_dim, int Fp, hipStream_t s) {
    const int per_clip = 2 * W + 2 * (H > 2 ? H - 2 : 0);
    const long long waves = (long long)B * per_clip;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    const int NO = in_dim * pf * pt;
    if (NO == 12) ESCX_LAUNCH((deembed_border_len_kernel<12>), dim3(grid), dim3(256), 0, s, x, wv, bv, out, wlen, B, H, W, C, Cp, pf, pt, in_dim, Fp);
    else if (NO == 8) ESCX_LAUNCH((deembed_border_len_kernel<8>), dim3(grid), dim3(256), 0, s, x, wv, bv, out, wlen, B, H, W, C, Cp, pf, pt, in_dim, Fp);
    else if (NO == 6) ESCX_LAUNCH((deembed_border_len_kernel<6>), dim3(grid), dim3(256), 0, s, x, wv, bv, out, wlen, B, H, W, C, Cp, pf, pt, in_dim, Fp);
    else if (NO == 4) ESCX_LAUNCH((deembed_border_len_kernel<4>), dim3(grid), dim3(256), 0, s, x, wv, bv, out, wlen, B, H, W, C, Cp, pf, pt, in_dim, Fp);
    else return -1;
    return 0;
}

void istft_ola_len(const float* frames, const float* win2, float* wave, const int* wlen, int pt, int B, int T, int ldf, int win, int hop, int left, int half,
                   int out_len, hipStream_t s) {
    const long long n = (long long)B * out_len;
    ESCX_LAUNCH(istft_ola_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, frames, win2, wave, wlen, pt, B, T, ldf, win, hop, left, half, out_len);
}

void loss_reduce_len(const float* terms, const int* wlen, int ov, int n_slots, int G, int B, int Tq, float* out, hipStream_t s) {
    ESCX_LAUNCH(loss_reduce_len_kernel, dim3(B), dim3(64), 0, s, terms, wlen, ov, n_slots, G, B * Tq, Tq, out);
}

void codes_mask_len(const long long* src, long long* dst, const int* wlen, int ov, int B, int rows, int Tq, long long fill, hipStream_t s) {
    const long long n = (long long)B * rows * Tq;
    ESCX_LAUNCH(codes_mask_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, wlen, ov, B, rows, Tq, fill);
}

void unpad_rows_len(const float* src, float* dst, const int* len, int per_w, int pt, int hop, int B, int T, int segs, int C, int Cp, hipStream_t s) {
    const long long n = (long long)B * T * segs * C;
    ESCX_LAUNCH(unpad_rows_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, len, per_w, pt, hop, B, T, segs, C, Cp);
}

}  // namespace escx
