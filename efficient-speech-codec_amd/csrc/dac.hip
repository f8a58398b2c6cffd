// DAC baseline codec (Descript audio codec; reference baselines/descript/dac/model/dac.py:148-247, nn/quantize.py) on MI355X, inference only.
//
// One handle = one DAC configuration.  Parameters live in a flat fp32 device buffer owned by the caller, in the reference's named_parameters()
// order (per layer: bias, weight_g, weight_v; Snake: alpha; codebook: weight); the weight-normalised, packed GEMM operands, the Snake reciprocals
// and the quantiser tables are re-derived on the device whenever (buffer, version) or the padding mode changes.  Activations are channels-last
// (B, T, Cp) maps in a handle-owned scratch; see dac_kernels.h for the loaders and epilogues.  escx_dac_set_padding(d, 0) runs every convolution
// without padding (CodecMixin.padding, base.py:58-80) and escx_dac_encode_chunks stages the overlapping windows of the chunked compress
// (base.py:182-214) straight from the signal; DESIGN.md section 13.2.  escx_dac_decode_tape / escx_dac_decode_backward are the decoder with its maps
// kept in a caller-owned tape and the latent gradient d audio / d z on it (dac_grad_kernels.h); escx_dac_encode_tape /
// escx_dac_encode_backward are the same for the encoder and the quantiser, with the audio gradient of z, latents and the commitment loss
// (DESIGN.md section 13.4).  escx_dac_decode_backward_params is the decoder's backward with the gradients of its parameters (bias, weight_g, weight_v,
// alpha) next to d_z, for fine-tuning a decoder (dac_param_grad_kernels.h, gemm_dw_kernel of train_kernels.h);
// escx_dac_set_param_grad_precision moves its weight-gradient contractions to the split-operand gemm_dw_bf16_kernel<.., 3> of gemm_bf16.h.
// escx_dac_encode_backward_params is the encoder's and the quantiser's backward with the gradients of their parameters (the codebooks included) next
// to d_audio, for fine-tuning the whole baseline (dac_param_grad_kernels.h).
// escx_dac_encode_lengths / escx_dac_from_codes_lengths / escx_dac_decode_lengths are encode, from_codes and decode for a batch with one length per
// clip (padding on): per-clip length tables in the loader and the epilogue, every clip bitwise its own call.
// escx_dac_quantize / escx_dac_quantize_backward / escx_dac_quantize_backward_params are the quantiser on a latent the caller brings (quantize.py:127-198)
// with its gradients, and escx_dac_from_latents is the independent per-codebook search (quantize.py:222-255); DESIGN.md section 13.8.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "escx_internal.h"
#include "dac_kernels.h"
#include "dac_x3.h"
#include "dac_grad_kernels.h"
#include "train_kernels.h"
#include "dac_param_grad_kernels.h"

using namespace escx;

namespace {

inline unsigned nblk(long long n, int per = 256) { return (unsigned)((n + per - 1) / per); }
size_t pad64(size_t n) { return (n + 63) / 64 * 64; }
inline int cpad(int C) { return rup(C, 4); }

struct DacLayer {
    int kind = 0;                   // 0: Conv1d, 1: ConvTranspose1d
    int Cin = 0, Cout = 0, K = 0, stride = 1, pad = 0, dil = 1;
    int CinP = 0, Np = 0, Kp = 0;   // operand geometry (Conv1d: Np = rup(Cout, 16), Kp = rup(K * CinP, 16); ConvT: per phase, Kp = rup(2 CinP, 16))
    size_t off_b = 0, off_g = 0, off_v = 0;
    float* W = nullptr; float* bias = nullptr;
    // once a backward has run: the transposed image [NpT = rup(Cin, 16)][KpT = rup(K * cpad(Cout), 16)]; the encoder's strided convolutions hold
    // `stride` phase images [NpT][rup(2 * cpad(Cout), 16)] instead (dac_wt_phase_pack_kernel)
    float* Wt = nullptr;
};
struct DacSnake { int C = 0; size_t off = 0; float* a = nullptr; float* inv = nullptr; };

}  // namespace

struct escx_dac_s {
    int device = 0;
    escx_dac_config cfg{};
    int latent = 0, hop = 1;
    std::vector<std::string> keys; std::vector<size_t> offs, numels;
    size_t total = 0;
    // encoder: conv0, per block (3 x (snake, conv7, snake, conv1), snake, strided conv), snake, conv3; decoder: conv0, per block (snake, convT,
    // 3 x residual unit), snake, conv7 -> tanh.  Layers and Snakes are stored in that execution order.
    std::vector<DacLayer> enc, dec; std::vector<DacSnake> enc_sn, dec_sn;
    std::vector<long long> qoffs;          // 6 per stage + 1 codebook per stage
    long long* qoffs_dev = nullptr;
    DacQTables qt{};
    float* wbuf = nullptr; size_t wfloats = 0;
    float* scratch = nullptr; size_t scratch_bytes = 0;
    const float* packed_ptr = nullptr; long long packed_version = -1;
    int snake_maps = ESCX_DAC_SNAKE_MAPS_DEFAULT;   // escx_dac_set_snake_maps: layer classes whose Snake is written to a map first
    int precision = ESCX_PRECISION_FP32;            // escx_dac_set_precision, read at each call
    // escx_dac_set_padding, read at each call.  Off: every convolution runs with padding 0 (CodecMixin.padding = False, base.py:64-80).  The transposed
    // convolutions' phase images depend on the padding, so the mode is part of the pack cache key: packed_padding is the mode wbuf was packed in.
    bool padding = true; int packed_padding = -1;
    // bf16x3: three bf16 planes of the packed convolution weights wbuf[0, conv_floats), plane p at w16 + p * conv_floats.  Allocated at the first
    // call in that mode; w16_valid is cleared by every re-pack of the fp32 image and set by refresh_w16, so the image can never be older than wbuf.
    __bf16* w16 = nullptr; size_t conv_floats = 0; bool w16_valid = false;
    int* counts = nullptr; size_t counts_cap = 0;   // per-clip stage counts / snapshot stages of the _ex calls, uploaded on the call's stream
    std::vector<int32_t> len_host;                  // the _lengths calls: the host image of their length tables, alive while the upload is in flight
    // escx_dac_decode_backward: the decoder's transposed weight images, allocated (zeroed) at the first backward of the handle; wt_valid is cleared by
    // every re-pack of wbuf and set by refresh_wt, as w16_valid is.  Calls that never differentiate pay nothing.
    float* wt = nullptr; bool wt_valid = false;
    float* wte = nullptr; bool wte_valid = false;   // escx_dac_encode_backward: the same for the encoder's layers
    // escx_dac_set_grad_precision, read at each backward call.  bf16x3: three bf16 planes of the whole transposed image wt[0, wt_floats) (plane p at
    // wt16 + p * wt_floats) and of wte likewise, allocated at the first backward in that mode and split from whatever fp32 image is current:
    // wt16_valid / wte16_valid are cleared wherever wt_valid / wte_valid are and set by refresh_wt16.  Handles that never ask for the mode pay nothing.
    int grad_precision = ESCX_PRECISION_FP32;
    size_t wt_floats = 0, wte_floats = 0;
    __bf16* wt16 = nullptr; bool wt16_valid = false;
    __bf16* wte16 = nullptr; bool wte16_valid = false;
    // escx_dac_decode_backward_params: the slices' partial dW tiles, the staged dW and the bias / alpha partial rows; allocated at the first
    // parameter backward of the handle, sized from the configuration alone (param_ws_plan)
    float* pw = nullptr;
    // escx_dac_set_param_grad_precision, read at each parameter backward.  bf16x3: the partial tiles of the 128 x 128 split-operand dW contraction
    // (param_ws16_plan), a second allocation made at the first parameter backward in that mode; the staged dW and the column partials stay in pw.
    int param_grad_precision = ESCX_PRECISION_FP32;
    float* pw16 = nullptr;
    // escx_dac_encode_backward_params: the same two workspaces for the encoder's layers and the quantiser's projections, allocated at the first
    // encode parameter backward of the handle (in that mode), sized from the configuration alone (enc_param_ws_plan)
    float* pwe = nullptr; float* pwe16 = nullptr;
};

namespace {

DacLayer make_layer(int kind, int Cin, int Cout, int K, int stride, int pad, int dil) {
    DacLayer l; l.kind = kind; l.Cin = Cin; l.Cout = Cout; l.K = K; l.stride = stride; l.pad = pad; l.dil = dil;
    l.CinP = cpad(Cin); l.Np = rup(Cout, 16);
    l.Kp = kind == 0 ? rup(K * l.CinP, 16) : rup(2 * l.CinP, 16);
    return l;
}
size_t layer_floats(const DacLayer& l) { return pad64((size_t)(l.kind ? l.stride : 1) * l.Np * l.Kp) + pad64(l.Np); }

void add_key(escx_dac_s* d, const std::string& k, size_t n, size_t* off) {
    d->keys.push_back(k); d->offs.push_back(*off); d->numels.push_back(n); *off += n;
}
void add_conv(escx_dac_s* d, std::vector<DacLayer>& v, const std::string& p, DacLayer l, size_t* off) {
    const size_t nv = (size_t)l.Cout * l.Cin * l.K;
    l.off_b = *off; add_key(d, p + "bias", l.Cout, off);
    l.off_g = *off; add_key(d, p + "weight_g", l.kind ? l.Cin : l.Cout, off);
    l.off_v = *off; add_key(d, p + "weight_v", nv, off);
    v.push_back(l);
}
void add_snake(escx_dac_s* d, std::vector<DacSnake>& v, const std::string& p, int C, size_t* off) {
    DacSnake s; s.C = C; s.off = *off; add_key(d, p + "alpha", C, off); v.push_back(s);
}
void add_res(escx_dac_s* d, std::vector<DacLayer>& L, std::vector<DacSnake>& S, const std::string& p, int C, int dil, size_t* off) {
    add_snake(d, S, p + "block.0.", C, off);
    add_conv(d, L, p + "block.1.", make_layer(0, C, C, 7, 1, 3 * dil, dil), off);
    add_snake(d, S, p + "block.2.", C, off);
    add_conv(d, L, p + "block.3.", make_layer(0, C, C, 1, 1, 0, 1), off);
}

// torch's length formulas.  Conv1d floors (T + 2p - dil (K - 1) - 1) / s; a negative numerator means no output frame (0 here, where the
// reference's layer gives an empty or invalid tensor) - C++ division would truncate it toward zero and report one frame.
// `padding` false: the layer's padding is taken as 0 (a ConvTranspose1d then gives (T + 1) * stride).
int conv_out_len(int T, const DacLayer& l, bool padding) {
    const int pad = padding ? l.pad : 0;
    if (l.kind == 0) {
        const int num = T + 2 * pad - l.dil * (l.K - 1) - 1;
        return num < 0 ? 0 : num / l.stride + 1;
    }
    return (T - 1) * l.stride - 2 * pad + l.K;
}

int pack(escx_dac_s* d, const float* flat, long long version, hipStream_t st) {
    if (version >= 0 && version == d->packed_version && flat == d->packed_ptr && (int)d->padding == d->packed_padding) return 0;
    d->packed_version = version; d->packed_ptr = flat; d->packed_padding = d->padding; d->w16_valid = false; d->wt_valid = false; d->wte_valid = false;
    d->wt16_valid = false; d->wte16_valid = false;
    for (auto* L : {&d->enc, &d->dec})
        for (DacLayer& l : *L) {
            if (l.kind == 0)
                hipLaunchKernelGGL(dac_wn_conv_kernel, dim3(l.Cout), dim3(256), 0, st, flat + l.off_v, flat + l.off_g, flat + l.off_b, l.W, l.bias, l.Cin, l.K, l.CinP, l.Kp);
            else {
                hipLaunchKernelGGL(dac_wn_convt_kernel, dim3(l.Cin), dim3(256), 0, st, flat + l.off_v, flat + l.off_g, l.W, l.Cout, l.stride, d->padding ? l.pad : 0, l.CinP, l.Np, l.Kp);
                ESCX_HIP(hipMemcpyAsync(l.bias, flat + l.off_b, l.Cout * sizeof(float), hipMemcpyDeviceToDevice, st));
            }
        }
    for (auto* S : {&d->enc_sn, &d->dec_sn})
        for (DacSnake& s : *S) hipLaunchKernelGGL(dac_snake_pack_kernel, dim3(nblk(s.C)), dim3(256), 0, st, flat + s.off, s.a, s.inv, s.C);
    const int S = d->cfg.n_codebooks, D = d->latent, dd = d->cfg.codebook_dim, K = d->cfg.codebook_size;
    hipLaunchKernelGGL(dac_wn_inproj_kernel, dim3(S * dd), dim3(256), 0, st, flat, (const long long*)d->qoffs_dev, d->qt, D, dd);
    hipLaunchKernelGGL(dac_qtables_kernel, dim3(nblk((long long)S * (D + K))), dim3(256), 0, st, flat, (const long long*)d->qoffs_dev, d->qt, S, D, dd, K);
    return launch_ok("dac_pack");
}

// The three-term image of the packed convolution weights, for the calls that run in bf16x3.  Called after pack() on the same stream: it splits
// whatever fp32 image is current, once per re-pack (in-place parameter changes, another buffer) and once after the mode is first switched on.
int refresh_w16(escx_dac_s* d, hipStream_t st) {
    if (d->precision != ESCX_PRECISION_BF16X3 || d->w16_valid) return 0;
    if (!d->w16) ESCX_HIP(hipMalloc((void**)&d->w16, 3 * d->conv_floats * sizeof(__bf16)));
    const size_t n4 = d->conv_floats / 4;
    hipLaunchKernelGGL(split3_bf16_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 4096)), dim3(256), 0, st, (const float*)d->wbuf, d->w16, n4, d->conv_floats);
    d->w16_valid = true;
    return launch_ok("dac_split_weights");
}

// Which layers run on the bf16 matrix cores in bf16x3, by geometry alone: every convolution with more than one input and more than one output
// channel.  The one-channel first layer (K = 7 real values per row) and the one-channel tanh layer (one real output column) stay on the fp32 MFMA,
// which is the same arithmetic grade; DESIGN.md section 13 has the measurements.
inline bool x3_layer(const DacLayer& l) { return l.Cin > 1 && l.Cout > 1; }

int ensure_scratch(escx_dac_s* d, size_t bytes) {
    if (d->scratch_bytes >= bytes) return 0;
    ESCX_HIP(hipDeviceSynchronize());
    if (d->scratch) ESCX_HIP(hipFree(d->scratch));
    d->scratch = nullptr; d->scratch_bytes = 0;
    ESCX_HIP(hipMalloc((void**)&d->scratch, bytes));
    d->scratch_bytes = bytes;
    return 0;
}

// What one pass needs besides the layer: the handle's Snake placement, a map-sized buffer for a Snaked copy, the stream, the padding mode.
struct Run { int snake_maps; float* tmp; hipStream_t st; const float* wbuf; const __bf16* w16; size_t plane; bool padding; };     // w16 == nullptr: fp32 mode

// The cropped skip of a ResidualUnit without padding: res has Tres rows per clip and is read `off` rows in (DacEpiCrop)
struct Crop { int Tres, off; };

template <class Ld, class Epi>
void launch_conv(const Run& run, const DacLayer& l, const __bf16* W16, const float* W, const Ld& ld, const Epi& ep) {
    const long long tiles = (long long)((ld.M + 127) / 128) * ((l.Np + 95) / 96);
    if (W16) launch_dac_x3(ld, W16, run.plane, ld.M, l.Np, l.Kp, ep, run.st);
    else if (tiles >= 512) launch_gemm<128>(ld, W, ld.M, l.Np, l.Kp, ep, run.st);
    else launch_gemm<64>(ld, W, ld.M, l.Np, l.Kp, ep, run.st);
}

// out = conv(snake?(x)) over (B, Tin, CinP) -> (B, Tout, cpad(Cout)) [+ res]; ConvT: one GEMM per output phase.  Snake is applied while the
// operand is staged, or - for the layer classes set in snake_maps - once per element into r.tmp, which the GEMM then reads plain (bitwise the
// same operand either way).  The padding is the layer's, or 0 when run.padding is off; `crop` (Conv1d only) selects the cropped residual.
void run_layer(const Run& run, int cls, const DacLayer& l, const DacSnake* sn, const float* x, int B, int Tin, float* out, int Tout, const float* res,
               int tanh_out, const Crop* crop = nullptr) {
    const hipStream_t st = run.st;
    if (sn && ((run.snake_maps >> cls) & 1)) {
        const long long n4 = (long long)B * Tin * l.CinP / 4;
        hipLaunchKernelGGL(dac_snake_map_kernel, dim3(nblk(n4)), dim3(256), 0, st, x, sn->a, sn->inv, run.tmp, n4, l.CinP / 4);
        x = run.tmp; sn = nullptr;
    }
    const int pad = run.padding ? l.pad : 0;
    const int phases = l.kind ? l.stride : 1;
    const __bf16* W16 = (run.w16 && x3_layer(l)) ? run.w16 + (l.W - run.wbuf) : nullptr;
    for (int r = 0; r < phases; ++r) {
        DacConvA ld{};
        ld.x = x; ld.alpha = sn ? sn->a : nullptr; ld.inv = sn ? sn->inv : nullptr; ld.Tin = Tin; ld.Cp = l.CinP; ld.dCp = FastDiv(l.CinP);
        DacEpi ep{};
        ep.out = out; ep.res = res; ep.Cp = tanh_out ? 4 : cpad(l.Cout); ep.Tmap = Tout; ep.tanh_out = tanh_out;
        if (l.kind == 0) {
            ld.Trows = Tout; ld.rs = l.stride; ld.r0 = -pad; ld.td = l.dil; ld.ntaps = l.K;
            ep.os = 1; ep.o0 = 0; ep.Trows = Tout; ep.bias = l.bias;
            ld.M = B * Tout; ld.dT = FastDiv(Tout); ep.dT = ld.dT;
            if (crop) {
                DacEpiCrop ec{};
                ec.out = out; ec.bias = l.bias; ec.res = res; ec.Cp = cpad(l.Cout); ec.Trows = Tout; ec.Tres = crop->Tres; ec.off = crop->off; ec.dT = ld.dT;
                launch_conv(run, l, W16, l.W, ld, ec);
            } else launch_conv(run, l, W16, l.W, ld, ep);
        } else {
            const int s = l.stride, Q = r < Tout ? (Tout - r + s - 1) / s : 0;
            if (Q == 0) continue;
            ld.Trows = Q; ld.rs = 1; ld.r0 = (r + pad) / s; ld.td = -1; ld.ntaps = 2;
            ep.os = s; ep.o0 = r; ep.Trows = Q; ep.bias = l.bias;
            ld.M = B * Q; ld.dT = FastDiv(Q); ep.dT = ld.dT;
            launch_conv(run, l, W16 ? W16 + (size_t)r * l.Np * l.Kp : nullptr, l.W + (size_t)r * l.Np * l.Kp, ld, ep);
        }
    }
}

// ResidualUnit on x: h = conv7_dil(snake(x)); x = crop(x) + conv1(snake(h))   (dac.py:24-41).  With padding the length is kept, the crop never
// triggers and the unit runs in place.  Without it h and the result have T - 6 dil rows and the skip is x cropped by 3 dil on each side: the
// result goes to the free map y (a lane reads x[t + 3 dil] while another workgroup would write x[t]) and the two maps swap; T becomes the new length.
void run_res(const Run& run, const DacLayer* L, const DacSnake* S, float*& x, float*& y, float* h, int B, int& T) {
    if (run.padding) {
        run_layer(run, ESCX_DAC_SNAKE_RES7, L[0], &S[0], x, B, T, h, T, nullptr, 0);
        run_layer(run, ESCX_DAC_SNAKE_RES1, L[1], &S[1], h, B, T, x, T, x, 0);
        return;
    }
    const int T2 = conv_out_len(T, L[0], false);
    const Crop crop{T, (T - T2) / 2};
    run_layer(run, ESCX_DAC_SNAKE_RES7, L[0], &S[0], x, B, T, h, T2, nullptr, 0);
    run_layer(run, ESCX_DAC_SNAKE_RES1, L[1], &S[1], h, B, T2, y, T2, x, 0, &crop);
    std::swap(x, y); T = T2;
}

size_t map_floats(int B, int T, int C) { return pad64((size_t)B * T * cpad(C)); }

// Lengths through the encoder / decoder under the padding in effect: the output length, or 0 as soon as any layer would give no row (without
// padding the receptive field is hundreds to thousands of samples; no kernel ever sees a non-positive row count).  *mx: the largest map of the
// pass for a batch of B, in floats; the scratch holds four of them (x, y, h and the Snaked copy).
int enc_walk(const escx_dac_s* d, bool padding, int B, int L, size_t* mx) {
    size_t m = map_floats(B, L, 1);
    int C = d->cfg.encoder_dim, T = conv_out_len(L, d->enc[0], padding);
    if (T < 1) return 0;
    m = std::max(m, map_floats(B, T, C));
    for (int i = 0; i < d->cfg.n_encoder_rates; ++i) {
        const DacLayer* Lb = &d->enc[1 + i * 7];
        for (int j = 0; j < 3; ++j) { T = conv_out_len(T, Lb[2 * j], padding); if (T < 1) return 0; }      // the 1x1 convolution keeps the length
        T = conv_out_len(T, Lb[6], padding); C *= 2;
        if (T < 1) return 0;
        m = std::max(m, map_floats(B, T, C));
    }
    T = conv_out_len(T, d->enc.back(), padding);
    if (T < 1) return 0;
    if (mx) *mx = std::max(m, map_floats(B, T, d->latent));
    return T;
}
int dec_walk(const escx_dac_s* d, bool padding, int B, int T, size_t* mx) {
    size_t m = map_floats(B, T, d->latent);
    int C = d->cfg.decoder_dim;
    T = conv_out_len(T, d->dec[0], padding);
    if (T < 1) return 0;
    m = std::max(m, map_floats(B, T, C));
    for (int i = 0; i < d->cfg.n_decoder_rates; ++i) {
        const DacLayer* Lb = &d->dec[1 + i * 7];
        T = conv_out_len(T, Lb[0], padding); C /= 2;
        if (T < 1) return 0;
        m = std::max(m, map_floats(B, T, C));
        for (int j = 0; j < 3; ++j) { T = conv_out_len(T, Lb[1 + 2 * j], padding); if (T < 1) return 0; }
    }
    T = conv_out_len(T, d->dec.back(), padding);
    if (T < 1) return 0;
    if (mx) *mx = m;
    return T;
}

// floor and ceiling of a / b for b > 0 and any a (C++ division truncates toward zero)
inline long long floor_div(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// CodecMixin.get_output_length (base.py:108-123): every convolution in module order, no padding, floor at every layer (negative values included,
// as get_delay calls it with 0).  The quantiser's 1x1 projections sit between encoder and decoder and change nothing.
long long ref_output_length(const escx_dac_s* d, long long L) {
    for (auto* V : {&d->enc, &d->dec})
        for (const DacLayer& l : *V) {
            const long long reach = (long long)l.dil * (l.K - 1) + 1;
            L = l.kind == 0 ? floor_div(L - reach, l.stride) + 1 : (L - 1) * l.stride + reach;
        }
    return L;
}

// One chunked-compress pass (escx_dac_encode_chunks): where the staged input map comes from instead of a (B, L) audio buffer
struct ChunkSrc { const float* signal; long long n_signal; int n_chunks, hop; long long lead; };

// Host counts -> the handle's device buffer on the call's stream (as rvq_upload of escx_api.cpp does for RVQCodecs); nullptr stays nullptr.
int upload_counts(escx_dac_s* d, const int32_t* host, int count, const int** dev, hipStream_t st) {
    *dev = nullptr;
    if (!host) return 0;
    if (d->counts_cap < (size_t)count) {
        ESCX_HIP(hipDeviceSynchronize());
        if (d->counts) ESCX_HIP(hipFree(d->counts));
        d->counts = nullptr; d->counts_cap = 0;
        const size_t cap = pad64((size_t)count);
        ESCX_HIP(hipMalloc((void**)&d->counts, cap * sizeof(int)));
        d->counts_cap = cap;
    }
    ESCX_HIP(hipMemcpyAsync(d->counts, host, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, st));
    *dev = d->counts;
    return 0;
}

template <bool FROM_CODES, int EXT>
void launch_rvq(int latent, long long M, const DacQArgs& qa, hipStream_t st) {
    const int J = (latent + 63) / 64;
    const dim3 g(nblk(M, 4)), blk(256);
    if (J <= 1) hipLaunchKernelGGL((dac_rvq_kernel<1, FROM_CODES, EXT>), g, blk, 0, st, qa);
    else if (J <= 2) hipLaunchKernelGGL((dac_rvq_kernel<2, FROM_CODES, EXT>), g, blk, 0, st, qa);
    else if (J <= 4) hipLaunchKernelGGL((dac_rvq_kernel<4, FROM_CODES, EXT>), g, blk, 0, st, qa);
    else if (J <= 8) hipLaunchKernelGGL((dac_rvq_kernel<8, FROM_CODES, EXT>), g, blk, 0, st, qa);
    else hipLaunchKernelGGL((dac_rvq_kernel<16, FROM_CODES, EXT>), g, blk, 0, st, qa);
}

// per-clip counts of an _ex call: each in [1, n_codebooks] and at most the n slots the call has
int check_clip_counts(escx_dac_s* d, const int32_t* clip_n, int B, int n) {
    for (int b = 0; b < B; ++b) {
        if (clip_n[b] < 1 || clip_n[b] > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "clip_n[%d]=%d outside [1, %d]", b, clip_n[b], d->cfg.n_codebooks);
        if (clip_n[b] > n) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "clip_n[%d]=%d above the %d code slots of the call", b, clip_n[b], n);
    }
    return 0;
}

int check_args(escx_dac_s* d, const float* flat, int B) {
    if (!d || !flat || B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    ESCX_HIP(hipSetDevice(d->device));
    return 0;
}

}  // namespace

extern "C" int escx_dac_create(const escx_dac_config* cfg, int device, escx_dac* out) {
    if (!cfg || !out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null argument");
    const escx_dac_config& c = *cfg;
    if (c.encoder_dim < 1 || c.decoder_dim < 1 || c.n_codebooks < 1 || c.codebook_size < 1 || c.codebook_dim < 1 || c.n_encoder_rates < 1 || c.n_decoder_rates < 1 ||
        c.n_encoder_rates > ESCX_DAC_MAX_RATES || c.n_decoder_rates > ESCX_DAC_MAX_RATES || c.latent_dim < 0)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad DAC configuration");
    const int latent = c.latent_dim ? c.latent_dim : c.encoder_dim << c.n_encoder_rates;
    for (int i = 0; i < c.n_encoder_rates; ++i) if (c.encoder_rates[i] < 1 || c.encoder_rates[i] > 16) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "encoder rate %d outside [1, 16]", c.encoder_rates[i]);
    for (int i = 0; i < c.n_decoder_rates; ++i) if (c.decoder_rates[i] < 1 || c.decoder_rates[i] > 16) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "decoder rate %d outside [1, 16]", c.decoder_rates[i]);
    if (c.decoder_dim % (1 << c.n_decoder_rates)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "decoder_dim %d is not divisible by 2^%d", c.decoder_dim, c.n_decoder_rates);
    if (latent > 1024 || latent % 4) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "latent_dim %d: the fused quantiser covers multiples of 4 up to 1024", latent);
    if (c.codebook_dim > DAC_DMAX) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "codebook_dim %d above %d", c.codebook_dim, DAC_DMAX);
    if (c.codebook_size > 65536) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "codebook_size %d above 65536", c.codebook_size);
    if ((long long)c.decoder_dim * 7 > (1 << 20) || (long long)(c.encoder_dim << c.n_encoder_rates) * 7 > (1 << 20)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "channel count too large");
    escx_dac_s* d = new escx_dac_s();
    d->device = device; d->cfg = c; d->latent = latent;
    d->hop = 1; for (int i = 0; i < c.n_encoder_rates; ++i) d->hop *= c.encoder_rates[i];
    size_t off = 0;
    // encoder (dac.py:64-91)
    int C = c.encoder_dim;
    add_conv(d, d->enc, "encoder.block.0.", make_layer(0, 1, C, 7, 1, 3, 1), &off);
    for (int i = 0; i < c.n_encoder_rates; ++i) {
        const int s = c.encoder_rates[i];
        const std::string p = "encoder.block." + std::to_string(i + 1) + ".block.";
        const int dl[3] = {1, 3, 9};
        for (int j = 0; j < 3; ++j) add_res(d, d->enc, d->enc_sn, p + std::to_string(j) + ".", C, dl[j], &off);
        add_snake(d, d->enc_sn, p + "3.", C, &off);
        add_conv(d, d->enc, p + "4.", make_layer(0, C, 2 * C, 2 * s, s, (s + 1) / 2, 1), &off);
        C *= 2;
    }
    const int nE = c.n_encoder_rates;
    add_snake(d, d->enc_sn, "encoder.block." + std::to_string(nE + 1) + ".", C, &off);
    add_conv(d, d->enc, "encoder.block." + std::to_string(nE + 2) + ".", make_layer(0, C, latent, 3, 1, 1, 1), &off);
    // quantiser (quantize.py:17-33, 127-150)
    const int S = c.n_codebooks, dd = c.codebook_dim, K = c.codebook_size;
    for (int i = 0; i < S; ++i) {
        const std::string p = "quantizer.quantizers." + std::to_string(i) + ".";
        long long o[7];
        o[0] = (long long)off; add_key(d, p + "in_proj.bias", dd, &off);
        o[1] = (long long)off; add_key(d, p + "in_proj.weight_g", dd, &off);
        o[2] = (long long)off; add_key(d, p + "in_proj.weight_v", (size_t)dd * latent, &off);
        o[3] = (long long)off; add_key(d, p + "out_proj.bias", latent, &off);
        o[4] = (long long)off; add_key(d, p + "out_proj.weight_g", latent, &off);
        o[5] = (long long)off; add_key(d, p + "out_proj.weight_v", (size_t)latent * dd, &off);
        o[6] = (long long)off; add_key(d, p + "codebook.weight", (size_t)K * dd, &off);
        for (int k = 0; k < 6; ++k) d->qoffs.push_back(o[k]);
        d->qoffs.push_back(o[6]);            // re-ordered below: 6 per stage, then the codebooks
    }
    {
        std::vector<long long> q; for (int i = 0; i < S; ++i) for (int k = 0; k < 6; ++k) q.push_back(d->qoffs[7 * i + k]);
        for (int i = 0; i < S; ++i) q.push_back(d->qoffs[7 * i + 6]);
        d->qoffs = q;
    }
    // decoder (dac.py:113-145)
    C = c.decoder_dim;
    add_conv(d, d->dec, "decoder.model.0.", make_layer(0, latent, C, 7, 1, 3, 1), &off);
    for (int i = 0; i < c.n_decoder_rates; ++i) {
        const int s = c.decoder_rates[i];
        const std::string p = "decoder.model." + std::to_string(i + 1) + ".block.";
        add_snake(d, d->dec_sn, p + "0.", C, &off);
        add_conv(d, d->dec, p + "1.", make_layer(1, C, C / 2, 2 * s, s, (s + 1) / 2, 1), &off);
        const int dl[3] = {1, 3, 9};
        for (int j = 0; j < 3; ++j) add_res(d, d->dec, d->dec_sn, p + std::to_string(j + 2) + ".", C / 2, dl[j], &off);
        C /= 2;
    }
    const int nD = c.n_decoder_rates;
    add_snake(d, d->dec_sn, "decoder.model." + std::to_string(nD + 1) + ".", C, &off);
    add_conv(d, d->dec, "decoder.model." + std::to_string(nD + 2) + ".", make_layer(0, C, 1, 7, 1, 3, 1), &off);
    d->total = off;
    // packed operands
    size_t wf = 0;
    for (auto* L : {&d->enc, &d->dec}) for (DacLayer& l : *L) wf += layer_floats(l);
    for (auto* Sn : {&d->enc_sn, &d->dec_sn}) for (DacSnake& s : *Sn) wf += 2 * pad64(cpad(s.C));
    const size_t qD = (size_t)S * dd * latent, qK = (size_t)S * K;
    wf += 2 * pad64(qD) + pad64((size_t)S * dd) + pad64((size_t)S * latent) + 2 * pad64(qK * dd) + pad64(qK);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { delete d; ESCX_FAIL(ESCX_ERR_HIP, "hipSetDevice failed"); }
    if (hipMalloc((void**)&d->wbuf, wf * sizeof(float)) != hipSuccess || hipMalloc((void**)&d->qoffs_dev, d->qoffs.size() * sizeof(long long)) != hipSuccess) {
        escx_dac_destroy(d); ESCX_FAIL(ESCX_ERR_HIP, "hipMalloc of the DAC weights failed");
    }
    (void)hipMemset(d->wbuf, 0, wf * sizeof(float));
    (void)hipMemcpy(d->qoffs_dev, d->qoffs.data(), d->qoffs.size() * sizeof(long long), hipMemcpyHostToDevice);
    d->wfloats = wf;
    size_t cur = 0;
    auto take = [&](size_t n) { float* p = d->wbuf + cur; cur += pad64(n); return p; };
    for (auto* L : {&d->enc, &d->dec})
        for (DacLayer& l : *L) { l.W = take((size_t)(l.kind ? l.stride : 1) * l.Np * l.Kp); l.bias = take(l.Np); }
    d->conv_floats = cur;                   // the layers come first in wbuf: the region the bf16x3 image mirrors
    for (auto* Sn : {&d->enc_sn, &d->dec_sn}) for (DacSnake& s : *Sn) { s.a = take(cpad(s.C)); s.inv = take(cpad(s.C)); }
    d->qt.win = take(qD); d->qt.bin = take((size_t)S * dd); d->qt.wout = take(qD); d->qt.bout = take((size_t)S * latent);
    d->qt.cbraw = take(qK * dd); d->qt.cbn = take(qK * dd); d->qt.c2 = take(qK);
    *out = d;
    return ESCX_OK;
}

extern "C" void escx_dac_destroy(escx_dac d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->wbuf) (void)hipFree(d->wbuf);
    if (d->w16) (void)hipFree(d->w16);
    if (d->wt) (void)hipFree(d->wt);
    if (d->wte) (void)hipFree(d->wte);
    if (d->wt16) (void)hipFree(d->wt16);
    if (d->wte16) (void)hipFree(d->wte16);
    if (d->pw) (void)hipFree(d->pw);
    if (d->pw16) (void)hipFree(d->pw16);
    if (d->pwe) (void)hipFree(d->pwe);
    if (d->pwe16) (void)hipFree(d->pwe16);
    if (d->qoffs_dev) (void)hipFree(d->qoffs_dev);
    if (d->scratch) (void)hipFree(d->scratch);
    if (d->counts) (void)hipFree(d->counts);
    delete d;
}

extern "C" int escx_dac_param_count(escx_dac d) { return d ? (int)d->keys.size() : 0; }
extern "C" const char* escx_dac_param_key(escx_dac d, int i) { return (d && i >= 0 && i < (int)d->keys.size()) ? d->keys[i].c_str() : nullptr; }
extern "C" int64_t escx_dac_param_offset(escx_dac d, int i) { return (d && i >= 0 && i < (int)d->offs.size()) ? (int64_t)d->offs[i] : -1; }
extern "C" int64_t escx_dac_param_numel(escx_dac d, int i) { return (d && i >= 0 && i < (int)d->numels.size()) ? (int64_t)d->numels[i] : -1; }
extern "C" int64_t escx_dac_param_total(escx_dac d) { return d ? (int64_t)d->total : 0; }

extern "C" int escx_dac_set_snake_maps(escx_dac d, int mask) {
    if (!d) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null handle");
    if (mask < 0 || mask > ESCX_DAC_SNAKE_ALL) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "snake map mask %d outside [0, %d]", mask, ESCX_DAC_SNAKE_ALL);
    d->snake_maps = mask;
    return ESCX_OK;
}
extern "C" int escx_dac_get_snake_maps(escx_dac d) { return d ? d->snake_maps : -1; }

extern "C" int escx_dac_set_precision(escx_dac d, int mode) {
    if (!d) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null handle");
    if (mode == ESCX_PRECISION_F16X2)
        ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "DAC has no f16x2 mode: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) and Snake outputs "
                                        "have none; bf16x3 keeps fp32's exponent range and needs no bound");
    if (mode != ESCX_PRECISION_FP32 && mode != ESCX_PRECISION_BF16X3) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "DAC precision %d: expected fp32 (0) or bf16x3 (3)", mode);
    d->precision = mode;
    return ESCX_OK;
}
extern "C" int escx_dac_get_precision(escx_dac d) { return d ? d->precision : -1; }

extern "C" int escx_dac_set_grad_precision(escx_dac d, int mode) {
    if (!d) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null handle");
    if (mode == ESCX_PRECISION_F16X2)
        ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "DAC has no f16x2 backward: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) and neither "
                                        "the output gradients nor Snake outputs have one; bf16x3 keeps fp32's exponent range and needs no bound");
    if (mode != ESCX_PRECISION_FP32 && mode != ESCX_PRECISION_BF16X3) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "DAC grad precision %d: expected fp32 (0) or bf16x3 (3)", mode);
    d->grad_precision = mode;
    return ESCX_OK;
}
extern "C" int escx_dac_get_grad_precision(escx_dac d) { return d ? d->grad_precision : -1; }

extern "C" int escx_dac_set_param_grad_precision(escx_dac d, int mode) {
    if (!d) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null handle");
    if (mode == ESCX_PRECISION_F16X2)
        ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "DAC has no f16x2 weight gradient: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) and "
                                        "neither the output gradients nor Snake outputs have one; bf16x3 keeps fp32's exponent range and needs no bound");
    if (mode != ESCX_PRECISION_FP32 && mode != ESCX_PRECISION_BF16X3)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "DAC param grad precision %d: expected fp32 (0) or bf16x3 (3)", mode);
    d->param_grad_precision = mode;
    return ESCX_OK;
}
extern "C" int escx_dac_get_param_grad_precision(escx_dac d) { return d ? d->param_grad_precision : -1; }

extern "C" int escx_dac_set_padding(escx_dac d, int on) {
    if (!d) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null handle");
    if (on != 0 && on != 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "padding %d: expected 0 or 1", on);
    d->padding = on != 0;
    return ESCX_OK;
}
extern "C" int escx_dac_get_padding(escx_dac d) { return d ? (int)d->padding : -1; }

extern "C" int escx_dac_output_length(escx_dac d, int n_samples) { return d ? (int)ref_output_length(d, n_samples) : 0; }

extern "C" int escx_dac_delay(escx_dac d) {
    if (!d) return -1;
    const long long l_out = ref_output_length(d, 0);
    long long L = l_out;
    for (auto* V : {&d->dec, &d->enc})
        for (auto it = V->rbegin(); it != V->rend(); ++it) {
            const long long reach = (long long)it->dil * (it->K - 1) + 1;
            L = it->kind == 1 ? ceil_div(L - reach, it->stride) + 1 : (L - 1) * it->stride + reach;
        }
    return (int)floor_div(L - l_out, 2);
}

extern "C" int escx_dac_num_frames(escx_dac d, int n_samples) {
    if (!d || n_samples < 1) return 0;
    return enc_walk(d, d->padding, 1, n_samples, nullptr);
}
extern "C" int escx_dac_output_samples(escx_dac d, int n_frames) {
    if (!d || n_frames < 1) return 0;
    return dec_walk(d, d->padding, 1, n_frames, nullptr);
}

extern "C" int escx_dac_encode(escx_dac d, const float* flat, int64_t version, const float* audio, int B, int L, int n_q, float* z, int64_t* codes,
                               float* latents, float* losses, void* stream) {
    return escx_dac_encode_ex(d, flat, version, audio, B, L, n_q, nullptr, nullptr, 0, z, codes, latents, losses, nullptr, stream);
}

namespace {

// escx_dac_encode_ex and escx_dac_encode_chunks: everything but where the staged (B, L, 4) input map comes from
int encode_impl(escx_dac d, const float* flat, int64_t version, const float* audio, const ChunkSrc* chunks, int B, int L, int n_q, const int32_t* clip_n,
                const int32_t* snap_n, int n_snaps, float* z, int64_t* codes, float* latents, float* losses, float* zsnap, void* stream) {
    int rc = 0;
    if (!z || !codes || !latents || !losses || n_q < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (clip_n && snap_n) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "per-clip counts and snapshots are not combined in one call");
    if (clip_n && n_q > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d code slots above the %d codebooks", n_q, d->cfg.n_codebooks);
    const int n = std::min(n_q, d->cfg.n_codebooks);
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    if (snap_n) {
        if (n_snaps < 1 || !zsnap) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "snapshots need n_snaps >= 1 and a zsnap buffer");
        for (int r = 0; r < n_snaps; ++r)
            if (snap_n[r] < 1 || snap_n[r] > n || (r && snap_n[r] <= snap_n[r - 1]))
                ESCX_FAIL(ESCX_ERR_INVALID_ARG, "snap_n[%d]=%d: strictly increasing stage counts in [1, %d] expected", r, snap_n[r], n);
    }
    const bool padding = d->padding;
    size_t mf = 0;
    const int Tz = L < 1 ? 0 : enc_walk(d, padding, B, L, &mf);
    if (Tz < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d samples give no latent frame (the hop is %d, padding %s)", L, d->hop, padding ? "on" : "off");
    hipStream_t st = (hipStream_t)stream;
    if ((unsigned long long)mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d samples: a feature map above 2^32 elements", B, L);
    const size_t M = (size_t)B * Tz;
    const size_t lossf = pad64((size_t)n * M) + pad64((size_t)n * B);
    if ((rc = ensure_scratch(d, (4 * mf + lossf) * sizeof(float)))) return rc;
    const int* cdev; if ((rc = upload_counts(d, clip_n ? clip_n : snap_n, clip_n ? B : n_snaps, &cdev, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_w16(d, st))) return rc;
    float* x = d->scratch; float* y = x + mf; float* h = y + mf; float* lossb = h + mf + mf;
    const Run run{d->snake_maps, h + mf, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, padding};
    if (chunks)
        hipLaunchKernelGGL(dac_chunk_in_kernel, dim3(nblk((long long)B * L)), dim3(256), 0, st, chunks->signal, h, (long long)B * L, chunks->n_signal, chunks->n_chunks, L,
                           chunks->hop, chunks->lead);
    else hipLaunchKernelGGL(dac_wave_in_kernel, dim3(nblk((long long)B * L)), dim3(256), 0, st, audio, h, (long long)B * L);
    const DacLayer* E = d->enc.data(); const DacSnake* SN = d->enc_sn.data();
    int T = conv_out_len(L, E[0], padding);
    run_layer(run, ESCX_DAC_SNAKE_LAST, E[0], nullptr, h, B, L, x, T, nullptr, 0);
    for (int i = 0; i < d->cfg.n_encoder_rates; ++i) {
        const DacLayer* Lb = E + 1 + i * 7; const DacSnake* Sb = SN + i * 7;        // 3 residual units (2 convolutions, 2 Snakes each), Snake, strided conv
        for (int j = 0; j < 3; ++j) run_res(run, Lb + 2 * j, Sb + 2 * j, x, y, h, B, T);
        const DacLayer& sc = Lb[6];
        const int T2 = conv_out_len(T, sc, padding);
        run_layer(run, ESCX_DAC_SNAKE_DOWN, sc, Sb + 6, x, B, T, y, T2, nullptr, 0);
        std::swap(x, y); T = T2;
    }
    const int T3 = conv_out_len(T, E[d->enc.size() - 1], padding);
    run_layer(run, ESCX_DAC_SNAKE_LAST, E[d->enc.size() - 1], SN + d->enc_sn.size() - 1, x, B, T, y, T3, nullptr, 0);
    T = T3;
    DacQArgs qa{};
    qa.t = d->qt; qa.zmap = y; qa.z = z; qa.codes = (long long*)codes; qa.latents = latents; qa.loss = lossb;
    qa.M = (int)M; qa.T = T; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n;
    if (clip_n) { qa.clip_n = cdev; launch_rvq<false, DAC_Q_CLIPS>(d->latent, (long long)M, qa, st); }
    else if (snap_n) { qa.snap_n = cdev; qa.n_snaps = n_snaps; qa.zsnap = zsnap; launch_rvq<false, DAC_Q_SNAPS>(d->latent, (long long)M, qa, st); }
    else launch_rvq<false, DAC_Q_PLAIN>(d->latent, (long long)M, qa, st);
    hipLaunchKernelGGL(dac_loss_kernel, dim3(1), dim3(256), 0, st, lossb, lossb + pad64((size_t)n * M), losses, B, T, n, d->cfg.codebook_dim);
    return launch_ok("escx_dac_encode");
}

}  // namespace

extern "C" int escx_dac_encode_ex(escx_dac d, const float* flat, int64_t version, const float* audio, int B, int L, int n_q, const int32_t* clip_n,
                                  const int32_t* snap_n, int n_snaps, float* z, int64_t* codes, float* latents, float* losses, float* zsnap, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!audio) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    return encode_impl(d, flat, version, audio, nullptr, B, L, n_q, clip_n, snap_n, n_snaps, z, codes, latents, losses, zsnap, stream);
}

extern "C" int escx_dac_encode_chunks(escx_dac d, const float* flat, int64_t version, const float* signal, int rows, int64_t n_signal, int n_chunks, int n_samples,
                                      int hop, int64_t lead, int n_q, float* z, int64_t* codes, float* latents, float* losses, void* stream) {
    int rc = check_args(d, flat, rows); if (rc) return rc;
    if (!signal || n_signal < 1 || n_chunks < 1 || n_samples < 1 || hop < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if ((long long)rows * n_chunks > 0x7fffffffll) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "%d rows x %d chunks in one pass", rows, n_chunks);
    const ChunkSrc src{signal, (long long)n_signal, n_chunks, hop, (long long)lead};
    return encode_impl(d, flat, version, nullptr, &src, rows * n_chunks, n_samples, n_q, nullptr, nullptr, 0, z, codes, latents, losses, nullptr, stream);
}

extern "C" int escx_dac_from_codes(escx_dac d, const float* flat, int64_t version, const int64_t* codes, int B, int n, int T, float* z, float* zp, void* stream) {
    return escx_dac_from_codes_ex(d, flat, version, codes, B, n, T, nullptr, z, zp, stream);
}

extern "C" int escx_dac_from_codes_ex(escx_dac d, const float* flat, int64_t version, const int64_t* codes, int B, int n, int T, const int32_t* clip_n,
                                      float* z, float* zp, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!codes || !z || !zp || T < 1 || n < 1 || n > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument (codes of %d codebooks, %d frames)", n, T);
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int* cdev; if ((rc = upload_counts(d, clip_n, B, &cdev, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st))) return rc;
    DacQArgs qa{};
    qa.t = d->qt; qa.codes_in = (const long long*)codes; qa.z = z; qa.latents = zp;
    qa.M = B * T; qa.T = T; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n;
    if (clip_n) { qa.clip_n = cdev; launch_rvq<true, DAC_Q_CLIPS>(d->latent, (long long)B * T, qa, st); }
    else launch_rvq<true, DAC_Q_PLAIN>(d->latent, (long long)B * T, qa, st);
    return launch_ok("escx_dac_from_codes");
}

extern "C" int escx_dac_decode(escx_dac d, const float* flat, int64_t version, const float* z, int B, int T, float* audio, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!z || !audio || T < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const bool padding = d->padding;
    size_t mf = 0;
    const int Lout = dec_walk(d, padding, B, T, &mf);
    if (Lout < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d latent frames decode to no sample (padding %s)", T, padding ? "on" : "off");
    if ((unsigned long long)mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d frames: a feature map above 2^32 elements", B, T);
    if ((rc = ensure_scratch(d, 4 * mf * sizeof(float)))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_w16(d, st))) return rc;
    float* x = d->scratch; float* y = x + mf; float* h = y + mf;
    const Run run{d->snake_maps, h + mf, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, padding};
    const int Dp = cpad(d->latent);
    hipLaunchKernelGGL(dac_z_in_kernel, dim3(nblk((long long)B * T * Dp)), dim3(256), 0, st, z, h, B, d->latent, Dp, T);
    const DacLayer* Dl = d->dec.data(); const DacSnake* SN = d->dec_sn.data();
    const int T0 = conv_out_len(T, Dl[0], padding);
    run_layer(run, ESCX_DAC_SNAKE_LAST, Dl[0], nullptr, h, B, T, x, T0, nullptr, 0);
    T = T0;
    for (int i = 0; i < d->cfg.n_decoder_rates; ++i) {
        const DacLayer* Lb = Dl + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int T2 = conv_out_len(T, Lb[0], padding);
        run_layer(run, ESCX_DAC_SNAKE_UP, Lb[0], Sb, x, B, T, y, T2, nullptr, 0);
        std::swap(x, y); T = T2;
        for (int j = 0; j < 3; ++j) run_res(run, Lb + 1 + 2 * j, Sb + 1 + 2 * j, x, y, h, B, T);
    }
    run_layer(run, ESCX_DAC_SNAKE_LAST, Dl[d->dec.size() - 1], SN + d->dec_sn.size() - 1, x, B, T, audio, Lout, nullptr, 1);
    return launch_ok("escx_dac_decode");
}

// ---- mixed-length batches: per-clip lengths in encode, from_codes and decode (padding on; dac.py:209-323) ------------------
namespace {

// run_layer for a batch with per-clip lengths: the padded maps' rows per clip (Tin, Tout) and the device tables of the clips' own rows in them.
// The launches are run_layer's - the same tile rule on the padded row count, and no output bit depends on it - with DacConvALen / DacEpiLen.
void run_layer_len(const Run& run, int cls, const DacLayer& l, const DacSnake* sn, const float* x, int B, int Tin, const int* tin, float* out, int Tout,
                   const int* tout, const float* res, int tanh_out) {
    const hipStream_t st = run.st;
    if (sn && ((run.snake_maps >> cls) & 1)) {                  // over the padded map: the rows past a clip's length are stale values nobody reads
        const long long n4 = (long long)B * Tin * l.CinP / 4;
        hipLaunchKernelGGL(dac_snake_map_kernel, dim3(nblk(n4)), dim3(256), 0, st, x, sn->a, sn->inv, run.tmp, n4, l.CinP / 4);
        x = run.tmp; sn = nullptr;
    }
    const int phases = l.kind ? l.stride : 1;
    const __bf16* W16 = (run.w16 && x3_layer(l)) ? run.w16 + (l.W - run.wbuf) : nullptr;
    for (int r = 0; r < phases; ++r) {
        DacConvALen ld{};
        ld.x = x; ld.alpha = sn ? sn->a : nullptr; ld.inv = sn ? sn->inv : nullptr; ld.tin = tin; ld.tout = tout; ld.Tin = Tin; ld.Cp = l.CinP;
        ld.dCp = FastDiv(l.CinP); ld.keep_dead = tanh_out;
        DacEpiLen ep{};
        ep.out = out; ep.res = res; ep.tout = tout; ep.Cp = tanh_out ? 4 : cpad(l.Cout); ep.Tmap = Tout; ep.tanh_out = tanh_out; ep.bias = l.bias;
        if (l.kind == 0) {
            ld.Trows = Tout; ld.rs = l.stride; ld.r0 = -l.pad; ld.td = l.dil; ld.ntaps = l.K; ld.os = 1; ld.o0 = 0;
            ld.M = B * Tout; ld.dT = FastDiv(Tout);
            ep.os = 1; ep.o0 = 0; ep.Trows = Tout; ep.dT = ld.dT;
            launch_conv(run, l, W16, l.W, ld, ep);
        } else {
            const int s = l.stride, Q = r < Tout ? (Tout - r + s - 1) / s : 0;
            if (Q == 0) continue;
            ld.Trows = Q; ld.rs = 1; ld.r0 = (r + l.pad) / s; ld.td = -1; ld.ntaps = 2; ld.os = s; ld.o0 = r;
            ld.M = B * Q; ld.dT = FastDiv(Q);
            ep.os = s; ep.o0 = r; ep.Trows = Q; ep.dT = ld.dT;
            launch_conv(run, l, W16 ? W16 + (size_t)r * l.Np * l.Kp : nullptr, l.W + (size_t)r * l.Np * l.Kp, ld, ep);
        }
    }
}

// ResidualUnit in place (padding on: the length is kept)
void run_res_len(const Run& run, const DacLayer* L, const DacSnake* S, float* x, float* h, int B, int T, const int* tl) {
    run_layer_len(run, ESCX_DAC_SNAKE_RES7, L[0], &S[0], x, B, T, tl, h, T, tl, nullptr, 0);
    run_layer_len(run, ESCX_DAC_SNAKE_RES1, L[1], &S[1], h, B, T, tl, x, T, tl, x, 0);
}

// Per-clip rows at every resolution level of the encoder (level 0: samples; one more level per strided convolution) or the decoder (level 0: latent
// frames; one more per ConvTranspose1d), from conv_out_len per clip: tab[level * B + b].  With the padding on the stride-1 layers keep the length, so
// one table per level serves every layer of it.  false when clip *bad gives no row at some layer.
bool level_table(const escx_dac_s* d, bool decoder, const int32_t* len0, int B, std::vector<int32_t>* tab, int* bad) {
    const std::vector<DacLayer>& V = decoder ? d->dec : d->enc;
    const int levels = 1 + (decoder ? d->cfg.n_decoder_rates : d->cfg.n_encoder_rates);
    tab->assign((size_t)levels * B, 0);
    for (int b = 0; b < B; ++b) {
        int T = len0[b], lv = 0;
        (*tab)[b] = T;
        for (const DacLayer& l : V) {
            const int T2 = conv_out_len(T, l, true);
            if (T2 < 1) { *bad = b; return false; }
            if (l.kind == 1 || l.stride > 1) (*tab)[(size_t)(++lv) * B + b] = T2;
            else if (T2 != T) { *bad = b; return false; }       // never with the padding on
            T = T2;
        }
    }
    return true;
}

int check_lengths(const escx_dac_s* d, const int32_t* len, int B, int hi, const char* what) {
    if (!d->padding) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "per-clip %s need the padding on (escx_dac_set_padding)", what);
    if (!len) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null %s", what);
    for (int b = 0; b < B; ++b)
        if (len[b] < 1 || len[b] > hi) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%s[%d]=%d outside [1, %d]", what, b, len[b], hi);
    return 0;
}

}  // namespace

extern "C" int escx_dac_encode_lengths(escx_dac d, const float* flat, int64_t version, const float* audio, int B, int Lmax, const int32_t* lengths, int pad_multiple,
                                       int n_q, const int32_t* clip_n, float* z, int64_t* codes, float* latents, float* losses, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!audio || !z || !codes || !latents || !losses || n_q < 1 || Lmax < 1 || pad_multiple < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if ((rc = check_lengths(d, lengths, B, Lmax, "lengths"))) return rc;
    if (clip_n && n_q > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d code slots above the %d codebooks", n_q, d->cfg.n_codebooks);
    const int n = std::min(n_q, d->cfg.n_codebooks);
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    // the clips' lengths as the encoder sees them: right-padded with zeros to a multiple of pad_multiple (DAC.preprocess, dac.py:198-207)
    std::vector<int32_t> padded(B), tab;
    int Lmap = 0;
    for (int b = 0; b < B; ++b) {
        const long long p = ((long long)lengths[b] + pad_multiple - 1) / pad_multiple * pad_multiple;
        if (p > 0x7fffffffll) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "lengths[%d]=%d padded to a multiple of %d overflows", b, lengths[b], pad_multiple);
        padded[b] = (int32_t)p; Lmap = std::max(Lmap, padded[b]);
    }
    int bad = 0;
    if (!level_table(d, false, padded.data(), B, &tab, &bad))
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "lengths[%d]=%d samples give no latent frame (the hop is %d)", bad, lengths[bad], d->hop);
    size_t mf = 0;
    const int Tz = enc_walk(d, true, B, Lmap, &mf);
    if (Tz < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d samples give no latent frame (the hop is %d)", Lmap, d->hop);
    if ((unsigned long long)mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d samples: a feature map above 2^32 elements", B, Lmap);
    hipStream_t st = (hipStream_t)stream;
    const size_t M = (size_t)B * Tz;
    const size_t lossf = pad64((size_t)n * M) + pad64((size_t)n * B);
    if ((rc = ensure_scratch(d, (4 * mf + lossf) * sizeof(float)))) return rc;
    // one upload: the lengths as given (what is read of the audio), the level tables, the stage counts
    const int nE = d->cfg.n_encoder_rates;
    std::vector<int32_t>& host = d->len_host;
    host.assign(lengths, lengths + B);
    host.insert(host.end(), tab.begin(), tab.end());
    if (clip_n) host.insert(host.end(), clip_n, clip_n + B);
    const int* dev; if ((rc = upload_counts(d, host.data(), (int)host.size(), &dev, st))) return rc;
    const int* lv = dev + B;                                    // lv + i * B: level i
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_w16(d, st))) return rc;
    float* x = d->scratch; float* y = x + mf; float* h = y + mf; float* lossb = h + mf + mf;
    const Run run{d->snake_maps, h + mf, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, true};
    hipLaunchKernelGGL(dac_wave_in_len_kernel, dim3(nblk((long long)B * Lmap)), dim3(256), 0, st, audio, h, (long long)B * Lmap, Lmax, Lmap, dev);
    const DacLayer* E = d->enc.data(); const DacSnake* SN = d->enc_sn.data();
    int T = Lmap;
    run_layer_len(run, ESCX_DAC_SNAKE_LAST, E[0], nullptr, h, B, T, lv, x, T, lv, nullptr, 0);
    for (int i = 0; i < nE; ++i) {
        const DacLayer* Lb = E + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int* tl = lv + (size_t)i * B;
        for (int j = 0; j < 3; ++j) run_res_len(run, Lb + 2 * j, Sb + 2 * j, x, h, B, T, tl);
        const int T2 = conv_out_len(T, Lb[6], true);
        run_layer_len(run, ESCX_DAC_SNAKE_DOWN, Lb[6], Sb + 6, x, B, T, tl, y, T2, tl + B, nullptr, 0);
        std::swap(x, y); T = T2;
    }
    const int* tz = lv + (size_t)nE * B;
    run_layer_len(run, ESCX_DAC_SNAKE_LAST, E[d->enc.size() - 1], SN + d->enc_sn.size() - 1, x, B, T, tz, y, T, tz, nullptr, 0);
    DacQArgs qa{};
    qa.t = d->qt; qa.zmap = y; qa.z = z; qa.codes = (long long*)codes; qa.latents = latents; qa.loss = lossb;
    qa.M = (int)M; qa.T = T; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n;
    qa.frame_len = tz;
    if (clip_n) { qa.clip_n = tz + B; launch_rvq<false, DAC_Q_LEN | DAC_Q_CLIPS>(d->latent, (long long)M, qa, st); }
    else launch_rvq<false, DAC_Q_LEN | DAC_Q_PLAIN>(d->latent, (long long)M, qa, st);
    hipLaunchKernelGGL(dac_loss_len_kernel, dim3(1), dim3(256), 0, st, lossb, lossb + pad64((size_t)n * M), losses, B, T, n, d->cfg.codebook_dim, tz);
    return launch_ok("escx_dac_encode_lengths");
}

extern "C" int escx_dac_from_codes_lengths(escx_dac d, const float* flat, int64_t version, const int64_t* codes, int B, int n, int Tmax, const int32_t* frame_lengths,
                                           const int32_t* clip_n, float* z, float* zp, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!codes || !z || !zp || Tmax < 1 || n < 1 || n > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument (codes of %d codebooks, %d frames)", n, Tmax);
    if ((rc = check_lengths(d, frame_lengths, B, Tmax, "frame_lengths"))) return rc;
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t>& host = d->len_host;
    host.assign(frame_lengths, frame_lengths + B);
    if (clip_n) host.insert(host.end(), clip_n, clip_n + B);
    const int* dev; if ((rc = upload_counts(d, host.data(), (int)host.size(), &dev, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st))) return rc;
    DacQArgs qa{};
    qa.t = d->qt; qa.codes_in = (const long long*)codes; qa.z = z; qa.latents = zp;
    qa.M = B * Tmax; qa.T = Tmax; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n;
    qa.frame_len = dev;
    if (clip_n) { qa.clip_n = dev + B; launch_rvq<true, DAC_Q_LEN | DAC_Q_CLIPS>(d->latent, (long long)B * Tmax, qa, st); }
    else launch_rvq<true, DAC_Q_LEN | DAC_Q_PLAIN>(d->latent, (long long)B * Tmax, qa, st);
    return launch_ok("escx_dac_from_codes_lengths");
}

extern "C" int escx_dac_decode_lengths(escx_dac d, const float* flat, int64_t version, const float* z, int B, int Tmax, const int32_t* frame_lengths,
                                       const int32_t* sample_caps, float* audio, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!z || !audio || Tmax < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if ((rc = check_lengths(d, frame_lengths, B, Tmax, "frame_lengths"))) return rc;
    std::vector<int32_t> tab;
    int bad = 0;
    if (!level_table(d, true, frame_lengths, B, &tab, &bad))
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "frame_lengths[%d]=%d latent frames decode to no sample", bad, frame_lengths[bad]);
    hipStream_t st = (hipStream_t)stream;
    size_t mf = 0;
    const int Lout = dec_walk(d, true, B, Tmax, &mf);
    if (Lout < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d latent frames decode to no sample", Tmax);
    if ((unsigned long long)mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d frames: a feature map above 2^32 elements", B, Tmax);
    // the audio's own table: a clip's decoded samples, cut at sample_caps[b] when given (DAC.forward trims to the input length, dac.py:316)
    const int nD = d->cfg.n_decoder_rates;
    for (int b = 0; b < B; ++b) {
        int v = tab[(size_t)nD * B + b];
        if (sample_caps) {
            if (sample_caps[b] < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "sample_caps[%d]=%d below 1", b, sample_caps[b]);
            v = std::min(v, (int)sample_caps[b]);
        }
        tab.push_back(v);
    }
    if ((rc = ensure_scratch(d, 4 * mf * sizeof(float)))) return rc;
    d->len_host = tab;
    const int* lv; if ((rc = upload_counts(d, d->len_host.data(), (int)d->len_host.size(), &lv, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_w16(d, st))) return rc;
    float* x = d->scratch; float* y = x + mf; float* h = y + mf;
    const Run run{d->snake_maps, h + mf, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, true};
    const int Dp = cpad(d->latent);
    hipLaunchKernelGGL(dac_z_in_len_kernel, dim3(nblk((long long)B * Tmax * Dp)), dim3(256), 0, st, z, h, B, d->latent, Dp, Tmax, lv);
    const DacLayer* Dl = d->dec.data(); const DacSnake* SN = d->dec_sn.data();
    int T = Tmax;
    run_layer_len(run, ESCX_DAC_SNAKE_LAST, Dl[0], nullptr, h, B, T, lv, x, T, lv, nullptr, 0);
    for (int i = 0; i < nD; ++i) {
        const DacLayer* Lb = Dl + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int* tl = lv + (size_t)i * B;
        const int T2 = conv_out_len(T, Lb[0], true);
        run_layer_len(run, ESCX_DAC_SNAKE_UP, Lb[0], Sb, x, B, T, tl, y, T2, tl + B, nullptr, 0);
        std::swap(x, y); T = T2;
        for (int j = 0; j < 3; ++j) run_res_len(run, Lb + 1 + 2 * j, Sb + 1 + 2 * j, x, h, B, T, tl + B);
    }
    run_layer_len(run, ESCX_DAC_SNAKE_LAST, Dl[d->dec.size() - 1], SN + d->dec_sn.size() - 1, x, B, T, lv + (size_t)nD * B, audio, Lout, lv + (size_t)(nD + 1) * B,
                  nullptr, 1);
    return launch_ok("escx_dac_decode_lengths");
}

// ---- latent gradient through the decoder, eval mode, padding on (dac.py:249-266) -----------------------------------------
namespace {

inline int np_t(const DacLayer& l) { return rup(l.Cin, 16); }
inline int kp_t(const DacLayer& l) { return rup(l.K * cpad(l.Cout), 16); }

// The activation tape of one padded decode of B x T: a header, then the decoder's maps in execution order, then the audio.
//   map 0            the first convolution's output = block 0's ConvTranspose input
//   map 7 i + 1 + 2 j, 7 i + 2 + 2 j    ResidualUnit j of block i: its input x (j = 0: the ConvTranspose output) and its 7-tap output h
//   map 7 i + 7      block i's output = block i + 1's ConvTranspose input, or the input of the last Snake
// Every map is channels-last (B, T_i, cpad(C_i)), rounded up to 64 floats; offsets are in floats.
struct TapePlan { std::vector<size_t> off; std::vector<int> Ts; size_t audio = 0, total = 0, mf = 0; int Lout = 0; };

bool tape_plan(const escx_dac_s* d, int B, int T, TapePlan* p) {
    p->Lout = dec_walk(d, true, B, T, &p->mf);
    if (p->Lout < 1) return false;
    size_t cur = DAC_TAPE_HEADER;
    int C = d->cfg.decoder_dim, Tc = conv_out_len(T, d->dec[0], true);
    p->Ts.push_back(Tc);
    p->off.push_back(cur); cur += map_floats(B, Tc, C);
    for (int i = 0; i < d->cfg.n_decoder_rates; ++i) {
        Tc = conv_out_len(Tc, d->dec[1 + i * 7], true); C /= 2;
        p->Ts.push_back(Tc);
        for (int k = 0; k < 7; ++k) { p->off.push_back(cur); cur += map_floats(B, Tc, C); }
    }
    p->audio = cur; cur += pad64((size_t)B * p->Lout);
    p->total = cur;
    return true;
}

// The decoder's transposed weight images, after pack() on the same stream: derived from whatever fp32 image is current, once per re-pack
int refresh_wt(escx_dac_s* d, hipStream_t st) {
    if (d->wt_valid) return 0;
    if (!d->wt) {
        size_t n = 0;
        for (const DacLayer& l : d->dec) n += pad64((size_t)np_t(l) * kp_t(l));
        d->wt_floats = n;
        ESCX_HIP(hipMalloc((void**)&d->wt, n * sizeof(float)));
        ESCX_HIP(hipMemsetAsync(d->wt, 0, n * sizeof(float), st));
        size_t cur = 0;
        for (DacLayer& l : d->dec) { l.Wt = d->wt + cur; cur += pad64((size_t)np_t(l) * kp_t(l)); }
    }
    for (const DacLayer& l : d->dec)
        hipLaunchKernelGGL(dac_wt_pack_kernel, dim3(nblk((long long)l.Cin * l.K * l.Cout)), dim3(256), 0, st, (const float*)l.W, l.Wt, l.kind, l.Cin, l.Cout, l.K,
                           l.stride, l.pad, l.CinP, cpad(l.Cout), l.Np, l.Kp, kp_t(l));
    d->wt_valid = true;
    return launch_ok("dac_transpose_weights");
}

// The three-plane bf16 mirror of a transposed image (wt or wte), for the backward calls that run in bf16x3.  Called after refresh_wt / refresh_wte on
// the same stream: refresh_w16's scheme, the exact three-term split of whatever fp32 image is current, once per re-pack and once after the mode is
// first switched on.  The images' pad rows and columns are zeros and split into zeros.
int refresh_wt16(const escx_dac_s* d, const float* img, size_t floats, __bf16** img16, bool* valid, hipStream_t st) {
    if (d->grad_precision != ESCX_PRECISION_BF16X3 || *valid) return 0;
    if (!*img16) ESCX_HIP(hipMalloc((void**)img16, 3 * floats * sizeof(__bf16)));
    const size_t n4 = floats / 4;
    hipLaunchKernelGGL(split3_bf16_kernel, dim3((unsigned)std::min<size_t>((n4 + 255) / 256, 4096)), dim3(256), 0, st, img, *img16, n4, floats);
    *valid = true;
    return launch_ok("dac_split_transposed_weights");
}

// What a backward pass needs besides the layer: the stream and, in bf16x3 grad mode, the mirror of the transposed image the layers' Wt point into
// (w16 == nullptr: fp32 grad mode).  The layers that run on the bf16 matrix cores are the forward's (x3_layer).
struct GradRun {
    hipStream_t st; const float* wt; const __bf16* w16; size_t plane;
    const __bf16* mirror(const DacLayer& l, const float* W) const { return (w16 && x3_layer(l)) ? w16 + (W - wt) : nullptr; }
};

// The tile rule is launch_conv's: by the layer's tile count (fp32) or launch_dac_x3's, and no output bit depends on it.
template <class Epi>
void launch_grad(const GradRun& run, const __bf16* W16, const float* W, const DacConvA& ld, int Np, int Kp, const Epi& ep) {
    const long long tiles = (long long)((ld.M + 127) / 128) * ((Np + 95) / 96);
    if (W16) launch_dac_x3(ld, W16, run.plane, ld.M, Np, Kp, ep, run.st);
    else if (tiles >= 512) launch_gemm<128>(ld, W, ld.M, Np, Kp, ep, run.st);
    else launch_gemm<64>(ld, W, ld.M, Np, Kp, ep, run.st);
}

// dX of layer l from dY (B, Tdy, cpad(Cout)):  out (B, Tx, cpad(Cin)) = [res +] conv^T(dY) * snake'(xs), or d_z (B, zD, Tx) when there is no Snake
// in front (the first convolution).
void bwd_layer(const GradRun& run, const DacLayer& l, const DacSnake* sn, const float* dY, int B, int Tdy, int Tx, const float* xs, const float* res, float* out,
               int zD = 0) {
    DacConvA ld{};
    ld.x = dY; ld.alpha = nullptr; ld.inv = nullptr; ld.Tin = Tdy; ld.Cp = cpad(l.Cout); ld.dCp = FastDiv(ld.Cp);
    ld.Trows = Tx; ld.M = B * Tx; ld.dT = FastDiv(Tx); ld.ntaps = l.K;
    if (l.kind == 0) { ld.rs = 1; ld.r0 = l.pad; ld.td = -l.dil; }
    else { ld.rs = l.stride; ld.r0 = -l.pad; ld.td = 1; }
    DacGradEpi ep{};
    ep.out = out; ep.res = res; ep.xs = xs; ep.alpha = sn ? sn->a : nullptr; ep.inv = sn ? sn->inv : nullptr;
    ep.Cp = cpad(l.Cin); ep.D = zD; ep.T = Tx; ep.dT = ld.dT;
    launch_grad(run, run.mirror(l, l.Wt), l.Wt, ld, np_t(l), kp_t(l), ep);
}

int tape_args(escx_dac_s* d, int B, int T, long long tape_floats, TapePlan* p) {
    if (!d->padding) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "the decoder's gradient is implemented with the padding on (the chunked path needs none)");
    if (!tape_plan(d, B, T, p)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d latent frames decode to no sample", T);
    if ((unsigned long long)p->mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d frames: a feature map above 2^32 elements", B, T);
    if (tape_floats != (long long)p->total)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "tape of %lld floats: a decode of %d x %d frames needs %lld (escx_dac_decode_tape_floats)", tape_floats, B, T, (long long)p->total);
    return 0;
}

}  // namespace

extern "C" int64_t escx_dac_decode_tape_floats(escx_dac d, int B, int T) {
    if (!d || B < 1 || T < 1) return 0;
    if (!d->padding) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "the decoder's gradient is implemented with the padding on (the chunked path needs none)");
    TapePlan p;
    return tape_plan(d, B, T, &p) ? (int64_t)p.total : 0;
}

extern "C" int escx_dac_decode_tape(escx_dac d, const float* flat, int64_t version, const float* z, int B, int T, float* audio, float* tape, int64_t tape_floats,
                                    void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!z || !audio || !tape || T < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    TapePlan p;
    if ((rc = tape_args(d, B, T, (long long)tape_floats, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t mf = p.mf;
    if ((rc = ensure_scratch(d, 4 * mf * sizeof(float)))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_w16(d, st))) return rc;
    float* zin = d->scratch + 2 * mf;                       // the staged latent and the Snaked copy stay in the handle's scratch: no backward reads them
    const Run run{d->snake_maps, d->scratch + 3 * mf, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, true};
    auto M = [&](int i) { return tape + p.off[i]; };
    hipLaunchKernelGGL(dac_tape_header_kernel, dim3(1), dim3(64), 0, st, (long long*)tape, (long long)version, (long long)B, (long long)T, (long long)p.total);
    const int Dp = cpad(d->latent);
    hipLaunchKernelGGL(dac_z_in_kernel, dim3(nblk((long long)B * T * Dp)), dim3(256), 0, st, z, zin, B, d->latent, Dp, T);
    const DacLayer* Dl = d->dec.data(); const DacSnake* SN = d->dec_sn.data();
    const int nb = d->cfg.n_decoder_rates;
    run_layer(run, ESCX_DAC_SNAKE_LAST, Dl[0], nullptr, zin, B, T, M(0), p.Ts[0], nullptr, 0);
    for (int i = 0; i < nb; ++i) {
        const DacLayer* Lb = Dl + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int Tc = p.Ts[i + 1];
        run_layer(run, ESCX_DAC_SNAKE_UP, Lb[0], Sb, M(7 * i), B, p.Ts[i], M(7 * i + 1), Tc, nullptr, 0);
        for (int j = 0; j < 3; ++j) {                       // run_res with padding, x and h kept: the sum goes to the next map instead of back into x
            float* x = M(7 * i + 1 + 2 * j); float* h = M(7 * i + 2 + 2 * j);
            run_layer(run, ESCX_DAC_SNAKE_RES7, Lb[1 + 2 * j], &Sb[1 + 2 * j], x, B, Tc, h, Tc, nullptr, 0);
            run_layer(run, ESCX_DAC_SNAKE_RES1, Lb[2 + 2 * j], &Sb[2 + 2 * j], h, B, Tc, M(7 * i + 3 + 2 * j), Tc, x, 0);
        }
    }
    run_layer(run, ESCX_DAC_SNAKE_LAST, Dl[d->dec.size() - 1], SN + d->dec_sn.size() - 1, M(7 * nb), B, p.Ts[nb], audio, p.Lout, nullptr, 1);
    ESCX_HIP(hipMemcpyAsync(tape + p.audio, audio, (size_t)B * p.Lout * sizeof(float), hipMemcpyDeviceToDevice, st));
    return launch_ok("escx_dac_decode_tape");
}

extern "C" int escx_dac_decode_backward(escx_dac d, const float* flat, int64_t version, const float* tape, int64_t tape_floats, const float* d_audio, int B, int T,
                                        float* d_z, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!tape || !d_audio || !d_z || T < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    TapePlan p;
    if ((rc = tape_args(d, B, T, (long long)tape_floats, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    // The tape says what it was made with; the handle keeps nothing per graph.  Checked before anything of the handle changes.
    long long hdr[5] = {0, 0, 0, 0, 0};
    ESCX_HIP(hipMemcpyAsync(hdr, tape, sizeof(hdr), hipMemcpyDeviceToHost, st));
    ESCX_HIP(hipStreamSynchronize(st));
    if (hdr[0] != DAC_TAPE_MAGIC || hdr[2] != B || hdr[3] != T || hdr[4] != (long long)p.total)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "the buffer is not a tape that escx_dac_decode_tape made for %d x %d frames", B, T);
    if (hdr[1] != (long long)version)
        ESCX_FAIL(ESCX_ERR_STATE, "the tape was made with parameter version %lld and the backward is called with %lld: the parameters changed between forward and backward",
                  hdr[1], (long long)version);
    const size_t mf = p.mf;
    if ((rc = ensure_scratch(d, 4 * mf * sizeof(float)))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_wt(d, st)) || (rc = refresh_wt16(d, d->wt, d->wt_floats, &d->wt16, &d->wt16_valid, st))) return rc;
    const GradRun run{st, d->wt, d->grad_precision == ESCX_PRECISION_BF16X3 ? d->wt16 : nullptr, d->wt_floats};
    float* G = d->scratch; float* G2 = G + mf; float* A = G2 + mf;
    auto M = [&](int i) { return tape + p.off[i]; };
    const DacLayer* Dl = d->dec.data(); const DacSnake* SN = d->dec_sn.data();
    const int nb = d->cfg.n_decoder_rates;
    const long long n = (long long)B * p.Lout;
    hipLaunchKernelGGL(dac_tanh_grad_in_kernel, dim3(nblk(n)), dim3(256), 0, st, d_audio, tape + p.audio, A, n);
    bwd_layer(run, Dl[d->dec.size() - 1], SN + d->dec_sn.size() - 1, A, B, p.Lout, p.Ts[nb], M(7 * nb), nullptr, G);
    for (int i = nb - 1; i >= 0; --i) {
        const DacLayer* Lb = Dl + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int Tc = p.Ts[i + 1];
        for (int j = 2; j >= 0; --j) {                      // g_x = g + conv7^T(conv1^T(g) * snake'(h)) * snake'(x), in place in G
            bwd_layer(run, Lb[2 + 2 * j], &Sb[2 + 2 * j], G, B, Tc, Tc, M(7 * i + 2 + 2 * j), nullptr, A);
            bwd_layer(run, Lb[1 + 2 * j], &Sb[1 + 2 * j], A, B, Tc, Tc, M(7 * i + 1 + 2 * j), G, G);
        }
        bwd_layer(run, Lb[0], Sb, G, B, Tc, p.Ts[i], M(7 * i), nullptr, G2);
        std::swap(G, G2);
    }
    bwd_layer(run, Dl[0], nullptr, G, B, p.Ts[0], T, nullptr, nullptr, d_z, d->latent);
    return launch_ok("escx_dac_decode_backward");
}

// ---- parameter gradients through the decoder, eval mode, padding on (dac.py:24-41, 94-145, 249-266, nn/layers.py:5-33) ----
namespace {

constexpr int DW_TARGET_WGS = 2048;     // workgroups a dW contraction aims for: 8 per CU of the 256
constexpr int DW_SLICE_ROWS = 128;      // a slice is a multiple of this many rows: one 32-row chunk for each of gemm_dw_kernel's four waves
constexpr int COLSUM_BLOCKS = 1024;     // most row ranges of a bias / alpha column sum

// The staged weight gradient of a decoder layer: dW[i][tap * JP + j], i the dimension the weight norm keeps (dac_param_grad_kernels.h)
struct DwGeom { int I, J, JP, Np, Kp, blocks, smax; };
DwGeom dw_geom(const DacLayer& l) {
    DwGeom g{};
    if (l.kind == 0) { g.I = l.Cout; g.J = l.Cin; g.JP = l.CinP; g.Np = l.Np; g.Kp = l.Kp; }
    else { g.I = l.Cin; g.J = l.Cout; g.JP = cpad(l.Cout); g.Np = np_t(l); g.Kp = kp_t(l); }
    g.blocks = ((g.Np + 47) / 48) * ((g.Kp + 47) / 48);
    g.smax = std::max(1, (DW_TARGET_WGS + g.blocks - 1) / g.blocks);
    return g;
}
// The slice rule: enough slices of M rows to reach DW_TARGET_WGS workgroups, none shorter than DW_SLICE_ROWS, from the geometry alone
void dw_slices(const DwGeom& g, int M, int* slices, int* mps) {
    const int s = std::max(1, std::min(g.smax, (M + DW_SLICE_ROWS - 1) / DW_SLICE_ROWS));
    *mps = ((M + s - 1) / s + DW_SLICE_ROWS - 1) / DW_SLICE_ROWS * DW_SLICE_ROWS;
    *slices = (M + *mps - 1) / *mps;
}

// The same for the split-operand contraction (escx_dac_set_param_grad_precision): gemm_dw_bf16_kernel's 128 x 128 tiles of dW, or
// dac_dw_x3_kernel's 64 x 128 and 32 x 128 for Np <= 64 and Np <= 32 (dac_x3.h dac_dw_x3_rows).  Which layers take it is a function of the layer's
// geometry alone: every convolution with more than one input and more than one output channel (x3_layer, the forward's and the input gradients'
// rule), whatever its (Np, Kp) - a tile's rows and columns behind Np / Kp are staged as zeros and not stored.  The one-channel last convolution
// keeps the fp32 kernel and the fp32 rule.
constexpr int DW16_TILE = 128;          // columns of dW per workgroup
constexpr int DW16_STEP = 32;           // a slice is a multiple of the kernel's row step (one MFMA deep)
constexpr int DW16_MIN_ROWS = 256;      // no more slices than 256-row pieces of the contraction: a slice's 64 KB partial tile is written and read back
inline bool dw16_layer(const DacLayer& l) { return x3_layer(l); }
DwGeom dw16_geom(const DacLayer& l) {
    DwGeom g = dw_geom(l);
    const int ta = dac_dw_x3_rows(g.Np);
    g.blocks = ((g.Np + ta - 1) / ta) * ((g.Kp + DW16_TILE - 1) / DW16_TILE);
    g.smax = std::max(1, (DW_TARGET_WGS + g.blocks - 1) / g.blocks);
    return g;
}
// Its slice rule: enough slices to reach DW_TARGET_WGS workgroups, none more than M / DW16_MIN_ROWS allows, each a multiple of DW16_STEP rows
void dw16_slices(const DwGeom& g, int M, int* slices, int* mps) {
    const int s = std::max(1, std::min(g.smax, (M + DW16_MIN_ROWS - 1) / DW16_MIN_ROWS));
    *mps = ((M + s - 1) / s + DW16_STEP - 1) / DW16_STEP * DW16_STEP;
    *slices = (M + *mps - 1) / *mps;
}
// Its partial tiles, in floats, whatever the batch: smax Np Kp of the layer that needs most
size_t param_ws16_plan(const std::vector<DacLayer>& layers) {
    size_t part = 0;
    for (const DacLayer& l : layers)
        if (dw16_layer(l)) { const DwGeom g = dw16_geom(l); part = std::max(part, pad64((size_t)g.smax * g.Np * g.Kp)); }
    return part;
}
size_t param_ws16_plan(const escx_dac_s* d) { return param_ws16_plan(d->dec); }

// The workspace, in floats, whatever the batch: [partial tiles: smax Np Kp] [staged dW: Np Kp] [column partials: blocks x Cp, fp64].  pw / pw16:
// the allocations a pass works in (the decoder's, or the encoder's and the quantiser's own).
struct ParamWs {
    size_t part = 0, stage = 0, cols = 0; int cmax = 4;
    float* pw = nullptr; float* pw16 = nullptr;
    size_t total() const { return part + stage + cols; }
};
void param_ws_take(ParamWs& w, const DacLayer& l) {
    const DwGeom g = dw_geom(l);
    const size_t nk = (size_t)g.Np * g.Kp;
    w.part = std::max(w.part, pad64((size_t)g.smax * nk));
    w.stage = std::max(w.stage, pad64(nk));
    w.cmax = std::max(w.cmax, std::max(l.CinP, cpad(l.Cout)));
    w.cols = pad64(2 * (size_t)COLSUM_BLOCKS * w.cmax);
}
ParamWs param_ws_plan(const escx_dac_s* d) {
    ParamWs w;
    for (const DacLayer& l : d->dec) param_ws_take(w, l);
    return w;
}

DacConvA rows_of(const float* x, int B, int T, int Cp) {                // the rows (b, t) of a map as a one-tap operand
    DacConvA a{};
    a.x = x; a.alpha = nullptr; a.inv = nullptr; a.Tin = T; a.Cp = Cp; a.dCp = FastDiv(Cp);
    a.Trows = T; a.M = B * T; a.dT = FastDiv(T); a.rs = 1; a.r0 = 0; a.td = 0; a.ntaps = 1;
    return a;
}

// sum over the rows of v (M, Cp) [times d snake / d alpha at xs] -> out[0, C)
void colsum(const escx_dac_s* d, const ParamWs& w, hipStream_t st, const float* v, const float* xs, const DacSnake* sn, long long M, int Cp, int C, float* out) {
    double* part = reinterpret_cast<double*>(w.pw + w.part + w.stage);           // 256-byte aligned: the regions are multiples of 64 floats
    const int rows = (int)std::max<long long>(16, (M + COLSUM_BLOCKS - 1) / COLSUM_BLOCKS);
    const int blocks = (int)((M + rows - 1) / rows);
    const dim3 grid(blocks, (Cp + 255) / 256);                  // y: 256-column groups (one group when Cp <= 256)
    if (sn) hipLaunchKernelGGL(dac_colsum_kernel<true>, grid, dim3(256), 0, st, v, xs, (const float*)sn->a, (const float*)sn->inv, M, Cp, rows, part);
    else hipLaunchKernelGGL(dac_colsum_kernel<false>, grid, dim3(256), 0, st, v, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, M, Cp, rows, part);
    hipLaunchKernelGGL(dac_reduce_cols_kernel, dim3(nblk(C, 16)), dim3(256), 0, st, (const double*)part, blocks, Cp, C, out);
}

// bias, weight_g and weight_v gradients of layer l from its output gradient dY (B, Tdy, cpad(Cout)) and its forward operand s (B, Ts, CinP), both
// plain maps (the Snake already applied to s).  split_ok false: the contraction stays on the fp32 MFMA whatever the switch says (the quantiser's
// projections).
void param_layer(const escx_dac_s* d, const ParamWs& w, hipStream_t st, const DacLayer& l, const float* dY, int Tdy, const float* s, int Ts, int B,
                 const float* flat, float* grad, bool split_ok = true) {
    const DwGeom g = dw_geom(l);
    const int CoutP = cpad(l.Cout);
    DacConvA la, lb;
    if (l.kind == 0) {
        la = rows_of(dY, B, Tdy, CoutP);
        lb = rows_of(s, B, Ts, l.CinP);
        lb.Trows = Tdy; lb.M = B * Tdy; lb.dT = FastDiv(Tdy); lb.rs = l.stride; lb.r0 = -l.pad; lb.td = l.dil; lb.ntaps = l.K;
    } else {
        la = rows_of(s, B, Ts, l.CinP);
        lb = rows_of(dY, B, Tdy, CoutP);
        lb.Trows = Ts; lb.M = B * Ts; lb.dT = FastDiv(Ts); lb.rs = l.stride; lb.r0 = -l.pad; lb.td = 1; lb.ntaps = l.K;
    }
    const int M = la.M;
    int slices, mps;
    float* part = w.pw; float* stage = w.pw + w.part;
    if (split_ok && d->param_grad_precision == ESCX_PRECISION_BF16X3 && dw16_layer(l)) {
        const DwGeom g16 = dw16_geom(l);
        dw16_slices(g16, M, &slices, &mps);
        part = w.pw16;
        launch_dac_dw_x3(la, lb, M, g.Np, g.Kp, slices, mps, part, st);
    } else {
        dw_slices(g, M, &slices, &mps);
        const int nbk = (g.Kp + 47) / 48;
        hipLaunchKernelGGL((gemm_dw_kernel<DacConvA, DacConvA, false>), dim3(g.blocks, slices), dim3(256), 0, st, la, lb, M, g.Np, g.Kp, nbk, mps, part, (float*)nullptr);
    }
    const float* dW = part;                                     // one slice: its tile is the sum
    if (slices > 1) { launch_reduce_partials(part, slices, (long long)g.Np * g.Kp, stage, 0, st); dW = stage; }
    colsum(d, w, st, dY, nullptr, nullptr, (long long)B * Tdy, CoutP, l.Cout, grad + l.off_b);
    hipLaunchKernelGGL(dac_wn_bwd_kernel, dim3(g.I), dim3(256), 0, st, dW, flat + l.off_v, flat + l.off_g, grad + l.off_v, grad + l.off_g, g.J, l.K, g.JP, g.Kp);
}

// bwd_layer for a layer behind a Snake, with v = conv^T(dY) kept in vout (DacGradEpiV): `out` has bwd_layer's bits
void bwd_layer_v(const GradRun& run, const DacLayer& l, const DacSnake* sn, const float* dY, int B, int Tdy, int Tx, const float* xs, const float* res, float* out,
                 float* vout) {
    DacConvA ld{};
    ld.x = dY; ld.alpha = nullptr; ld.inv = nullptr; ld.Tin = Tdy; ld.Cp = cpad(l.Cout); ld.dCp = FastDiv(ld.Cp);
    ld.Trows = Tx; ld.M = B * Tx; ld.dT = FastDiv(Tx); ld.ntaps = l.K;
    if (l.kind == 0) { ld.rs = 1; ld.r0 = l.pad; ld.td = -l.dil; }
    else { ld.rs = l.stride; ld.r0 = -l.pad; ld.td = 1; }
    DacGradEpiV ep{};
    ep.out = out; ep.res = res; ep.xs = xs; ep.alpha = sn->a; ep.inv = sn->inv; ep.vout = vout; ep.Cp = cpad(l.Cin);
    launch_grad(run, run.mirror(l, l.Wt), l.Wt, ld, np_t(l), kp_t(l), ep);
}

// The quantiser's projections of stage i as 1 x 1 convolutions with their slots of the flat layout: in_proj (D -> d), out_proj (d -> D)
DacLayer q_layer(const escx_dac_s* d, int i, bool out_proj) {
    DacLayer l = out_proj ? make_layer(0, d->cfg.codebook_dim, d->latent, 1, 1, 0, 1) : make_layer(0, d->latent, d->cfg.codebook_dim, 1, 1, 0, 1);
    const long long* o = d->qoffs.data() + 6 * (size_t)i + (out_proj ? 3 : 0);
    l.off_b = (size_t)o[0]; l.off_g = (size_t)o[1]; l.off_v = (size_t)o[2];
    return l;
}
// The encode parameter backward's own workspace: param_ws_plan over the encoder's layers and the quantiser's two projections
ParamWs enc_param_ws_plan(const escx_dac_s* d) {
    ParamWs w;
    for (const DacLayer& l : d->enc) param_ws_take(w, l);
    param_ws_take(w, q_layer(d, 0, false));
    param_ws_take(w, q_layer(d, 0, true));
    return w;
}

}  // namespace

extern "C" int64_t escx_dac_param_grad_workspace_floats(escx_dac d) {
    if (!d) return 0;
    const bool held16 = d->param_grad_precision == ESCX_PRECISION_BF16X3 && d->pw16;
    const bool helde16 = d->param_grad_precision == ESCX_PRECISION_BF16X3 && d->pwe16;
    return (int64_t)(param_ws_plan(d).total() + (held16 ? param_ws16_plan(d) : 0) + (d->pwe ? enc_param_ws_plan(d).total() : 0) +
                     (helde16 ? param_ws16_plan(d->enc) : 0));
}

extern "C" int escx_dac_param_grad_slices(escx_dac d, int B, int T, int layer) {
    if (!d || B < 1 || T < 1 || layer < 0 || layer >= (int)d->dec.size()) return 0;
    TapePlan p;
    if (!tape_plan(d, B, T, &p)) return 0;
    // rows of the contraction: the output rows of a Conv1d, the input rows of a ConvTranspose1d
    int Trows;
    if (layer == 0) Trows = p.Ts[0];
    else if (layer == (int)d->dec.size() - 1) Trows = p.Lout;
    else { const int i = (layer - 1) / 7, k = (layer - 1) % 7; Trows = k == 0 ? p.Ts[i] : p.Ts[i + 1]; }
    int slices, mps;
    if (d->param_grad_precision == ESCX_PRECISION_BF16X3 && dw16_layer(d->dec[layer])) dw16_slices(dw16_geom(d->dec[layer]), B * Trows, &slices, &mps);
    else dw_slices(dw_geom(d->dec[layer]), B * Trows, &slices, &mps);
    return slices;
}

extern "C" int escx_dac_decode_backward_params(escx_dac d, const float* flat, int64_t version, const float* tape, int64_t tape_floats, const float* z,
                                               const float* d_audio, int B, int T, float* d_z, float* grad, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!tape || !d_audio || !z || !grad || T < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    TapePlan p;
    if ((rc = tape_args(d, B, T, (long long)tape_floats, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    long long hdr[5] = {0, 0, 0, 0, 0};                         // as escx_dac_decode_backward: checked before anything of the handle changes
    ESCX_HIP(hipMemcpyAsync(hdr, tape, sizeof(hdr), hipMemcpyDeviceToHost, st));
    ESCX_HIP(hipStreamSynchronize(st));
    if (hdr[0] != DAC_TAPE_MAGIC || hdr[2] != B || hdr[3] != T || hdr[4] != (long long)p.total)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "the buffer is not a tape that escx_dac_decode_tape made for %d x %d frames", B, T);
    if (hdr[1] != (long long)version)
        ESCX_FAIL(ESCX_ERR_STATE, "the tape was made with parameter version %lld and the backward is called with %lld: the parameters changed between forward and backward",
                  hdr[1], (long long)version);
    if ((long long)B * p.Lout > 0x7fffffffll) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d frames: more than 2^31 audio rows in one contraction", B, T);
    const size_t mf = p.mf;
    ParamWs w = param_ws_plan(d);
    if ((rc = ensure_scratch(d, 4 * mf * sizeof(float)))) return rc;
    if (!d->pw) ESCX_HIP(hipMalloc((void**)&d->pw, w.total() * sizeof(float)));
    if (d->param_grad_precision == ESCX_PRECISION_BF16X3 && !d->pw16) ESCX_HIP(hipMalloc((void**)&d->pw16, param_ws16_plan(d) * sizeof(float)));
    w.pw = d->pw; w.pw16 = d->pw16;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_wt(d, st)) || (rc = refresh_wt16(d, d->wt, d->wt_floats, &d->wt16, &d->wt16_valid, st))) return rc;
    const GradRun run{st, d->wt, d->grad_precision == ESCX_PRECISION_BF16X3 ? d->wt16 : nullptr, d->wt_floats};
    // escx_dac_decode_backward's walk and maps; S holds the Snaked operand of the layer at hand, then the v of its input gradient
    float* G = d->scratch; float* G2 = G + mf; float* A = G2 + mf; float* S = d->scratch + 3 * mf;
    auto M = [&](int i) { return tape + p.off[i]; };
    const DacLayer* Dl = d->dec.data(); const DacSnake* SN = d->dec_sn.data();
    const int nb = d->cfg.n_decoder_rates;
    // one layer behind a Snake: its parameter gradients from (dY, snake(xs)), then its input gradient with v kept, then the Snake's alpha gradient
    auto layer = [&](const DacLayer& l, const DacSnake* sn, const float* dY, int Tdy, int Tx, const float* xs, const float* res, float* out) {
        const long long n4 = (long long)B * Tx * l.CinP / 4;
        hipLaunchKernelGGL(dac_snake_map_kernel, dim3(nblk(n4)), dim3(256), 0, st, xs, (const float*)sn->a, (const float*)sn->inv, S, n4, l.CinP / 4);
        param_layer(d, w, st, l, dY, Tdy, S, Tx, B, flat, grad);
        bwd_layer_v(run, l, sn, dY, B, Tdy, Tx, xs, res, out, S);
        colsum(d, w, st, S, xs, sn, (long long)B * Tx, l.CinP, sn->C, grad + sn->off);
    };
    const long long n = (long long)B * p.Lout;
    hipLaunchKernelGGL(dac_tanh_grad_in_kernel, dim3(nblk(n)), dim3(256), 0, st, d_audio, tape + p.audio, A, n);
    layer(Dl[d->dec.size() - 1], SN + d->dec_sn.size() - 1, A, p.Lout, p.Ts[nb], M(7 * nb), nullptr, G);
    for (int i = nb - 1; i >= 0; --i) {
        const DacLayer* Lb = Dl + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int Tc = p.Ts[i + 1];
        for (int j = 2; j >= 0; --j) {
            layer(Lb[2 + 2 * j], &Sb[2 + 2 * j], G, Tc, Tc, M(7 * i + 2 + 2 * j), nullptr, A);
            layer(Lb[1 + 2 * j], &Sb[1 + 2 * j], A, Tc, Tc, M(7 * i + 1 + 2 * j), G, G);
        }
        layer(Lb[0], Sb, G, Tc, p.Ts[i], M(7 * i), nullptr, G2);
        std::swap(G, G2);
    }
    // the first convolution reads the latent itself, staged channels-last as the forward stages it
    const int Dp = cpad(d->latent);
    hipLaunchKernelGGL(dac_z_in_kernel, dim3(nblk((long long)B * T * Dp)), dim3(256), 0, st, z, A, B, d->latent, Dp, T);
    param_layer(d, w, st, Dl[0], G, p.Ts[0], A, T, B, flat, grad);
    if (d_z) bwd_layer(run, Dl[0], nullptr, G, B, p.Ts[0], T, nullptr, nullptr, d_z, d->latent);
    return launch_ok("escx_dac_decode_backward_params");
}

// ---- audio gradient through the encoder and the quantiser, eval mode, padding on (dac.py:209-247, quantize.py:58-70, 173-198) ------
namespace {

inline int kp_ph(const DacLayer& l) { return rup(2 * cpad(l.Cout), 16); }                          // one phase image of a strided Conv1d
inline bool phased(const DacLayer& l) { return l.kind == 0 && l.stride > 1; }
size_t wt_floats(const DacLayer& l) { return pad64(phased(l) ? (size_t)l.stride * np_t(l) * kp_ph(l) : (size_t)np_t(l) * kp_t(l)); }

// The activation tape of one padded encode of B x L with n quantiser stages: a header, the encoder's maps in execution order, then what the
// quantiser's backward reads.
//   map 7 i + 2 j, 7 i + 2 j + 1     ResidualUnit j of block i: its input x_j (j = 0: the block's input) and its 7-tap output h_j
//   map 7 i + 6                      the input of the Snake in front of block i's strided convolution
//   map 7 nE                         the last block's output = the input of the last Snake
//   latents (B, n d, T), codes (B, n, T) int64, counts [B] int32
// Every part is rounded up to 64 floats; offsets are in floats.
struct EncTapePlan { std::vector<size_t> off; std::vector<int> Ts; size_t latents = 0, codes = 0, counts = 0, total = 0, mf = 0; int Tz = 0, n = 0; };

bool enc_tape_plan(const escx_dac_s* d, int B, int L, int n_q, EncTapePlan* p) {
    if (L < 1 || n_q < 1) return false;
    p->Tz = enc_walk(d, true, B, L, &p->mf);
    if (p->Tz < 1) return false;
    p->n = std::min(n_q, d->cfg.n_codebooks);
    size_t cur = DAC_TAPE_HEADER;
    int C = d->cfg.encoder_dim, Tc = conv_out_len(L, d->enc[0], true);
    for (int i = 0; i < d->cfg.n_encoder_rates; ++i) {
        p->Ts.push_back(Tc);
        for (int k = 0; k < 7; ++k) { p->off.push_back(cur); cur += map_floats(B, Tc, C); }
        Tc = conv_out_len(Tc, d->enc[7 + i * 7], true); C *= 2;
    }
    p->Ts.push_back(Tc);
    p->off.push_back(cur); cur += map_floats(B, Tc, C);
    const size_t M = (size_t)B * p->Tz;
    p->latents = cur; cur += pad64((size_t)p->n * d->cfg.codebook_dim * M);
    p->codes = cur; cur += pad64(2 * (size_t)p->n * M);
    p->counts = cur; cur += pad64((size_t)B);
    p->total = cur;
    return true;
}

const char* const ENC_GRAD_PADDING = "the encoder's gradient is implemented with the padding on (the chunked path needs none)";

// bwd_strided's two taps per phase, k0 and k0 + s, are EncoderBlock's K = 2 s (dac.py:55-58): checked with the arguments, before the handle changes
int check_phased(const escx_dac_s* d) {
    for (const DacLayer& l : d->enc)
        if (phased(l) && l.K != 2 * l.stride) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "a strided convolution of %d taps at stride %d: the phase backward covers K = 2 * stride", l.K, l.stride);
    return 0;
}

int refresh_wte(escx_dac_s* d, hipStream_t st) {
    if (d->wte_valid) return 0;
    if (!d->wte) {
        size_t n = 0;
        for (const DacLayer& l : d->enc) n += wt_floats(l);
        d->wte_floats = n;
        ESCX_HIP(hipMalloc((void**)&d->wte, n * sizeof(float)));
        ESCX_HIP(hipMemsetAsync(d->wte, 0, n * sizeof(float), st));
        size_t cur = 0;
        for (DacLayer& l : d->enc) { l.Wt = d->wte + cur; cur += wt_floats(l); }
    }
    for (const DacLayer& l : d->enc) {
        if (phased(l))
            hipLaunchKernelGGL(dac_wt_phase_pack_kernel, dim3(nblk((long long)l.stride * l.Cin * 2 * l.Cout)), dim3(256), 0, st, (const float*)l.W, l.Wt, l.Cin, l.Cout,
                               l.stride, l.pad, l.CinP, cpad(l.Cout), l.Kp, np_t(l), kp_ph(l));
        else
            hipLaunchKernelGGL(dac_wt_pack_kernel, dim3(nblk((long long)l.Cin * l.K * l.Cout)), dim3(256), 0, st, (const float*)l.W, l.Wt, 0, l.Cin, l.Cout, l.K, l.stride,
                               l.pad, l.CinP, cpad(l.Cout), l.Np, l.Kp, kp_t(l));
    }
    d->wte_valid = true;
    return launch_ok("dac_transpose_encoder_weights");
}

// dX of a strided Conv1d (K = 2 stride) from dY (B, Tdy, cpad(Cout)):  out (B, Tx, cpad(Cin)) = conv^T(dY) * snake'(xs), one two-tap GEMM per input
// phase r (rows t = q s + r).  Every row of out is written by its phase.
void bwd_strided(const GradRun& run, const DacLayer& l, const DacSnake& sn, const float* dY, int B, int Tdy, int Tx, const float* xs, float* out) {
    const int s = l.stride, Np = np_t(l), Kp = kp_ph(l);
    for (int r = 0; r < s && r < Tx; ++r) {
        const int Q = (Tx - r + s - 1) / s;
        DacConvA ld{};
        ld.x = dY; ld.alpha = nullptr; ld.inv = nullptr; ld.Tin = Tdy; ld.Cp = cpad(l.Cout); ld.dCp = FastDiv(ld.Cp);
        ld.Trows = Q; ld.M = B * Q; ld.dT = FastDiv(Q); ld.ntaps = 2; ld.rs = 1; ld.r0 = (r + l.pad) / s; ld.td = -1;
        DacGradPhaseEpi ep{};
        ep.out = out; ep.xs = xs; ep.alpha = sn.a; ep.inv = sn.inv; ep.Cp = cpad(l.Cin); ep.Trows = Q; ep.Tmap = Tx; ep.os = s; ep.o0 = r; ep.dT = ld.dT;
        const float* W = l.Wt + (size_t)r * Np * Kp;
        launch_grad(run, run.mirror(l, W), W, ld, Np, Kp, ep);
    }
}

void launch_rvq_grad(int latent, long long M, const DacQGradArgs& qa, hipStream_t st) {
    const int J = (latent + 63) / 64;
    const dim3 g(nblk(M, 4)), blk(256);
    if (J <= 1) hipLaunchKernelGGL((dac_rvq_grad_kernel<1>), g, blk, 0, st, qa);
    else if (J <= 2) hipLaunchKernelGGL((dac_rvq_grad_kernel<2>), g, blk, 0, st, qa);
    else if (J <= 4) hipLaunchKernelGGL((dac_rvq_grad_kernel<4>), g, blk, 0, st, qa);
    else if (J <= 8) hipLaunchKernelGGL((dac_rvq_grad_kernel<8>), g, blk, 0, st, qa);
    else hipLaunchKernelGGL((dac_rvq_grad_kernel<16>), g, blk, 0, st, qa);
}

}  // namespace

extern "C" int64_t escx_dac_encode_tape_floats(escx_dac d, int B, int L, int n_q) {
    if (!d || B < 1 || L < 1 || n_q < 1) return 0;
    if (!d->padding) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "%s", ENC_GRAD_PADDING);
    EncTapePlan p;
    return enc_tape_plan(d, B, L, n_q, &p) ? (int64_t)p.total : 0;
}

extern "C" int escx_dac_encode_tape(escx_dac d, const float* flat, int64_t version, const float* audio, int B, int L, int n_q, const int32_t* clip_n, float* z,
                                    int64_t* codes, float* latents, float* losses, float* tape, int64_t tape_floats, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!audio || !z || !codes || !latents || !losses || !tape || n_q < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (!d->padding) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "%s", ENC_GRAD_PADDING);
    if (clip_n && n_q > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d code slots above the %d codebooks", n_q, d->cfg.n_codebooks);
    EncTapePlan p;
    if (!enc_tape_plan(d, B, L, n_q, &p)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d samples give no latent frame (the hop is %d)", L, d->hop);
    const int n = p.n;
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    if ((unsigned long long)p.mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d samples: a feature map above 2^32 elements", B, L);
    if (tape_floats != (long long)p.total)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "tape of %lld floats: an encode of %d x %d samples with %d codebooks needs %lld (escx_dac_encode_tape_floats)",
                  (long long)tape_floats, B, L, n, (long long)p.total);
    hipStream_t st = (hipStream_t)stream;
    const size_t mf = p.mf, M = (size_t)B * p.Tz;
    const size_t lossf = pad64((size_t)n * M) + pad64((size_t)n * B);
    if ((rc = ensure_scratch(d, (4 * mf + lossf) * sizeof(float)))) return rc;
    const int* cdev; if ((rc = upload_counts(d, clip_n, B, &cdev, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_w16(d, st))) return rc;
    // the staged input, the encoder's output map and the Snaked copies stay in the handle's scratch: no backward reads them
    float* zmap = d->scratch + mf; float* in = d->scratch + 2 * mf; float* lossb = d->scratch + 4 * mf;
    const Run run{d->snake_maps, d->scratch + 3 * mf, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, true};
    auto Mp = [&](int i) { return tape + p.off[i]; };
    hipLaunchKernelGGL(dac_enc_tape_header_kernel, dim3(nblk(B)), dim3(256), 0, st, (long long*)tape, (long long)version, (long long)B, (long long)L, (long long)p.total,
                       (long long)n, cdev, (int*)(tape + p.counts));
    hipLaunchKernelGGL(dac_wave_in_kernel, dim3(nblk((long long)B * L)), dim3(256), 0, st, audio, in, (long long)B * L);
    const DacLayer* E = d->enc.data(); const DacSnake* SN = d->enc_sn.data();
    const int nE = d->cfg.n_encoder_rates;
    run_layer(run, ESCX_DAC_SNAKE_LAST, E[0], nullptr, in, B, L, Mp(0), p.Ts[0], nullptr, 0);
    for (int i = 0; i < nE; ++i) {
        const DacLayer* Lb = E + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int Tc = p.Ts[i];
        for (int j = 0; j < 3; ++j) {                       // run_res with padding, x and h kept: the sum goes to the next map instead of back into x
            float* x = Mp(7 * i + 2 * j); float* h = Mp(7 * i + 2 * j + 1);
            run_layer(run, ESCX_DAC_SNAKE_RES7, Lb[2 * j], &Sb[2 * j], x, B, Tc, h, Tc, nullptr, 0);
            run_layer(run, ESCX_DAC_SNAKE_RES1, Lb[2 * j + 1], &Sb[2 * j + 1], h, B, Tc, Mp(7 * i + 2 * j + 2), Tc, x, 0);
        }
        run_layer(run, ESCX_DAC_SNAKE_DOWN, Lb[6], Sb + 6, Mp(7 * i + 6), B, Tc, Mp(7 * i + 7), p.Ts[i + 1], nullptr, 0);
    }
    run_layer(run, ESCX_DAC_SNAKE_LAST, E[d->enc.size() - 1], SN + d->enc_sn.size() - 1, Mp(7 * nE), B, p.Ts[nE], zmap, p.Tz, nullptr, 0);
    DacQArgs qa{};
    qa.t = d->qt; qa.zmap = zmap; qa.z = z; qa.codes = (long long*)codes; qa.latents = latents; qa.loss = lossb;
    qa.M = (int)M; qa.T = p.Tz; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n;
    if (clip_n) { qa.clip_n = cdev; launch_rvq<false, DAC_Q_CLIPS>(d->latent, (long long)M, qa, st); }
    else launch_rvq<false, DAC_Q_PLAIN>(d->latent, (long long)M, qa, st);
    hipLaunchKernelGGL(dac_loss_kernel, dim3(1), dim3(256), 0, st, lossb, lossb + pad64((size_t)n * M), losses, B, p.Tz, n, d->cfg.codebook_dim);
    ESCX_HIP(hipMemcpyAsync(tape + p.latents, latents, (size_t)n * d->cfg.codebook_dim * M * sizeof(float), hipMemcpyDeviceToDevice, st));
    ESCX_HIP(hipMemcpyAsync(tape + p.codes, codes, (size_t)n * M * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    return launch_ok("escx_dac_encode_tape");
}

extern "C" int escx_dac_encode_backward(escx_dac d, const float* flat, int64_t version, const float* tape, int64_t tape_floats, const float* d_z,
                                        const float* d_latents, const float* d_commitment, int B, int L, float* d_audio, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!tape || !d_audio || L < 1 || tape_floats < DAC_TAPE_HEADER) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (!d->padding) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "%s", ENC_GRAD_PADDING);
    if ((rc = check_phased(d))) return rc;
    hipStream_t st = (hipStream_t)stream;
    // The tape says what it was made with, the stage count included; the handle keeps nothing per graph.  Checked before anything of the handle changes.
    long long hdr[6] = {0, 0, 0, 0, 0, 0};
    ESCX_HIP(hipMemcpyAsync(hdr, tape, sizeof(hdr), hipMemcpyDeviceToHost, st));
    ESCX_HIP(hipStreamSynchronize(st));
    EncTapePlan p;
    if (hdr[0] != DAC_ENC_TAPE_MAGIC || hdr[2] != B || hdr[3] != L || hdr[4] != (long long)tape_floats || hdr[5] < 1 || hdr[5] > d->cfg.n_codebooks ||
        !enc_tape_plan(d, B, L, (int)hdr[5], &p) || (long long)p.total != (long long)tape_floats)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "the buffer of %lld floats is not a tape that escx_dac_encode_tape made for %d x %d samples", (long long)tape_floats, B, L);
    if ((unsigned long long)p.mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d samples: a feature map above 2^32 elements", B, L);
    if (hdr[1] != (long long)version)
        ESCX_FAIL(ESCX_ERR_STATE, "the tape was made with parameter version %lld and the backward is called with %lld: the parameters changed between forward and backward",
                  hdr[1], (long long)version);
    const size_t mf = p.mf;
    if ((rc = ensure_scratch(d, 4 * mf * sizeof(float)))) return rc;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_wte(d, st)) || (rc = refresh_wt16(d, d->wte, d->wte_floats, &d->wte16, &d->wte16_valid, st))) return rc;
    const GradRun run{st, d->wte, d->grad_precision == ESCX_PRECISION_BF16X3 ? d->wte16 : nullptr, d->wte_floats};
    float* G = d->scratch; float* G2 = G + mf; float* A = G2 + mf;
    auto Mp = [&](int i) { return tape + p.off[i]; };
    const DacLayer* E = d->enc.data(); const DacSnake* SN = d->enc_sn.data();
    const int nE = d->cfg.n_encoder_rates;
    DacQGradArgs qa{};
    qa.win = d->qt.win; qa.wout = d->qt.wout; qa.cbraw = d->qt.cbraw; qa.g_z = d_z; qa.g_lat = d_latents; qa.g_cm = d_commitment;
    qa.latents = tape + p.latents; qa.codes = (const long long*)(tape + p.codes); qa.clip_n = (const int*)(tape + p.counts); qa.out = A;
    qa.M = B * p.Tz; qa.T = p.Tz; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = p.n; qa.B = B;
    launch_rvq_grad(d->latent, (long long)B * p.Tz, qa, st);
    bwd_layer(run, E[d->enc.size() - 1], SN + d->enc_sn.size() - 1, A, B, p.Tz, p.Ts[nE], Mp(7 * nE), nullptr, G);
    for (int i = nE - 1; i >= 0; --i) {
        const DacLayer* Lb = E + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int Tc = p.Ts[i];
        if (phased(Lb[6])) bwd_strided(run, Lb[6], Sb[6], G, B, p.Ts[i + 1], Tc, Mp(7 * i + 6), G2);
        else bwd_layer(run, Lb[6], &Sb[6], G, B, p.Ts[i + 1], Tc, Mp(7 * i + 6), nullptr, G2);          // a rate of 1: a plain two-tap convolution
        std::swap(G, G2);
        for (int j = 2; j >= 0; --j) {                      // g_x = g + conv7^T(conv1^T(g) * snake'(h)) * snake'(x), in place in G
            bwd_layer(run, Lb[2 * j + 1], &Sb[2 * j + 1], G, B, Tc, Tc, Mp(7 * i + 2 * j + 1), nullptr, A);
            bwd_layer(run, Lb[2 * j], &Sb[2 * j], A, B, Tc, Tc, Mp(7 * i + 2 * j), G, G);
        }
    }
    bwd_layer(run, E[0], nullptr, G, B, p.Ts[0], L, nullptr, nullptr, d_audio, 1);
    return launch_ok("escx_dac_encode_backward");
}

// ---- parameter gradients through the encoder and the quantiser, eval mode, padding on (dac.py:24-91, quantize.py:58-70, 173-198,
// nn/layers.py:5-33) ------------------------------------------------------------------------------------------------------
namespace {

// bwd_strided with v = conv^T(dY) kept in vout (DacGradPhaseEpiV): `out` has bwd_strided's bits
void bwd_strided_v(const GradRun& run, const DacLayer& l, const DacSnake& sn, const float* dY, int B, int Tdy, int Tx, const float* xs, float* out, float* vout) {
    const int s = l.stride, Np = np_t(l), Kp = kp_ph(l);
    for (int r = 0; r < s && r < Tx; ++r) {
        const int Q = (Tx - r + s - 1) / s;
        DacConvA ld{};
        ld.x = dY; ld.alpha = nullptr; ld.inv = nullptr; ld.Tin = Tdy; ld.Cp = cpad(l.Cout); ld.dCp = FastDiv(ld.Cp);
        ld.Trows = Q; ld.M = B * Q; ld.dT = FastDiv(Q); ld.ntaps = 2; ld.rs = 1; ld.r0 = (r + l.pad) / s; ld.td = -1;
        DacGradPhaseEpiV ep{};
        ep.out = out; ep.xs = xs; ep.alpha = sn.a; ep.inv = sn.inv; ep.vout = vout; ep.Cp = cpad(l.Cin); ep.Trows = Q; ep.Tmap = Tx; ep.os = s; ep.o0 = r;
        ep.dT = ld.dT;
        const float* W = l.Wt + (size_t)r * Np * Kp;
        launch_grad(run, run.mirror(l, W), W, ld, Np, Kp, ep);
    }
}

void launch_rvq_param_rows(int latent, long long M, const DacQParamArgs& qa, hipStream_t st) {
    const int J = (latent + 63) / 64;
    const dim3 g(nblk(M, 4)), blk(256);
    if (J <= 1) hipLaunchKernelGGL((dac_rvq_param_rows_kernel<1>), g, blk, 0, st, qa);
    else if (J <= 2) hipLaunchKernelGGL((dac_rvq_param_rows_kernel<2>), g, blk, 0, st, qa);
    else if (J <= 4) hipLaunchKernelGGL((dac_rvq_param_rows_kernel<4>), g, blk, 0, st, qa);
    else if (J <= 8) hipLaunchKernelGGL((dac_rvq_param_rows_kernel<8>), g, blk, 0, st, qa);
    else hipLaunchKernelGGL((dac_rvq_param_rows_kernel<16>), g, blk, 0, st, qa);
}

// Output rows per clip of encoder layer `layer` (every one a Conv1d: the rows of its dW contraction)
int enc_layer_rows(const escx_dac_s* d, const EncTapePlan& p, int layer) {
    if (layer == 0) return p.Ts[0];
    if (layer == (int)d->enc.size() - 1) return p.Tz;
    const int i = (layer - 1) / 7, k = (layer - 1) % 7;
    return k == 6 ? p.Ts[i + 1] : p.Ts[i];
}

// The quantiser's parameter backward for B x T latent rows and n stages (quantize.py:58-70, 173-198 differentiated; escx.h has the formulas), shared
// by escx_dac_encode_backward_params and escx_dac_quantize_backward_params: per stage in reverse the row launch, then the two projections'
// contractions, column sums and weight-norm backward; then the codebooks; then zeros for the stages no clip ran.  zmap is the quantiser's input
// channels-last - the encoder's last convolution run again, or the staged z of the stand-alone call; gr, U, R are (M, Dp) maps and E, Q (M, dp)
// maps the launches work in.  lat / codes / counts are the forward's latents, codes and per-clip stage counts on the device.
struct QParamMaps { const float* zmap; float* gr; float* U; float* R; float* E; float* Q; };
int quantizer_param_grads(escx_dac_s* d, const ParamWs& w, hipStream_t st, const QParamMaps& m, const float* lat, const long long* codes, const int* counts,
                          const float* d_z, const float* d_latents, const float* d_commitment, const float* d_codebook, int B, int T, int n, const float* flat,
                          float* grad) {
    const int D = d->latent, Dp = cpad(D), dd = d->cfg.codebook_dim, dp = cpad(dd), S = d->cfg.n_codebooks, K = d->cfg.codebook_size;
    const size_t M = (size_t)B * T;
    ESCX_HIP(hipMemsetAsync(m.gr, 0, M * Dp * sizeof(float), st));
    DacQParamArgs qp{};
    qp.win = d->qt.win; qp.wout = d->qt.wout; qp.bout = d->qt.bout; qp.cbraw = d->qt.cbraw; qp.g_z = d_z; qp.g_lat = d_latents; qp.g_cm = d_commitment;
    qp.latents = lat; qp.codes = codes; qp.clip_n = counts; qp.zmap = m.zmap; qp.gr = m.gr; qp.U = m.U; qp.R = m.R; qp.E = m.E; qp.Q = m.Q;
    qp.M = (int)M; qp.T = T; qp.D = D; qp.Dp = Dp; qp.d = dd; qp.dp = dp; qp.K = K; qp.n = n; qp.B = B;
    for (int i = n - 1; i >= 0; --i) {
        qp.stage = i;
        launch_rvq_param_rows(D, (long long)M, qp, st);
        param_layer(d, w, st, q_layer(d, i, true), m.U, T, m.Q, T, B, flat, grad, false);
        param_layer(d, w, st, q_layer(d, i, false), m.E, T, m.R, T, B, flat, grad, false);
    }
    hipLaunchKernelGGL(dac_codebook_grad_kernel, dim3(nblk((long long)n * K, 4)), dim3(256), 0, st, (const float*)d->qt.cbraw, lat, codes, counts, d_codebook,
                       (const long long*)(d->qoffs_dev + 6 * (size_t)S), (int)M, T, dd, K, n, B, grad);
    if (n < S) {                                                // the stages no clip ran: a stage's seven tensors are consecutive, and so are the stages
        const size_t lo = (size_t)d->qoffs[6 * (size_t)n], hi = (size_t)d->qoffs[6 * (size_t)S + S - 1] + (size_t)K * dd;
        ESCX_HIP(hipMemsetAsync(grad + lo, 0, (hi - lo) * sizeof(float), st));
    }
    return 0;
}

}  // namespace

extern "C" int escx_dac_encode_param_grad_slices(escx_dac d, int B, int L, int layer) {
    if (!d || B < 1 || L < 1 || layer < 0 || layer >= (int)d->enc.size() || !d->padding) return 0;
    EncTapePlan p;
    if (!enc_tape_plan(d, B, L, 1, &p)) return 0;
    const DacLayer& l = d->enc[layer];
    int slices, mps;
    if (d->param_grad_precision == ESCX_PRECISION_BF16X3 && dw16_layer(l)) dw16_slices(dw16_geom(l), B * enc_layer_rows(d, p, layer), &slices, &mps);
    else dw_slices(dw_geom(l), B * enc_layer_rows(d, p, layer), &slices, &mps);
    return slices;
}

extern "C" int escx_dac_encode_backward_params(escx_dac d, const float* flat, int64_t version, const float* tape, int64_t tape_floats, const float* audio,
                                               const float* d_z, const float* d_latents, const float* d_commitment, const float* d_codebook, int B, int L,
                                               int parts, float* d_audio, float* grad, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!tape || !audio || !grad || L < 1 || tape_floats < DAC_TAPE_HEADER) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (parts < 1 || parts > 3) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "parts %d: expected 1 (encoder), 2 (quantiser) or 3 (both)", parts);
    if (!d->padding) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "%s", ENC_GRAD_PADDING);
    if ((rc = check_phased(d))) return rc;
    hipStream_t st = (hipStream_t)stream;
    long long hdr[6] = {0, 0, 0, 0, 0, 0};                      // as escx_dac_encode_backward: checked before anything of the handle changes
    ESCX_HIP(hipMemcpyAsync(hdr, tape, sizeof(hdr), hipMemcpyDeviceToHost, st));
    ESCX_HIP(hipStreamSynchronize(st));
    EncTapePlan p;
    if (hdr[0] != DAC_ENC_TAPE_MAGIC || hdr[2] != B || hdr[3] != L || hdr[4] != (long long)tape_floats || hdr[5] < 1 || hdr[5] > d->cfg.n_codebooks ||
        !enc_tape_plan(d, B, L, (int)hdr[5], &p) || (long long)p.total != (long long)tape_floats)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "the buffer of %lld floats is not a tape that escx_dac_encode_tape made for %d x %d samples", (long long)tape_floats, B, L);
    if ((unsigned long long)p.mf >= (1ull << 32)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d samples: a feature map above 2^32 elements", B, L);
    if (hdr[1] != (long long)version)
        ESCX_FAIL(ESCX_ERR_STATE, "the tape was made with parameter version %lld and the backward is called with %lld: the parameters changed between forward and backward",
                  hdr[1], (long long)version);
    if ((long long)B * L > 0x7fffffffll) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d samples: more than 2^31 audio rows in one contraction", B, L);
    const bool enc = parts & 1, qnt = parts & 2;
    const bool walk = enc || d_audio;                           // the encoder's layers are walked for their parameters or for the audio gradient
    const size_t mf = p.mf, M = (size_t)B * p.Tz;
    const int D = d->latent, Dp = cpad(D), dd = d->cfg.codebook_dim, dp = cpad(dd), K = d->cfg.codebook_size, n = p.n;
    const size_t qrow = pad64(M * dp);
    ParamWs w = enc_param_ws_plan(d);
    if ((rc = ensure_scratch(d, (5 * mf + 2 * qrow) * sizeof(float)))) return rc;
    if (!d->pwe) ESCX_HIP(hipMalloc((void**)&d->pwe, w.total() * sizeof(float)));
    if (d->param_grad_precision == ESCX_PRECISION_BF16X3 && !d->pwe16) ESCX_HIP(hipMalloc((void**)&d->pwe16, std::max<size_t>(64, param_ws16_plan(d->enc)) * sizeof(float)));
    w.pw = d->pwe; w.pw16 = d->pwe16;
    if ((rc = pack(d, flat, (long long)version, st)) || (rc = refresh_wte(d, st)) || (rc = refresh_wt16(d, d->wte, d->wte_floats, &d->wte16, &d->wte16_valid, st))) return rc;
    if (qnt && (rc = refresh_w16(d, st))) return rc;
    const GradRun run{st, d->wte, d->grad_precision == ESCX_PRECISION_BF16X3 ? d->wte16 : nullptr, d->wte_floats};
    // escx_dac_encode_backward's maps; Sm holds the Snaked operand of the layer at hand, then the v of its input gradient
    float* G = d->scratch; float* G2 = G + mf; float* A = G2 + mf; float* Sm = d->scratch + 3 * mf;
    auto Mp = [&](int i) { return tape + p.off[i]; };
    const DacLayer* E = d->enc.data(); const DacSnake* SN = d->enc_sn.data();
    const int nE = d->cfg.n_encoder_rates;
    const float* lat = tape + p.latents; const long long* codes = (const long long*)(tape + p.codes); const int* counts = (const int*)(tape + p.counts);
    if (walk) {                                                 // d_z_enc, the dY of the encoder's last convolution: escx_dac_encode_backward's launch
        DacQGradArgs qa{};
        qa.win = d->qt.win; qa.wout = d->qt.wout; qa.cbraw = d->qt.cbraw; qa.g_z = d_z; qa.g_lat = d_latents; qa.g_cm = d_commitment;
        qa.latents = lat; qa.codes = codes; qa.clip_n = counts; qa.out = A;
        qa.M = (int)M; qa.T = p.Tz; qa.D = D; qa.Dp = Dp; qa.d = dd; qa.K = K; qa.n = n; qa.B = B;
        launch_rvq_grad(D, (long long)M, qa, st);
    }
    if (qnt) {
        // z_enc: the encoder's last convolution again from the last taped map, the forward's launch (the tape does not hold the quantiser's input)
        float* zmap = d->scratch + 4 * mf; float* Em = d->scratch + 5 * mf;
        const Run frun{d->snake_maps, Sm, st, d->wbuf, d->precision == ESCX_PRECISION_BF16X3 ? d->w16 : nullptr, d->conv_floats, true};
        run_layer(frun, ESCX_DAC_SNAKE_LAST, E[d->enc.size() - 1], SN + d->enc_sn.size() - 1, Mp(7 * nE), B, p.Ts[nE], zmap, p.Tz, nullptr, 0);
        const QParamMaps qm{zmap, G, G2, Sm, Em, Em + qrow};
        if ((rc = quantizer_param_grads(d, w, st, qm, lat, codes, counts, d_z, d_latents, d_commitment, d_codebook, B, p.Tz, n, flat, grad))) return rc;
    }
    if (!walk) return launch_ok("escx_dac_encode_backward_params");
    // one layer behind a Snake.  With the encoder chosen: its parameter gradients from (dY, snake(xs)), its input gradient with v kept, the Snake's
    // alpha gradient; otherwise escx_dac_encode_backward's launch.  `out` has the same bits either way.
    auto layer = [&](const DacLayer& l, const DacSnake* sn, const float* dY, int Tdy, int Tx, const float* xs, const float* res, float* out) {
        if (!enc) {
            if (phased(l)) bwd_strided(run, l, *sn, dY, B, Tdy, Tx, xs, out);
            else bwd_layer(run, l, sn, dY, B, Tdy, Tx, xs, res, out);
            return;
        }
        const long long n4 = (long long)B * Tx * l.CinP / 4;
        hipLaunchKernelGGL(dac_snake_map_kernel, dim3(nblk(n4)), dim3(256), 0, st, xs, (const float*)sn->a, (const float*)sn->inv, Sm, n4, l.CinP / 4);
        param_layer(d, w, st, l, dY, Tdy, Sm, Tx, B, flat, grad);
        if (phased(l)) bwd_strided_v(run, l, *sn, dY, B, Tdy, Tx, xs, out, Sm);
        else bwd_layer_v(run, l, sn, dY, B, Tdy, Tx, xs, res, out, Sm);
        colsum(d, w, st, Sm, xs, sn, (long long)B * Tx, l.CinP, sn->C, grad + sn->off);
    };
    layer(E[d->enc.size() - 1], SN + d->enc_sn.size() - 1, A, p.Tz, p.Ts[nE], Mp(7 * nE), nullptr, G);
    for (int i = nE - 1; i >= 0; --i) {
        const DacLayer* Lb = E + 1 + i * 7; const DacSnake* Sb = SN + i * 7;
        const int Tc = p.Ts[i];
        layer(Lb[6], &Sb[6], G, p.Ts[i + 1], Tc, Mp(7 * i + 6), nullptr, G2);
        std::swap(G, G2);
        for (int j = 2; j >= 0; --j) {
            layer(Lb[2 * j + 1], &Sb[2 * j + 1], G, Tc, Tc, Mp(7 * i + 2 * j + 1), nullptr, A);
            layer(Lb[2 * j], &Sb[2 * j], A, Tc, Tc, Mp(7 * i + 2 * j), G, G);
        }
    }
    if (enc) {                                                  // the first convolution reads the audio itself, staged as the forward stages it; no Snake in front
        hipLaunchKernelGGL(dac_wave_in_kernel, dim3(nblk((long long)B * L)), dim3(256), 0, st, audio, A, (long long)B * L);
        param_layer(d, w, st, E[0], G, p.Ts[0], A, L, B, flat, grad);
    }
    if (d_audio) bwd_layer(run, E[0], nullptr, G, B, p.Ts[0], L, nullptr, nullptr, d_audio, 1);
    return launch_ok("escx_dac_encode_backward_params");
}

// ---- the stand-alone quantiser: ResidualVectorQuantize.forward on a latent z (nn/quantize.py:127-198) with its gradients (quantize.py:58-70 under
// autograd), and ResidualVectorQuantize.from_latents (quantize.py:222-255 over decode_latents, quantize.py:78-94); DESIGN.md section 13.8 ----------
namespace {

// per-clip frame counts of a quantiser call: each in [1, T].  The quantiser has no convolution, so the padding mode plays no part.
int check_frame_lengths(const int32_t* fl, int B, int T) {
    for (int b = 0; b < B; ++b)
        if (fl[b] < 1 || fl[b] > T) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "frame_lengths[%d]=%d outside [1, %d]", b, fl[b], T);
    return 0;
}

// the rows of a quantiser call as the kernels index them: an int row number, a (B, T, Dp) map below 2^31 elements
int check_rows(const escx_dac_s* d, int B, int T) {
    if ((unsigned long long)B * T * cpad(d->latent) >= (1ull << 31)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "batch of %d x %d frames: a latent map above 2^31 elements", B, T);
    return 0;
}

// [frame_lengths][clip_n], each optional, in one upload (upload_counts); *fl / *cn point into the device copy or stay nullptr
int upload_tables(escx_dac_s* d, const int32_t* frame_lengths, const int32_t* clip_n, int B, const int** fl, const int** cn, hipStream_t st) {
    *fl = *cn = nullptr;
    if (!frame_lengths && !clip_n) return 0;
    std::vector<int32_t>& host = d->len_host;
    host.clear();
    if (frame_lengths) host.insert(host.end(), frame_lengths, frame_lengths + B);
    if (clip_n) host.insert(host.end(), clip_n, clip_n + B);
    const int* dev; int rc = upload_counts(d, host.data(), (int)host.size(), &dev, st); if (rc) return rc;
    if (frame_lengths) { *fl = dev; dev += B; }
    if (clip_n) *cn = dev;
    return 0;
}

// escx_dac_quantize / _ex / _lengths: the staged z, then the quantiser and loss launches of escx_dac_encode_ex / escx_dac_encode_lengths on it
int quantize_impl(escx_dac d, const float* flat, int64_t version, const float* z, int B, int T, int n_q, const int32_t* frame_lengths, const int32_t* clip_n,
                  float* zq, int64_t* codes, float* latents, float* losses, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!z || !zq || !codes || !latents || !losses || T < 1 || n_q < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (frame_lengths && (rc = check_frame_lengths(frame_lengths, B, T))) return rc;
    if (clip_n && n_q > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d code slots above the %d codebooks", n_q, d->cfg.n_codebooks);
    const int n = std::min(n_q, d->cfg.n_codebooks);
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    if ((rc = check_rows(d, B, T))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int D = d->latent, Dp = cpad(D);
    const size_t M = (size_t)B * T, zf = pad64(M * Dp);
    if ((rc = ensure_scratch(d, (zf + pad64((size_t)n * M) + pad64((size_t)n * B)) * sizeof(float)))) return rc;
    const int* fl; const int* cn; if ((rc = upload_tables(d, frame_lengths, clip_n, B, &fl, &cn, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st))) return rc;
    float* zmap = d->scratch; float* lossb = zmap + zf;
    if (fl) hipLaunchKernelGGL(dac_z_in_len_kernel, dim3(nblk((long long)M * Dp)), dim3(256), 0, st, z, zmap, B, D, Dp, T, fl);
    else hipLaunchKernelGGL(dac_z_in_kernel, dim3(nblk((long long)M * Dp)), dim3(256), 0, st, z, zmap, B, D, Dp, T);
    DacQArgs qa{};
    qa.t = d->qt; qa.zmap = zmap; qa.z = zq; qa.codes = (long long*)codes; qa.latents = latents; qa.loss = lossb;
    qa.M = (int)M; qa.T = T; qa.D = D; qa.Dp = Dp; qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n;
    qa.clip_n = cn; qa.frame_len = fl;
    if (fl && cn) launch_rvq<false, DAC_Q_LEN | DAC_Q_CLIPS>(D, (long long)M, qa, st);
    else if (fl) launch_rvq<false, DAC_Q_LEN | DAC_Q_PLAIN>(D, (long long)M, qa, st);
    else if (cn) launch_rvq<false, DAC_Q_CLIPS>(D, (long long)M, qa, st);
    else launch_rvq<false, DAC_Q_PLAIN>(D, (long long)M, qa, st);
    if (fl) hipLaunchKernelGGL(dac_loss_len_kernel, dim3(1), dim3(256), 0, st, lossb, lossb + pad64((size_t)n * M), losses, B, T, n, d->cfg.codebook_dim, fl);
    else hipLaunchKernelGGL(dac_loss_kernel, dim3(1), dim3(256), 0, st, lossb, lossb + pad64((size_t)n * M), losses, B, T, n, d->cfg.codebook_dim);
    return launch_ok("escx_dac_quantize");
}

// what both backwards check of the forward's shapes; the per-clip stage counts go to the device as [B] ints (clip_n == NULL: n everywhere)
int quantize_backward_args(escx_dac d, const float* flat, const float* latents, const int64_t* codes, int B, int T, int n, const int32_t* clip_n) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!latents || !codes || T < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (n < 1 || n > d->cfg.n_codebooks) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%d code slots outside [1, %d]", n, d->cfg.n_codebooks);
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    return check_rows(d, B, T);
}
int upload_stage_counts(escx_dac_s* d, const int32_t* clip_n, int B, int n, const int** dev, hipStream_t st) {
    std::vector<int32_t>& host = d->len_host;
    if (clip_n) host.assign(clip_n, clip_n + B); else host.assign((size_t)B, n);
    return upload_counts(d, host.data(), B, dev, st);
}

void launch_rvq_grad_out(escx_dac_s* d, const float* latents, const int64_t* codes, const int* counts, const float* d_zq, const float* d_latents,
                         const float* d_commitment, int B, int T, int n, float* A, float* d_z, hipStream_t st) {
    const int D = d->latent, Dp = cpad(D);
    DacQGradArgs qa{};
    qa.win = d->qt.win; qa.wout = d->qt.wout; qa.cbraw = d->qt.cbraw; qa.g_z = d_zq; qa.g_lat = d_latents; qa.g_cm = d_commitment;
    qa.latents = latents; qa.codes = (const long long*)codes; qa.clip_n = counts; qa.out = A;
    qa.M = B * T; qa.T = T; qa.D = D; qa.Dp = Dp; qa.d = d->cfg.codebook_dim; qa.K = d->cfg.codebook_size; qa.n = n; qa.B = B;
    launch_rvq_grad(D, (long long)B * T, qa, st);
    hipLaunchKernelGGL(dac_z_out_kernel, dim3(nblk((long long)B * D * T)), dim3(256), 0, st, (const float*)A, d_z, B, D, Dp, T);
}

// escx_dac_from_latents / _ex / _lengths: the independent search, then from_codes' launch on its codes
int from_latents_impl(escx_dac d, const float* flat, int64_t version, const float* latents, int B, int C, int T, const int32_t* frame_lengths, const int32_t* clip_n,
                      float* z, float* zp, int64_t* codes, void* stream) {
    int rc = check_args(d, flat, B); if (rc) return rc;
    if (!latents || !z || !zp || !codes || T < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    const int dd = d->cfg.codebook_dim;
    if (C < dd) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "latents of %d channels hold no codebook of %d dimensions", C, dd);
    const int n = std::min(C / dd, d->cfg.n_codebooks);
    if (frame_lengths && (rc = check_frame_lengths(frame_lengths, B, T))) return rc;
    if (clip_n && (rc = check_clip_counts(d, clip_n, B, n))) return rc;
    if ((rc = check_rows(d, B, T))) return rc;
    if ((unsigned long long)B * C * T >= (1ull << 31)) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "latents of %d x %d x %d: above 2^31 elements", B, C, T);
    hipStream_t st = (hipStream_t)stream;
    const int* fl; const int* cn; if ((rc = upload_tables(d, frame_lengths, clip_n, B, &fl, &cn, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st))) return rc;
    const long long M = (long long)B * T;
    DacSearchArgs sa{};
    sa.cbn = d->qt.cbn; sa.c2 = d->qt.c2; sa.latents = latents; sa.codes = (long long*)codes; sa.clip_n = cn; sa.frame_len = fl;
    sa.M = (int)M; sa.T = T; sa.C = C; sa.d = dd; sa.K = d->cfg.codebook_size; sa.n = n;
    hipLaunchKernelGGL(dac_latent_search_kernel, dim3(nblk(M * n, 4)), dim3(256), 0, st, sa);
    DacQArgs qa{};
    qa.t = d->qt; qa.codes_in = (const long long*)codes; qa.z = z; qa.latents = zp;
    qa.M = (int)M; qa.T = T; qa.D = d->latent; qa.Dp = cpad(d->latent); qa.d = dd; qa.K = d->cfg.codebook_size; qa.n = n;
    qa.clip_n = cn; qa.frame_len = fl;
    if (fl && cn) launch_rvq<true, DAC_Q_LEN | DAC_Q_CLIPS>(d->latent, M, qa, st);
    else if (fl) launch_rvq<true, DAC_Q_LEN | DAC_Q_PLAIN>(d->latent, M, qa, st);
    else if (cn) launch_rvq<true, DAC_Q_CLIPS>(d->latent, M, qa, st);
    else launch_rvq<true, DAC_Q_PLAIN>(d->latent, M, qa, st);
    return launch_ok("escx_dac_from_latents");
}

}  // namespace

extern "C" int escx_dac_quantize(escx_dac d, const float* flat, int64_t version, const float* z, int B, int T, int n_q, float* zq, int64_t* codes, float* latents,
                                 float* losses, void* stream) {
    return quantize_impl(d, flat, version, z, B, T, n_q, nullptr, nullptr, zq, codes, latents, losses, stream);
}
extern "C" int escx_dac_quantize_ex(escx_dac d, const float* flat, int64_t version, const float* z, int B, int T, int n_q, const int32_t* clip_n, float* zq,
                                    int64_t* codes, float* latents, float* losses, void* stream) {
    return quantize_impl(d, flat, version, z, B, T, n_q, nullptr, clip_n, zq, codes, latents, losses, stream);
}
extern "C" int escx_dac_quantize_lengths(escx_dac d, const float* flat, int64_t version, const float* z, int B, int Tmax, const int32_t* frame_lengths, int n_q,
                                         const int32_t* clip_n, float* zq, int64_t* codes, float* latents, float* losses, void* stream) {
    if (!frame_lengths) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null frame_lengths");
    return quantize_impl(d, flat, version, z, B, Tmax, n_q, frame_lengths, clip_n, zq, codes, latents, losses, stream);
}

extern "C" int escx_dac_quantize_backward(escx_dac d, const float* flat, int64_t version, const float* latents, const int64_t* codes, int B, int T, int n,
                                          const int32_t* clip_n, const float* d_zq, const float* d_latents, const float* d_commitment, float* d_z, void* stream) {
    int rc = quantize_backward_args(d, flat, latents, codes, B, T, n, clip_n); if (rc) return rc;
    if (!d_z) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_scratch(d, pad64((size_t)B * T * cpad(d->latent)) * sizeof(float)))) return rc;
    const int* counts; if ((rc = upload_stage_counts(d, clip_n, B, n, &counts, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st))) return rc;
    launch_rvq_grad_out(d, latents, codes, counts, d_zq, d_latents, d_commitment, B, T, n, d->scratch, d_z, st);
    return launch_ok("escx_dac_quantize_backward");
}

extern "C" int escx_dac_quantize_backward_params(escx_dac d, const float* flat, int64_t version, const float* z, const float* latents, const int64_t* codes, int B,
                                                 int T, int n, const int32_t* clip_n, const float* d_zq, const float* d_latents, const float* d_commitment,
                                                 const float* d_codebook, float* d_z, float* grad, void* stream) {
    int rc = quantize_backward_args(d, flat, latents, codes, B, T, n, clip_n); if (rc) return rc;
    if (!z || !grad) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int D = d->latent, Dp = cpad(D), dp = cpad(d->cfg.codebook_dim);
    const size_t M = (size_t)B * T, zf = pad64(M * Dp), qrow = pad64(M * dp);
    ParamWs w = enc_param_ws_plan(d);
    if ((rc = ensure_scratch(d, (5 * zf + 2 * qrow) * sizeof(float)))) return rc;
    if (!d->pwe) ESCX_HIP(hipMalloc((void**)&d->pwe, w.total() * sizeof(float)));
    w.pw = d->pwe; w.pw16 = d->pwe16;                           // the projections' contractions stay on the fp32 MFMA (param_layer, split_ok false)
    const int* counts; if ((rc = upload_stage_counts(d, clip_n, B, n, &counts, st))) return rc;
    if ((rc = pack(d, flat, (long long)version, st))) return rc;
    float* A = d->scratch; float* zmap = A + zf; float* Em = A + 5 * zf;
    if (d_z) launch_rvq_grad_out(d, latents, codes, counts, d_zq, d_latents, d_commitment, B, T, n, A, d_z, st);   // escx_dac_quantize_backward's launches
    hipLaunchKernelGGL(dac_z_in_kernel, dim3(nblk((long long)M * Dp)), dim3(256), 0, st, z, zmap, B, D, Dp, T);
    const QParamMaps qm{zmap, A + 2 * zf, A + 3 * zf, A + 4 * zf, Em, Em + qrow};
    if ((rc = quantizer_param_grads(d, w, st, qm, latents, (const long long*)codes, counts, d_zq, d_latents, d_commitment, d_codebook, B, T, n, flat, grad))) return rc;
    return launch_ok("escx_dac_quantize_backward_params");
}

extern "C" int escx_dac_from_latents(escx_dac d, const float* flat, int64_t version, const float* latents, int B, int C, int T, float* z, float* zp, int64_t* codes,
                                     void* stream) {
    return from_latents_impl(d, flat, version, latents, B, C, T, nullptr, nullptr, z, zp, codes, stream);
}
extern "C" int escx_dac_from_latents_ex(escx_dac d, const float* flat, int64_t version, const float* latents, int B, int C, int T, const int32_t* clip_n, float* z,
                                        float* zp, int64_t* codes, void* stream) {
    return from_latents_impl(d, flat, version, latents, B, C, T, nullptr, clip_n, z, zp, codes, stream);
}
extern "C" int escx_dac_from_latents_lengths(escx_dac d, const float* flat, int64_t version, const float* latents, int B, int C, int Tmax,
                                             const int32_t* frame_lengths, const int32_t* clip_n, float* z, float* zp, int64_t* codes, void* stream) {
    if (!frame_lengths) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null frame_lengths");
    return from_latents_impl(d, flat, version, latents, B, C, Tmax, frame_lengths, clip_n, z, zp, codes, stream);
}

extern "C" int escx_dac_test_grad_math(const float* x, const float* alpha, float* out, int64_t n, int mode, void* stream) {
    if (!x || !out || n < 0 || mode < 0 || mode > 1 || (mode == 0 && !alpha)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (n) hipLaunchKernelGGL(dac_test_grad_math_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, x, alpha, out, (long long)n, mode);
    return launch_ok("escx_dac_test_grad_math");
}

extern "C" int escx_dac_test_math(const float* x, const float* alpha, float* out, int64_t n, int mode, void* stream) {
    if (!x || !out || n < 0 || mode < 0 || mode > 1 || (mode == 0 && !alpha)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if (n) hipLaunchKernelGGL(dac_test_math_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, x, alpha, out, (long long)n, mode);
    return launch_ok("escx_dac_test_math");
}
