/*
 * escx.h -- C ABI of the MI355X-native ESC encode/decode hot path (libescx.so, HIP / gfx950).
 *
 * The reference (yzGuu830/efficient-speech-codec) is pure Python; it has no FFI layer.  The boundary
 * this library replaces is the body of `esc.ESC.encode/.decode/.forward` (esc/models/codecs.py:30-94)
 * and the modules underneath.  Each entry point below names the reference function it stands for.
 * The reference-side binding a maintainer would add is a ctypes stub: see INTEGRATION.md.
 *
 * Conventions
 *   - every function returns 0 on success, a negative escx_status on failure; the message for the
 *     calling thread is available from escx_last_error().  Nothing throws across the ABI.
 *   - `*_dev` pointers are device pointers owned by the caller (e.g. torch `tensor.data_ptr()`);
 *     `stream` is a hipStream_t passed as void* (0 = the null stream).  Calls are asynchronous with
 *     respect to the host unless stated otherwise.
 *   - parameters are uploaded once from HOST fp32 buffers under the reference's state_dict key names
 *      and packed into MFMA-friendly padded layouts owned by the handle.
 *   - the handle owns one workspace, sized by escx_reserve(); a handle serves one stream at a time.
 *   - stage-level entry points take and return tensors in the REFERENCE layouts (unpadded), so they can
 *     be compared one-to-one with the reference functions; the whole-path calls keep activations in the
 *     internal padded layouts between kernels.
 */
#ifndef ESCX_H
#define ESCX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESCX_MAX_SCALES 8

typedef enum {
    ESCX_OK = 0,
    ESCX_ERR_INVALID_ARG = -1,      /* bad shape / null pointer / unknown key             */
    ESCX_ERR_UNSUPPORTED = -2,      /* configuration outside what the kernels implement   */
    ESCX_ERR_HIP = -3,              /* a HIP runtime call failed                          */
    ESCX_ERR_STATE = -4,            /* e.g. parameters not finalised                      */
    ESCX_ERR_ASSERT = -5            /* a reference assertion would have fired             */
} escx_status;

/* Mirrors the kwargs of esc.ESC.__init__ (esc/models/codecs.py:11-18). */
typedef struct {
    int32_t in_dim;                         /* 2                                           */
    int32_t in_freq;                        /* 192  -> n_fft = 2*(in_freq-1)               */
    int32_t n_scales;                       /* len(h_dims) = 6                             */
    int32_t h_dims[ESCX_MAX_SCALES];        /* 45,72,96,144,192,384                        */
    int32_t max_streams;                    /* 6                                           */
    int32_t win_length;                     /* int(win_len*sr*1e-3) = 320                  */
    int32_t hop_length;                     /* int(hop_len*sr*1e-3) = 80                   */
    int32_t patch_f, patch_t;               /* 3, 2                                        */
    int32_t swin_heads[ESCX_MAX_SCALES];    /* encoder order: 3,6,12,24,24                 */
    int32_t swin_depth;                     /* 2 (Base) / 4 (Large)                        */
    int32_t window_size;                    /* 2 .. 16; 4 = fused kernels, other sizes: unfused fallback, inference only */
    float   mlp_ratio;                      /* 4.0                                         */
    int32_t overlap;                        /* 2                                           */
    int32_t group_size;                     /* 3                                           */
    int32_t codebook_size;                  /* 1024                                        */
    int32_t codebook_dims[ESCX_MAX_SCALES]; /* per stream                                  */
    int32_t l2norm;                         /* 1                                           */
} escx_config;

typedef struct escx_handle_s* escx_handle;

/* Mirrors the kwargs of esc.RVQCodecs.__init__ (esc/models/codecs.py:96-127, the rvq+swinT ablation): the Swin backbone of ESC with a
 * product-residual VQ at the bottleneck only (quantization.py:292-431).  base.group_size = number of product groups (num_pvqs),
 * base.codebook_dims is ignored (every stage of every group has codebook_dim), base.max_streams = len(h_dims) as for ESC. */
typedef struct {
    escx_config base;
    int32_t num_rvqs;                       /* residual stages per group = the largest num_streams (6)   */
    int32_t codebook_dim;                   /* 8                                                          */
} escx_rvq_config;

/* ---- lifetime ------------------------------------------------------------------------------- */
const char* escx_last_error(void);
const char* escx_version(void);
/* ESC.__init__ (codecs.py:11-28, base.py:12-27,49-71): validates the configuration, derives geometry. */
int escx_create(const escx_config* cfg, int device, escx_handle* out);
/* RVQCodecs.__init__ (codecs.py:96-127, base.py:73-84).  The quantiser runs as one fused gfx950 kernel per batch part (fused_prvq.h), instantiated
 * for codebook_dim 5..8 with 3 or 4 groups (the ablation yaml: 3 x 8) and for codebook_dim <= 4 with up to 4 groups; another geometry, a group whose
 * width equals codebook_dim (no projection in the reference) or num_rvqs outside [1, 16] is ESCX_ERR_UNSUPPORTED here, never wrong output later.
 * Required keys: the backbone's (encoder.*, decoder.blocks.*, decoder.post_nn.*, decoder.patch_deembed.*) and, per group m and stage i,
 * quantizers.vqs.{m}.proj_down.weight (d, D_m), quantizers.vqs.{m}.proj_up.weight (D_m, d), quantizers.vqs.{m}.vqs.{i}.embedding.weight (K, d).
 * On such a handle escx_encode / escx_decode / escx_forward / escx_forward_feat and the three *_streams calls run the rvq+swinT codec with
 * num_streams (per clip, for *_streams) in [1, num_rvqs]; codes keep the (B, S, G, T) layout.  The training step has entry points of its own
 * (escx_rvq_train_forward / escx_rvq_train_backward); escx_train_forward, escx_train_forward_feat, escx_train_backward, escx_train_backward_ex,
 * escx_pvq_encode and escx_pvq_decode return ESCX_ERR_UNSUPPORTED; the flat-parameter calls (escx_flat_param_*, escx_load_flat_params) and
 * escx_train_tape_bytes / escx_train_tape_generation work as for ESC. */
int escx_create_rvq(const escx_rvq_config* cfg, int device, escx_handle* out);
/* 0 = cross-scale product VQ (escx_create, ESC), 1 = bottleneck product-residual VQ (escx_create_rvq, RVQCodecs); negative for a null handle. */
int escx_quantizer_kind(escx_handle h);
void escx_destroy(escx_handle h);

/* nn.Module.load_state_dict (compress.py:23-25): one call per state_dict entry, HOST fp32, C-contiguous.
 * Keys: SURVEY.md appendix C.  `*.relative_position_index` and `*.window` are accepted and ignored
 * (the index is regenerated, the window is folded into the DFT matrices). */
int escx_set_param(escx_handle h, const char* key, const float* host_data, const int64_t* shape, int ndim);
/* Packs (pads, permutes, pre-normalises codebooks) and uploads; fails if a required key is missing. */
int escx_finalize_params(escx_handle h);
/* Number of keys escx_finalize_params() requires, and the i-th one (for load_state_dict(strict=True)). */
int escx_num_required_keys(escx_handle h);
const char* escx_required_key(escx_handle h, int i);

/* Allocates the workspace for batches up to `batch` clips of `n_samples` samples (synchronous; never
 * call while capturing a graph).  Whole-path calls reserve on demand. */
int escx_reserve(escx_handle h, int batch, int n_samples);
int64_t escx_workspace_bytes(escx_handle h);

/* ---- arithmetic of the code-emitting path ------------------------------------------------------
 * The reference computes every contraction in fp32 on ATen sgemm / bmm (esc/modules/transformer/attention.py:215-272, esc/modules/transformer/scale.py:42-145,
 * esc/modules/vq/codebook.py:31-40).  This library accumulates in fp32 everywhere; what can be chosen PER HANDLE is the form of the operands of the dense contractions
 * with K = C - fc1 / fc2 of every FeedForward, the Q / K / V projections (and, in the two-term mode, the output projection) of every WindowAttention, PatchMerge /
 * PatchSplit and, in the two-term mode, the composed PatchDeEmbed convolution (the attention's scores and P.V, the codebook search of Codebook.quantize_to_code,
 * PatchEmbed and the STFT / ISTFT GEMMs run on the fp32 MFMA in every mode):
 *   ESCX_PRECISION_FP32    every contraction on v_mfma_f32_16x16x4_f32 with fp32 operands.
 *   ESCX_PRECISION_BF16X3  every fp32 operand split EXACTLY into three bf16 terms (a = a1 + a2 + a3; bf16 has fp32's exponent range, so there is no range condition);
 *                          the six leading cross products are accumulated in fp32 on v_mfma_f32_16x16x32_bf16, smallest first.  Dropped terms < 2^-24 of a product:
 *                          the result differs from ESCX_PRECISION_FP32 only by fp32 summation order.
 *   ESCX_PRECISION_F16X2   (default) every fp32 operand a ~ a1 + a2, two fp16 terms (|a - a1 - a2| <= 2^-22 |a|), three cross products on v_mfma_f32_16x16x32_f16.
 *                          NOT exact: truncation ~1e-7 of the result magnitude, below fp32 accumulation rounding (measured: tests/test_gpu_parity.py
 *                          test_layer_accuracy_against_fp64).  Range-safe by construction: every operand is multiplied by a power of two chosen from a bound that
 *                          holds for ANY finite input (weights: max |w|; LayerNorm outputs: max |gamma| sqrt(C) + max |beta|; GELU outputs: Cauchy-Schwarz on fc1;
 *                          attention outputs: the V bound; de-embedding input: the tile's own max) and the accumulator by its inverse - exact operations - so no finite input overflows fp16 and
 *                          low terms stay normal numbers (csrc/split_terms.h).  No silent NaN, no fallback, no host synchronisation.
 * The mode is a property of the handle: it takes effect with the next call (the split weight images are re-derived on that call's stream) and a clip's codes do not
 * depend on the batch or shard it is processed in under any mode.  New handles start in the mode named by the environment variable ESCX_PRECISION (fp32 | bf16x3 | f16x2)
 * if set, else ESCX_PRECISION_F16X2.  escx_set_precision returns ESCX_ERR_INVALID_ARG for another value; escx_get_precision returns the mode in effect. */
#define ESCX_PRECISION_FP32   0
#define ESCX_PRECISION_F16X2  2
#define ESCX_PRECISION_BF16X3 3
int escx_set_precision(escx_handle h, int mode);
int escx_get_precision(escx_handle h);

/* ---- whole path ----------------------------------------------------------------------------- */
/* ESC.encode (codecs.py:68-81): wave (B,L) f32 -> codes (B,num_streams,group_size,W/overlap) int64,
 * feat_shape (H_bottom, W) written to host ints. */
int escx_encode(escx_handle h, const float* wave_dev, int batch, int n_samples, int num_streams,
                int64_t* codes_dev, int* feat_h, int* feat_w, void* stream);
/* ESC.decode (codecs.py:83-94): codes (B,S,G,T) int64 + feat_shape -> wave (B, hop*(2W-1)) f32.
 * recon_feat_dev (optional, may be NULL): (B, 2W, 2, in_freq) f32 frame-major spectrum, i.e. the
 * reference's recon_feat (B,2,F,T) permuted (0,3,1,2). */
/* Code indices outside [0, codebook_size) are clamped (the reference's F.embedding raises a device-side assert there). */
int escx_decode(escx_handle h, const int64_t* codes_dev, int batch, int num_streams, int feat_h, int feat_w,
                float* wave_out_dev, float* recon_feat_dev, void* stream);
/* ESC.forward in eval mode (codecs.py:30-66, csrvq.py:97-129): encoder once, quantise + decode in one pass.
 * raw_feat_dev (optional): (B, T, 2, in_freq) frame-major; cm_loss_dev (optional): (B,) f32 (== cb_loss). */
int escx_forward(escx_handle h, const float* wave_dev, int batch, int n_samples, int num_streams,
                 int64_t* codes_dev, float* wave_out_dev, float* raw_feat_dev, float* recon_feat_dev,
                 float* cm_loss_dev, void* stream);
/* The same with a precomputed spectrum instead of the waveform (forward(x, x_feat=...), codecs.py:33-34): feat_dev is
 * (B, T, 2, in_freq) f32 frame-major, i.e. the reference's x_feat (B,F,T,2) permuted (0,2,3,1); the STFT is skipped. */
int escx_forward_feat(escx_handle h, const float* feat_dev, int batch, int n_frames, int num_streams,
                      int64_t* codes_dev, float* wave_out_dev, float* recon_feat_dev, float* cm_loss_dev, void* stream);
/* Mixed-bitrate batches: the same three calls with a stream count PER CLIP.  `streams` is a HOST array of `batch` counts, each in [1, max_streams]
 * (the counts shape the launches).  Clip b's results are bit for bit those of the uniform call at num_streams = streams[b]: the codes of S streams
 * are the first S of the S = max_streams codes (csrvq.py:131-158) and untransmitted streams pass through the decoder (csrvq.py:160-183, :35-36).
 * Each stream and each decoder block that feeds a later stream runs only on the clips that need it.  A null `streams`, batch < 1 or a count
 * outside the range is ESCX_ERR_INVALID_ARG.  The counts are uploaded with every call and the handle's staging buffer grows (synchronously) on first
 * use of a larger batch: these calls are not meant for graph capture.
 * ESC.encode (codecs.py:68-81): codes (B, Smax, G, W/overlap) int64, Smax = max(streams); slots [streams[b], Smax) of clip b are -1. */
int escx_encode_streams(escx_handle h, const float* wave_dev, int batch, int n_samples, const int32_t* streams,
                        int64_t* codes_dev, int* feat_h, int* feat_w, void* stream);
/* ESC.decode (codecs.py:83-94): codes (B, smax, G, T) with smax >= max(streams); slots at or past streams[b] are never read.  Codes outside
 * [0, codebook_size) in the slots below streams[b] are clamped, as in escx_decode. */
int escx_decode_streams(escx_handle h, const int64_t* codes_dev, int batch, int smax, const int32_t* streams, int feat_h, int feat_w,
                        float* wave_out_dev, float* recon_feat_dev, void* stream);
/* ESC.forward in eval mode (codecs.py:30-66, csrvq.py:97-129): exactly one of wave_dev (B, n_samples) / feat_dev (B, n_frames, 2, in_freq)
 * is given (n_samples_or_frames is the matching length); outputs as escx_forward with codes (B, max(streams), G, T), -1 past each clip's streams;
 * cm_loss[b] sums only clip b's own streams. */
int escx_forward_streams(escx_handle h, const float* wave_dev, const float* feat_dev, int batch, int n_samples_or_frames, const int32_t* streams,
                         int64_t* codes_dev, float* wave_out_dev, float* raw_feat_dev, float* recon_feat_dev, float* cm_loss_dev, void* stream);
/* Mixed-length batches (csvq+swinT handles, window_size 4): the same three calls with a length PER CLIP.  wave_dev is (B, row_len) f32; `lengths` is a HOST
 * array of `batch` sample counts, each in (n_fft / 2, row_len]; what is stored at or past lengths[b] in row b is not read.  Clip b has
 * W_b = (1 + lengths[b] / hop) / patch_t latent frames and gets what the plain call on its own lengths[b] samples computes (same codes under the near-tie
 * rule of the parity tests, audio within fp32 summation order): the STFT reflects about its last sample, the shifted windows roll over its own padded width,
 * the de-embedding zero-pads at its own end and the overlap-add normalises its own tail.  A clip's results are a function of its samples, lengths[b],
 * Wmax = max W_b, num_streams and the precision mode - bit for bit the same in any batch, at any position, next to any other clips of the same Wmax.
 * A W_b that is no multiple of `overlap` is ESCX_ERR_ASSERT (the message names the clip); a null table, batch < 1 or a length out of range is
 * ESCX_ERR_INVALID_ARG; rvq+swinT handles and other window sizes are ESCX_ERR_UNSUPPORTED - all before any launch.  The tables are uploaded with every call
 * and the batch runs as one part on the caller's stream: not meant for graph capture.
 * ESC.encode (codecs.py:68-81): codes (B, num_streams, G, Wmax / overlap) int64, -1 at the frames at or past W_b / overlap; feat_shape (H_bottom, Wmax). */
int escx_encode_lengths(escx_handle h, const float* wave_dev, int batch, int row_len, const int32_t* lengths, int num_streams,
                        int64_t* codes_dev, int* feat_h, int* feat_w, void* stream);
/* ESC.decode (codecs.py:83-94): `widths` is a HOST array of `batch` latent widths W_b, each a positive multiple of `overlap` and at most feat_w.
 * wave_out (B, hop * (patch_t * feat_w - 1)) is 0 at and past hop * (patch_t * W_b - 1); recon_feat_dev (optional) has zero frames past patch_t * W_b.
 * The code frames at or past W_b / overlap are never read. */
int escx_decode_lengths(escx_handle h, const int64_t* codes_dev, int batch, int num_streams, const int32_t* widths, int feat_h, int feat_w,
                        float* wave_out_dev, float* recon_feat_dev, void* stream);
/* ESC.forward in eval mode (codecs.py:30-66, csrvq.py:97-129): outputs as escx_forward at Tmax = 1 + max(lengths) / hop and Wmax; raw_feat_dev (optional) is
 * (B, Tmax, 2, in_freq) with zero frames past 1 + lengths[b] / hop, codes / wave_out / recon_feat as the two calls above, cm_loss[b] (== cb_loss) the mean
 * over clip b's own W_b / overlap code frames. */
int escx_forward_lengths(escx_handle h, const float* wave_dev, int batch, int row_len, const int32_t* lengths, int num_streams,
                         int64_t* codes_dev, float* wave_out_dev, float* raw_feat_dev, float* recon_feat_dev, float* cm_loss_dev, void* stream);
int escx_num_frames(escx_handle h, int n_samples);      /* T = 1 + n_samples / hop                      */
int escx_output_samples(escx_handle h, int feat_w);     /* hop * (patch_t * W - 1)                      */

/* ---- stage level (reference layouts; used by the parity tests) ------------------------------- */
/* BaseAudioCodec.spec_transform (base.py:29-37): (B,L) -> (B,T,2,F) frame-major [= (B,2,F,T).permute(0,3,1,2)] */
int escx_spec_transform(escx_handle h, const float* wave_dev, int batch, int n_samples, float* spec_dev, void* stream);
/* BaseAudioCodec.audio_reconstruct (base.py:39-47): (B,T,2,F) -> (B, hop*(T-1)) */
int escx_audio_reconstruct(escx_handle h, const float* spec_dev, int batch, int n_frames, float* wave_dev, void* stream);
/* PatchEmbed.forward (scale.py:42-50): spec (B,T,2,F) -> tokens (B, H*W, C0) */
int escx_patch_embed(escx_handle h, const float* spec_dev, int batch, int n_frames, float* tokens_dev, void* stream);
/* TransformerLayer.forward (attention.py:48-91).  layer_id: 0 = encoder.pre_nn, 1..n-1 = encoder.blocks[i-1],
 * n..2n-2 = decoder.blocks[i-n], 2n-1 = decoder.post_nn  (n = n_scales).  x (B,H*W,C) -> y (B,H'*W,C'). */
int escx_transformer_layer(escx_handle h, int layer_id, const float* x_dev, int batch, int H, int W,
                           float* y_dev, int* H_out, void* stream);
/* CrossScaleRVQ.csrvq_encode / PVQ.encode (csrvq.py:50-54, quantization.py:74-91, codebook.py:20-43):
 * codes[b,g,t] for residual = enc - dec (dec may be NULL -> residual = enc).  codes_dev: (B,G,T) int64
 * with `code_batch_stride` elements between clips (lets the caller write straight into (B,S,G,T)). */
int escx_pvq_encode(escx_handle h, int stream_id, const float* enc_dev, const float* dec_dev, int batch, int W,
                    int64_t* codes_dev, int64_t code_batch_stride, void* stream);
/* CrossScaleRVQ.csrvq_decode / PVQ.decode (csrvq.py:56-60, quantization.py:93-108): out = dec + dequant(codes). */
int escx_pvq_decode(escx_handle h, int stream_id, const int64_t* codes_dev, int64_t code_batch_stride,
                    const float* dec_dev, int batch, int W, float* out_dev, void* stream);
/* ProductResidualVectorQuantize.encode / .forward in eval mode (quantization.py:292-378) on an rvq handle: tokens (B, Hq*W, C) of the bottleneck
 * (reference layout) -> codes (B, S, G, W/overlap) int64, 1 <= S <= num_rvqs; zq_out (optional, (B, Hq*W, C)) = post_process(proj_up(sum of the
 * raw rows of the S stages)), the decoder's input.  Synchronous with respect to `stream` only. */
int escx_rvq_encode(escx_handle h, const float* tokens_dev, int batch, int W, int num_streams, int64_t* codes_dev, float* zq_out_dev, void* stream);
/* ProductResidualVectorQuantize.decode (quantization.py:406-420): codes (B, S, G, W/overlap) -> tokens (B, Hq*W, C). */
int escx_rvq_decode(escx_handle h, const int64_t* codes_dev, int batch, int num_streams, int W, float* tokens_out_dev, void* stream);
/* PatchDeEmbed.forward (scale.py:73-81): tokens (B,H0*W,C0) -> spec (B, 2W, 2, F) frame-major */
int escx_patch_deembed(escx_handle h, const float* tokens_dev, int batch, int W, float* spec_dev, void* stream);

/* ---- per-kernel timing (HIP events recorded on the caller's stream around every launch) ------- */
/* enable != 0 starts recording (and clears earlier records); enable == 0 stops.  enable == 2 additionally runs the batch parts
 * back to back on the caller's stream, so that each kernel is timed alone on the GPU. */
int escx_profile_enable(escx_handle h, int enable);
/* Synchronises, aggregates by kernel label and returns a JSON array
 * [{"name":..., "calls":n, "ms":total, "flops":algorithmic, "bytes":algorithmic}, ...] valid until the next call. */
const char* escx_profile_report(escx_handle h);

/* Device math used inside the fused kernels, exposed for the accuracy tests: which = 0 gelu (branch-free erf),
 * 1 erf (branch-free), 2 exp via v_exp_f32, 3 gelu via libm erff (the unfused epilogue). */
/* Debug: device buffer for the per-wave phase stamps of the fused attention / product-VQ kernels (phase-trace builds: -DESCX_ATTN_TRACE, -DESCX_PVQ_TRACE). */
int escx_debug_mlp_trace(unsigned long long* dev_buf);
int escx_test_math(const float* x_dev, float* y_dev, int64_t n, int which, void* stream);
/* Counter calibration (tools/pmc_calib.py): copies `rows` rows of `row_floats` floats with the fused kernels' access pattern (16 lanes per
 * row, 16 B per lane), so that rocprofv3's FETCH_SIZE / WRITE_SIZE can be compared with a known byte count. */
int escx_test_copy_rows(const float* src_dev, float* dst_dev, int64_t rows, int row_floats, void* stream);
/* Host-side evaluation of the multiply-high division the gather loaders / scatter epilogues use on the device (gemm_engine.h FastDiv):
 * returns n / d for 0 <= n < 2^31, 1 <= d < 2^31 (no GPU needed; tests compare it with exact division). */
int escx_test_fastdiv(int n, int d);

/* ---- code packing for transport (10-bit codes; all-gather payload) --------------------------- */
/* 10-bit wire format (codebook_size 1024): n codes <-> 5*ceil(n/4) bytes; 6 streams x 3 groups x 50 Hz x 10 b = 9 kbps (base.py:70). */
int escx_codes_pack10(const int64_t* codes_dev, uint8_t* out_dev, int64_t n, void* stream);
int escx_codes_unpack10(const uint8_t* in_dev, int64_t* codes_dev, int64_t n, void* stream);
/* Ragged form for mixed-stream batches: codes (batch, smax, gt) with gt = G*T and a HOST array of per-clip counts in [1, smax].  Pack writes
 * clip b's first streams[b]*gt codes, clips in order, as one 10-bit stream of 5*ceil(n/4) bytes (n = gt * sum(streams)); unpack restores the
 * padded layout with -1 in the slots at or past streams[b].  One launch each. */
int escx_codes_pack10_streams(const int64_t* codes_dev, int batch, int smax, int64_t gt, const int32_t* streams, uint8_t* out_dev, void* stream);
int escx_codes_unpack10_streams(const uint8_t* in_dev, int batch, int smax, int64_t gt, const int32_t* streams, int64_t* codes_dev, void* stream);
int escx_codes_narrow(const int64_t* codes_dev, int16_t* out_dev, int64_t n, void* stream);
int escx_codes_widen(const int16_t* in_dev, int64_t* codes_dev, int64_t n, void* stream);

/* ---- training step (BASELINE configs[4]) --------------------------------------------------------------
 * Reference: scripts/trainer_no_adv.py:95-118 (step), esc/models/codecs.py:30-66 + esc/models/csrvq.py:23-48,97-129 (training-mode
 * forward), esc/modules/vq/codebook.py:57-75 (straight-through estimator, commitment / codebook losses),
 * esc/modules/vq/quantization.py:53-64 (freeze_vq), esc/modules/loss/generator_loss.py:12-74 (losses).  fp32, like the reference.
 * Trainable parameters live in ONE flat fp32 device buffer owned by the caller, in the order escx_flat_param_*() reports (the keys
 * escx_finalize_params requires, reference shapes, C-contiguous); gradients are returned in a buffer of the same layout. */
int escx_flat_param_count(escx_handle h);
const char* escx_flat_param_key(escx_handle h, int i);
int64_t escx_flat_param_offset(escx_handle h, int i);        /* in floats */
int64_t escx_flat_param_numel(escx_handle h, int i);
int64_t escx_flat_param_total(escx_handle h);
/* Re-derives every packed layout from the flat buffer.  full == 0: on the device (gather + codebook normalisation; asynchronous),
 * enough for the training step; full != 0: additionally rebuilds the host-folded layouts of the inference path (synchronous). */
int escx_load_flat_params(escx_handle h, const float* flat_params_dev, int full, void* stream);
/* ESC.forward in training mode (ESCX_ERR_UNSUPPORTED on an RVQCodecs handle, whose step is escx_rvq_train_forward).  flat_params_dev may be NULL (keep the currently packed weights).  codes_dev: (B, max_streams, G, T)
 * int64 - every stream is quantised in training mode (csrvq.py:104-113); wave_out (B, hop*(2W-1)); raw_feat (B,T,2,F) and recon_feat
 * (B,2W,2,F) frame-major, optional; cm_loss / cb_loss (B,), optional.  Activations stay on the handle's tape until the backward. */
int escx_train_forward(escx_handle h, const float* flat_params_dev, const float* wave_dev, int batch, int n_samples, int num_streams,
                       int freeze_codebook, int64_t* codes_dev, float* wave_out_dev, float* raw_feat_dev, float* recon_feat_dev,
                       float* cm_loss_dev, float* cb_loss_dev, void* stream);
/* The same with a precomputed spectrum instead of the waveform (forward(x, x_feat=...) in training mode, codecs.py:33-34): feat_dev is (B, T, in_dim, F) f32 frame-major,
 * i.e. the reference's x_feat (B,F,T,2) permuted (0,2,3,1); the STFT is skipped, everything downstream (tape, backward) is escx_train_forward's.
 * ESCX_ERR_UNSUPPORTED on an RVQCodecs handle (escx_rvq_train_forward takes the spectrum there). */
int escx_train_forward_feat(escx_handle h, const float* flat_params_dev, const float* feat_dev, int batch, int n_frames, int num_streams, int freeze_codebook,
                            int64_t* codes_dev, float* wave_out_dev, float* recon_feat_dev, float* cm_loss_dev, float* cb_loss_dev, void* stream);
/* Backward of the last escx_train_forward.  Upstream gradients (any may be NULL = zero): d_wave (B, out_len), d_recon_feat (B,2W,2,F),
 * d_cm_loss / d_cb_loss (B,).  grad_flat_dev receives d loss / d parameter in the flat layout (overwritten, not accumulated).
 * ESCX_ERR_UNSUPPORTED on an RVQCodecs handle (escx_rvq_train_backward). */
int escx_train_backward(escx_handle h, const float* d_wave_dev, const float* d_recon_feat_dev, const float* d_cm_loss_dev,
                        const float* d_cb_loss_dev, float* grad_flat_dev, void* stream);
/* escx_train_backward with the input side (the reference's autograd through spec_transform and the straight-through estimator).
 * d_raw_feat_dev (B,T,2,F), optional: upstream gradient of the forward's raw spectrum output.  d_input_dev, optional: receives d loss / d input,
 * (B, n_samples) after escx_train_forward (patch-embedding dX + d_raw_feat, then the STFT adjoint), (B,T,2,F) after escx_train_forward_feat.
 * grad_flat_dev may be NULL: no parameter gradient, and no launch whose only product is one (a frozen codec in a larger graph).
 * ESCX_ERR_INVALID_ARG when both outputs are NULL; ESCX_ERR_UNSUPPORTED on an RVQCodecs handle (escx_rvq_train_backward). */
int escx_train_backward_ex(escx_handle h, const float* d_wave_dev, const float* d_recon_feat_dev, const float* d_raw_feat_dev,
                           const float* d_cm_loss_dev, const float* d_cb_loss_dev, float* grad_flat_dev, float* d_input_dev, void* stream);
/* RVQCodecs.forward in training mode (codecs.py:127-167) on an rvq handle: encoder, ONE product-residual quantiser step at the bottleneck
 * (quantization.py:298-335 ProductResidualVectorQuantize.forward, 167-196 residual_vector_quantization, codebook.py:57-75 straight-through estimator and
 * losses), the plain decoder (base.py:195-203).  Exactly one of wave_dev (B, n) and feat_dev ((B, n, in_dim, F) frame-major as escx_forward_feat's) is
 * given, n = samples or frames.  Every one of the num_rvqs stages runs, so codes_dev is (B, num_rvqs, G, T) int64; stages >= num_streams are masked
 * out of the reconstruction and of the losses (quantization.py:185-187); num_streams in [1, num_rvqs].  freeze_codebook: the up-projection sees
 * z_e + z_q * 0 and the losses are zero (quantization.py:319-321).  cm_loss = cb_loss = sum over groups and live stages of mse(z_q_i, residual_i)
 * per clip / groups.  raw_feat_dev is ignored with feat_dev.  Other outputs, the tape, the batch parts and flat_params_dev as escx_train_forward.
 * ESCX_ERR_UNSUPPORTED on an escx_create handle and for window_size != 4. */
int escx_rvq_train_forward(escx_handle h, const float* flat_params_dev, const float* wave_dev, const float* feat_dev, int batch, int n_samples_or_frames,
                           int num_streams, int freeze_codebook, int64_t* codes_dev, float* wave_out_dev, float* raw_feat_dev, float* recon_feat_dev,
                           float* cm_loss_dev, float* cb_loss_dev, void* stream);
/* Backward of the last escx_rvq_train_forward: what the reference's autograd gives through RVQCodecs.forward_one_step (codecs.py:127-148).  With
 * g = d L / d z_q_m from the up-projection: d z_e = g + 2 / (T d G) d_cm[b] (z_e - q_0) (frozen: g); the residual chain carries no gradient
 * (d r_{i+1} / d r_i = 1 - 1: quantization.py:184 with codebook.py:70); codebook row code_i of a stage i < num_streams receives
 * 2 / (T d G) d_cb[b] (q_i - r_i) summed over the vectors that chose it, in a fixed order; stages >= num_streams and the frozen form get exact zeros.
 * Arguments and null rules as escx_train_backward_ex. */
int escx_rvq_train_backward(escx_handle h, const float* d_wave_dev, const float* d_recon_feat_dev, const float* d_raw_feat_dev,
                            const float* d_cm_loss_dev, const float* d_cb_loss_dev, float* grad_flat_dev, float* d_input_dev, void* stream);
/* Bytes held for activation tapes (both kinds of handle). */
int64_t escx_train_tape_bytes(escx_handle h);
/* Number of training forwards (escx_train_forward*, escx_rvq_train_forward) on this handle so far.  The handle holds ONE tape: escx_train_backward consumes the activations of the
 * LAST forward.  A caller that interleaves several forwards (autograd graphs alive at the same time) records this value after its forward
 * and compares it before its backward; a mismatch means the tape belongs to a later forward (esc/models/codecs.py raises). */
int64_t escx_train_tape_generation(escx_handle h);
/* ComplexSTFTLoss (generator_loss.py:12-35): per-clip loss (B,) = mean over the clip's `per_clip` spectrum values (any layout, the
 * same for both inputs) of (pl(raw) - pl(recon))^2, pl = power-law compression; optionally d loss_b / d recon_feat. */
int escx_stft_loss(const float* raw_feat_dev, const float* recon_feat_dev, int batch, int64_t per_clip, float* loss_dev,
                   float* d_recon_feat_dev, void* stream);
/* The same with d loss_b / d raw_feat as well (d_raw_feat_dev optional; the recon side is computed exactly as escx_stft_loss does). */
int escx_stft_loss_ex(const float* raw_feat_dev, const float* recon_feat_dev, int batch, int64_t per_clip, float* loss_dev,
                      float* d_recon_feat_dev, float* d_raw_feat_dev, void* stream);
/* MelSpectrogramLoss (generator_loss.py:37-74; 7 resolutions, windows 32..2048, hop = window/4, HTK mel filterbanks of 5..320 bins,
 * L1 on the mel magnitudes + L1 on log10(clamp(mel)^2)): per-clip loss (B,) and, optionally, d loss_b / d recon_wave (B,L).
 * Runs on the current device; the DFT / filterbank matrices are built once per device (and rebuilt when sample_rate changes).
 * sample_rate: even rates only are verified (the reference fixes 16000): at an odd rate the filterbank's top edge (sr / 2.0) and the bin grid (sr / 2) differ. */
int escx_mel_loss(const float* raw_wave_dev, const float* recon_wave_dev, int batch, int n_samples, int sample_rate, float* loss_dev,
                  float* d_recon_wave_dev, void* stream);
/* The same with d loss_b / d raw_wave (B,L) as well (d_raw_wave_dev optional; the recon side is computed exactly as escx_mel_loss does). */
int escx_mel_loss_ex(const float* raw_wave_dev, const float* recon_wave_dev, int batch, int n_samples, int sample_rate, float* loss_dev,
                     float* d_recon_wave_dev, float* d_raw_wave_dev, void* stream);
int escx_scale_rows(const float* x_dev, const float* g_dev, float* out_dev, int rows, int64_t per_row, void* stream);   /* out[r][:] = x[r][:] * g[r] */
/* clip_grad_norm_ + AdamW on flat buffers (trainer_no_adv.py:116-117).  norm_out_dev: 2 + 1024 floats ([0] = norm, [1] = clip coefficient). */
int escx_grad_norm_clip(const float* grad_flat_dev, int64_t n, float max_norm, float* norm_out_dev, void* stream);
/* Hyper-parameters are doubles, as torch.optim.AdamW holds them (python floats): 1 - beta, lr / (1 - beta1^t), sqrt(1 - beta2^t) and 1 - lr * wd are
 * evaluated in double on the host and reach the kernel as fp32 scalars, exactly as torch's single-tensor path does. */
int escx_adamw_step(float* param_flat_dev, const float* grad_flat_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n, int step,
                    double lr, double beta1, double beta2, double eps, double weight_decay, const float* clip_dev, void* stream);

/* ---- adversarial step: DAC discriminator + GAN losses (BASELINE configs[4]; scripts/trainer_adv.py:61-107) ---------------------------------
 * Reference: esc/models/discriminator.py:31-221 (MPD :31-66, MSD :69-99, MRD :105-176, Discriminator :179-215), esc/modules/loss/gan_loss.py:5-51.
 * Sub-discriminators in the reference's order: one MPD per period, one MSD per rate, one MRD per fft size.  An MSD resamples the pre-processed
 * waveform to sample_rate / rate (integer decimation by a windowed-sinc FIR, DESIGN.md 14.1: the audiotools / julius resampler of the reference is
 * restated, not pinned) and its feature maps are (B, C, T) tensors: D1 = P1 = 1, off1 = 0.  Parameters: one flat fp32 device buffer in the order escx_disc_param_*() reports (the reference's
 * named_parameters(): per convolution bias, weight_g, weight_v).  Feature maps are caller-owned channels-last buffers [B][D0][P1][Cp]
 * (escx_disc_fmap_shape); the reference's (B, C, D0, D1) tensor of map i is buffer[:, :, off1 : off1 + D1, :C] permuted (0, 3, 1, 2). */
typedef struct {
    int32_t sample_rate;                 /* 16000                                                  */
    int32_t n_rates;                     /* 0 .. 8 multi-scale discriminators, see rates[] below   */
    int32_t n_periods; int32_t periods[8];      /* 2, 3, 5, 7, 11                                  */
    int32_t n_ffts; int32_t fft_sizes[8];       /* 2048, 1024, 512                                 */
    int32_t n_bands; float bands[8][2];         /* (0, .1), (.1, .25), (.25, .5), (.5, .75), (.75, 1) */
    int32_t rates[8];                    /* read only when n_rates > 0: each >= 1 (else ESCX_ERR_INVALID_ARG) and a divisor of sample_rate (else ESCX_ERR_UNSUPPORTED) */
} escx_disc_config;
typedef struct escx_disc_s* escx_disc;
int escx_disc_create(const escx_disc_config* cfg, int device, escx_disc* out);
void escx_disc_destroy(escx_disc d);
int escx_disc_param_count(escx_disc d);
const char* escx_disc_param_key(escx_disc d, int i);
int64_t escx_disc_param_offset(escx_disc d, int i);
int64_t escx_disc_param_numel(escx_disc d, int i);
int64_t escx_disc_param_total(escx_disc d);
int escx_disc_num_fmaps(escx_disc d, int n_samples);
int escx_disc_fmap_shape(escx_disc d, int n_samples, int i, int* sub, int* C, int* Cp, int* D0, int* D1, int* P1, int* off1);
/* Discriminator.forward: wave (B, L) -> every feature map (fmaps_dev: HOST array of device pointers, map i's own base address).
 * params_version: a number that changes whenever the CONTENTS of the flat buffer change (negative: unknown); the weight-normalised GEMM operands
 * are re-derived from the flat buffer only when (pointer, version) differs from the previous call. */
int escx_disc_forward(escx_disc d, const float* flat_params_dev, int64_t params_version, const float* wave_dev, int batch, int n_samples,
                      float* const* fmaps_dev, void* stream);
/* Backward of a forward on the same (params, wave, fmaps): d_fmaps_dev[i] (same layout, NULL = zero) -> grad_flat_dev (optional, overwritten)
 * and / or d_wave_dev (optional, (B, L), overwritten). */
int escx_disc_backward(escx_disc d, const float* flat_params_dev, int64_t params_version, const float* wave_dev, int batch, int n_samples,
                       float* const* fmaps_dev, const float* const* d_fmaps_dev, float* grad_flat_dev, float* d_wave_dev, void* stream);
/* Arithmetic of the discriminator's wide convolutions (round 4; BASELINE configs[4] names bf16, the reference's trainer_adv.py runs fp32).
 * 0 (default): fp32 MFMA everywhere, the parity-tested path.  1: the implicit GEMMs with at least 128 output and 256 contraction columns (the 128 -> 512 ->
 * 1024 -> 1024 period convolutions: forward, dX, dW) and the 32 -> 32-channel band convolutions of the spectrogram discriminators (forward, dX, dW) round
 * their operands to bf16 (nearest even) while staging them and accumulate in fp32 on the bf16 MFMA;
 * feature maps, parameters, gradients and every other kernel stay fp32.
 * 2 (round 5; the default of the Python host's Discriminator): the same wide implicit GEMMs (forward, dX, dW of the period convolutions) on the bf16 MFMA with BOTH
 * operands split exactly into three bf16 terms (a = a1 + a2 + a3) and the six leading cross products accumulated in fp32, smallest first - fp32-grade results
 * (within fp32 summation-order noise of mode 0; the truncated terms are below 2^-26 relative); the band convolutions stay on the fp32 MFMA.
 * Returns ESCX_ERR_INVALID_ARG for another mode. */
int escx_disc_set_precision(escx_disc d, int mode);
int escx_disc_get_precision(escx_disc d);
/* One GAN loss term over a feature-map buffer (gan_loss.py:30-51): loss_dev[b] (+)= mean over the C x D0 x D1 real elements of
 * (target - x)^2 (mode 0) or |x - ref| (mode 1); grad_dev (optional, layout of x) receives d term_b / d x. */
int escx_gan_term(const float* x_dev, const float* ref_dev, float* grad_dev, int batch, int C, int Cp, int D0, int D1, int P1, int mode, float target,
                  float* loss_dev, int accumulate, void* stream);
/* Backward of escx_gan_term with the upstream per-clip gradient folded in (what autograd does with `loss.mean().backward()` in trainer_adv.py:77-105):
 * grad_dev (layout of x) = g_dev[b] * d term_b / d x.  The forward keeps no per-map gradient buffer; x (and ref) are re-read here. */
int escx_gan_term_grad(const float* x_dev, const float* ref_dev, const float* g_dev, float* grad_dev, int batch, int C, int Cp, int D0, int D1, int P1, int mode,
                       float target, void* stream);
/* Per-layer timing of the discriminator's convolutions (diagnostic: HIP events and a stream sync around every launch group while enabled, so the step
 * itself runs slower).  escx_disc_profile_enable(1) clears and starts, (0) stops; the report is a JSON array of {"name": "D.<fwd|dX|dW>[<layer>]",
 * "calls", "ms", "flops"} - the same record format as escx_profile_report.  Process-wide (not per handle). */
int escx_disc_profile_enable(int enable);
const char* escx_disc_profile_report(void);

/* ---- multi-GPU: the one exchange step of the sharded path (BASELINE configs[3]; SURVEY.md 8(b),(e)) ------------- */
/* The reference has no inference-time collective (clips are independent end to end); batch shards exchange only the emitted codes.
 * codes_local_dev: n_local_codes int64 values of this rank (e.g. 36*S*G*T); codes_all_dev: world_size * n_local_codes, rank order.
 * The codes cross xGMI as int16 (RCCL byte payload).  nccl_comm is the caller's ncclComm_t; libescx resolves RCCL at run time
 * (dlopen of "librccl.so.1": in a PyTorch process torch's bundled copy, already mapped) so that communicator and collective come
 * from one RCCL instance; escx_set_rccl_library(path) overrides the name before the first call.  Asynchronous on `stream`, except
 * that growing the int16 staging buffer synchronises (first call / larger shard).  Equal shard sizes on every rank. */
int escx_set_rccl_library(const char* path);
int escx_allgather_codes(escx_handle h, const int64_t* codes_local_dev, int64_t n_local_codes, int64_t* codes_all_dev,
                         int world_size, void* nccl_comm, void* stream);

/* ---- DAC baseline codec (Descript audio codec), inference only ---------------------------------------------------------------------------
 * Reference: baselines/descript/dac/model/dac.py:148-247 (DAC), nn/layers.py:9-33 (WNConv1d, WNConvTranspose1d, Snake1d), nn/quantize.py:13-220
 * (VectorQuantize, ResidualVectorQuantize).  Parameters: one caller-owned flat fp32 device buffer in the order escx_dac_param_*() reports (the
 * reference's named_parameters(): per convolution bias, weight_g, weight_v; per Snake alpha; per codebook weight).  Weight normalisation (the
 * transposed convolutions normalise over their INPUT channels, dim 0), the Snake reciprocals and the normalised codebooks are re-derived on the
 * device when (buffer, params_version) changes; a negative version always re-derives.  Tensors are the reference's layouts: audio (B, 1, L),
 * z (B, D, T), codes (B, n, T) int64, latents (B, n * codebook_dim, T).  Arithmetic is fp32 (escx_dac_set_precision offers an exact split-operand form).  A configuration the kernels do not cover
 * (rates above 16, latent_dim above 1024 or not a multiple of 4, codebook_dim above 8, decoder_dim not divisible by 2^n_decoder_rates)
 * fails at create with ESCX_ERR_UNSUPPORTED. */
#define ESCX_DAC_MAX_RATES 8
typedef struct {
    int32_t encoder_dim; int32_t n_encoder_rates; int32_t encoder_rates[ESCX_DAC_MAX_RATES];
    int32_t latent_dim;             /* 0: encoder_dim * 2^n_encoder_rates (dac.py:173-174) */
    int32_t decoder_dim; int32_t n_decoder_rates; int32_t decoder_rates[ESCX_DAC_MAX_RATES];
    int32_t n_codebooks; int32_t codebook_size; int32_t codebook_dim;
    int32_t sample_rate;
} escx_dac_config;
typedef struct escx_dac_s* escx_dac;
/* DAC.__init__ (dac.py:149-196) */
int escx_dac_create(const escx_dac_config* cfg, int device, escx_dac* out);
void escx_dac_destroy(escx_dac d);
int escx_dac_param_count(escx_dac d);
const char* escx_dac_param_key(escx_dac d, int i);
int64_t escx_dac_param_offset(escx_dac d, int i);
int64_t escx_dac_param_numel(escx_dac d, int i);
int64_t escx_dac_param_total(escx_dac d);
/* Latent frames of an n_samples clip through the encoder (torch's Conv1d length formula; 0 = the clip gives none), and samples decoded from
 * n_frames frames (ConvTranspose1d's (T - 1) s - 2 p + 2 s per block: 320 T - 8 for rates [8, 5, 4, 2]). */
int escx_dac_num_frames(escx_dac d, int n_samples);
int escx_dac_output_samples(escx_dac d, int n_frames);
/* DAC.encode (dac.py:209-247) with ResidualVectorQuantize.forward in eval mode (quantize.py:127-198): audio (B, L) device -> z (B, D, T),
 * codes (B, n, T), latents (B, n * codebook_dim, T), losses[2] = (commitment_loss, codebook_loss) on the device.  n = min(n_quantizers,
 * n_codebooks); n_quantizers < 1 is ESCX_ERR_INVALID_ARG.  The quantiser is one launch. */
int escx_dac_encode(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* audio_dev, int batch, int n_samples, int n_quantizers,
                    float* z_dev, int64_t* codes_dev, float* latents_dev, float* losses_dev, void* stream);
/* escx_dac_encode with one of two optional HOST arrays (both NULL: escx_dac_encode itself, the same bits; both given: ESCX_ERR_INVALID_ARG).  They
 * are copied to a handle-owned device buffer on the call's stream.
 *   clip_n[batch]    per-clip stage counts, the per-item mask the reference's quantiser applies for quantiser dropout (quantize.py:181-190): clip b
 *                    runs codebooks i < clip_n[b].  Each entry lies in [1, n_codebooks]; n_quantizers is then the number of code slots per clip and
 *                    must lie in [max(clip_n), n_codebooks].  codes (B, n_quantizers, T) hold -1 and latents (B, n_quantizers * codebook_dim, T) hold
 *                    0 in the slots at or past a clip's count; losses are sum_i mean_b(loss_ib * [i < clip_n[b]]) (quantize.py:189-190).  z, codes
 *                    and latents of clip b up to its count are bitwise those of a call with n_quantizers = clip_n[b] (one wave per latent row).
 *   snap_n[n_snaps]  strictly increasing stage counts in [1, min(n_quantizers, n_codebooks)]: zsnap (n_snaps, B, D, T) receives the running sum z_q
 *                    (quantize.py:185) after snap_n[r] codebooks, bitwise the z of a call with n_quantizers = snap_n[r].  Both codecs' codes are
 *                    prefix codes, so one encode serves every bitrate of an evaluation sweep.  zsnap_dev is ignored without snap_n.
 * A bad count (0, above n_codebooks, above n_quantizers, snapshots not increasing) is ESCX_ERR_INVALID_ARG and leaves the handle usable. */
int escx_dac_encode_ex(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* audio_dev, int batch, int n_samples, int n_quantizers,
                       const int32_t* clip_n, const int32_t* snap_n, int n_snaps, float* z_dev, int64_t* codes_dev, float* latents_dev, float* losses_dev,
                       float* zsnap_dev, void* stream);
/* ResidualVectorQuantize.from_codes (quantize.py:200-220): codes (B, n, T) -> z_q (B, D, T) and z_p (B, n * codebook_dim, T).  The kernel clamps
 * a code outside [0, codebook_size) to the nearest valid row instead of reading outside the codebook; the reference's F.embedding raises there,
 * and the Python host (esc.baselines.DAC) checks the range and raises IndexError before calling. */
int escx_dac_from_codes(escx_dac d, const float* flat_params_dev, int64_t params_version, const int64_t* codes_dev, int batch, int n_codes, int n_frames,
                        float* z_dev, float* zp_dev, void* stream);
/* escx_dac_from_codes (quantize.py:200-220) with optional per-clip counts clip_n[batch] (HOST array, each in [1, min(n_codes, n_codebooks)]; NULL:
 * escx_dac_from_codes itself): clip b sums the codebooks i < clip_n[b], the slots past its count are never read whatever they hold, and z_p is 0
 * there - the inverse of escx_dac_encode_ex's per-clip form (quantize.py:181-185). */
int escx_dac_from_codes_ex(escx_dac d, const float* flat_params_dev, int64_t params_version, const int64_t* codes_dev, int batch, int n_codes, int n_frames,
                           const int32_t* clip_n, float* z_dev, float* zp_dev, void* stream);
/* DAC.decode (dac.py:249-266): z (B, D, T) -> audio (B, escx_dac_output_samples(T)). */
int escx_dac_decode(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, int batch, int n_frames, float* audio_dev, void* stream);
/* ---- Mixed-length batches: per-clip lengths (dac.py:209-323; padding on) -------------------------------------------------
 * The three entry points below take one length per clip as a HOST int32 array, copied with the tables derived from it (conv_out_len per clip and
 * resolution level) to a handle-owned device buffer on the call's stream.  Clip b's results are bitwise those of the uniform entry point on that
 * clip alone, in fp32 and in bf16x3; nothing at or past a clip's length is read, whatever it holds; everything at or past a clip's length in an
 * output is a fixed filler (0, codes -1).  A null array, batch < 1, an entry outside its range, a clip that gives no frame or no sample (the
 * message names the clip) and a handle with the padding off are ESCX_ERR_INVALID_ARG before anything is launched, and leave the handle usable. */
/* DAC.encode (dac.py:209-247) of audio (B, row_samples) with lengths[b] in [1, row_samples] samples of clip b.  Each clip is first right-padded with
 * zeros to a multiple of pad_multiple (1: as it is; the hop: DAC.preprocess, dac.py:198-207) - staged, not read: the audio tensor need not hold
 * those samples.  With Lp_b that padded length, T_b = escx_dac_num_frames(Lp_b) and Tmax = escx_dac_num_frames(max_b Lp_b), the outputs are those
 * of escx_dac_encode_ex at n_frames = Tmax: z (B, D, Tmax), codes (B, n_quantizers, Tmax), latents (B, n_quantizers * codebook_dim, Tmax), with z
 * and latents 0 and codes -1 at frames >= T_b.  losses[0..1] = sum_i mean_b([i < clip_n[b]] * loss_ib), loss_ib the mean over clip b's own T_b
 * frames: the mean over the clips of the single-clip calls' losses (quantize.py:189-190).  clip_n (HOST array or NULL) is escx_dac_encode_ex's. */
int escx_dac_encode_lengths(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* audio_dev, int batch, int row_samples,
                            const int32_t* lengths, int pad_multiple, int n_quantizers, const int32_t* clip_n, float* z_dev, int64_t* codes_dev,
                            float* latents_dev, float* losses_dev, void* stream);
/* ResidualVectorQuantize.from_codes (quantize.py:200-220) of codes (B, n_codes, n_frames) with frame_lengths[b] in [1, n_frames] frames of clip b:
 * the slots at frames >= frame_lengths[b] are never read, whatever they hold (escx_dac_encode_lengths writes -1 there), and z_q and z_p are 0 there.
 * clip_n (HOST array or NULL) is escx_dac_from_codes_ex's. */
int escx_dac_from_codes_lengths(escx_dac d, const float* flat_params_dev, int64_t params_version, const int64_t* codes_dev, int batch, int n_codes, int n_frames,
                                const int32_t* frame_lengths, const int32_t* clip_n, float* z_dev, float* zp_dev, void* stream);
/* DAC.decode (dac.py:249-266) of z (B, D, n_frames) with frame_lengths[b] in [1, n_frames] frames of clip b: audio (B, escx_dac_output_samples(n_frames)),
 * clip b bitwise escx_dac_decode of its own frame_lengths[b] frames and 0 from sample escx_dac_output_samples(frame_lengths[b]) on.  sample_caps (HOST
 * array or NULL) cuts clip b's audio at min(that, sample_caps[b]) samples, 0 from there on: the trim to the input length of DAC.forward (dac.py:316). */
int escx_dac_decode_lengths(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, int batch, int n_frames,
                            const int32_t* frame_lengths, const int32_t* sample_caps, float* audio_dev, void* stream);
/* Where Snake (nn/layers.py:19-24) is evaluated, per layer class: bit set = written once per element into a Snaked copy of the map that the
 * convolution then reads; bit clear = applied to the operand while the convolution stages it (once per tap and per output-column tile).  Both
 * give bitwise the same results; the default is the faster per class on MI355X.  A/B switch, not a numerics setting. */
#define ESCX_DAC_SNAKE_RES7 0       /* ResidualUnit's dilated 7-tap convolution (input x)            */
#define ESCX_DAC_SNAKE_RES1 1       /* ResidualUnit's 1x1 convolution (input: the 7-tap output)      */
#define ESCX_DAC_SNAKE_DOWN 2       /* EncoderBlock's strided convolution                           */
#define ESCX_DAC_SNAKE_UP 3         /* DecoderBlock's transposed convolution (every phase GEMM)     */
#define ESCX_DAC_SNAKE_LAST 4       /* the encoder's last 3-tap and the decoder's last 7-tap layer  */
#define ESCX_DAC_SNAKE_ALL 31
#define ESCX_DAC_SNAKE_MAPS_DEFAULT ESCX_DAC_SNAKE_ALL   /* measured faster for every class: profiles/dac_snake_ab.txt */
int escx_dac_set_snake_maps(escx_dac d, int mask);
int escx_dac_get_snake_maps(escx_dac d);
/* Arithmetic of the convolutions of encode / decode, per handle, read at each call; the modes carry escx_set_precision's numbers:
 *   ESCX_PRECISION_FP32    (default) every convolution on v_mfma_f32_16x16x4_f32 with fp32 operands; bitwise what the library computed before this switch existed.
 *   ESCX_PRECISION_BF16X3  every fp32 operand (packed weight-normalised weights, feature maps after Snake) split EXACTLY into three bf16 terms, six cross
 *                          products accumulated in fp32 on v_mfma_f32_16x16x32_bf16: fp32-grade results that differ from ESCX_PRECISION_FP32 by summation
 *                          order and the three dropped cross terms (below 2^-24 relative).  The one-channel first and last convolutions stay on the fp32
 *                          MFMA and the quantiser on the fp32 VALU (the rule is on the layer geometry, never on the batch).
 *   ESCX_PRECISION_F16X2   ESCX_ERR_UNSUPPORTED: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) and Snake outputs have none.
 * Any other value is ESCX_ERR_INVALID_ARG.  In both modes a clip's codes and audio do not depend on the batch, and both Snake placements give the same bits.
 * The three-term weight image is rebuilt whenever the packed fp32 weights are (params_version, buffer) and when the mode is first switched on. */
int escx_dac_set_precision(escx_dac d, int mode);
int escx_dac_get_precision(escx_dac d);
/* Arithmetic of the backward entry points (escx_dac_decode_backward, escx_dac_decode_backward_params, escx_dac_encode_backward), per handle and
 * independent of escx_dac_set_precision: all four combinations of forward and backward mode are legal.  The mode is read when a backward entry point
 * is called, not when the tape was made: a tape is valid under either mode.  escx_set_precision's numbers:
 *   ESCX_PRECISION_FP32    (default) every contraction of the backward on v_mfma_f32_16x16x4_f32; bitwise what the library computed before this switch existed.
 *   ESCX_PRECISION_BF16X3  the input gradient (dX) of every convolution of the decoder and of the encoder - the stride-1 layers, the ConvTranspose1d's
 *                          strided form and the strided Conv1d's two-tap GEMM per input phase - on v_mfma_f32_16x16x32_bf16: the output gradient and the
 *                          transposed weight image each split EXACTLY into three bf16 terms, six cross products accumulated in fp32 in two levels (the MFMA
 *                          chain restarts every 1, 2, 4 or 8 steps of 32, by the layer's K alone, and the chunk sums are added in order, with alternating signs so that a
 *                          one-sided rounding of the matrix core's accumulation cancels: DESIGN.md section 13.3).  The weight terms
 *                          come from a three-plane bf16 mirror of the transposed images, allocated at the first backward of the handle in this mode and
 *                          rebuilt on the call's stream whenever the transposed images are (a parameter change).  As in the forward mode the one-channel
 *                          first and last convolutions stay on the fp32 MFMA.  NOT covered, the same in both modes: the weight gradients (dW) of
 *                          escx_dac_decode_backward_params (a switch of their own: escx_dac_set_param_grad_precision) with their bias / alpha /
 *                          weight-norm reductions, and the quantiser's backward.
 *   ESCX_PRECISION_F16X2   ESCX_ERR_UNSUPPORTED: two fp16 terms need an a-priori bound on every operand and neither output gradients nor Snake outputs have one.
 * Any other value is ESCX_ERR_INVALID_ARG; a refusal leaves the mode as it was.  Forward results never depend on this mode.  In both modes the backward
 * has no atomics, two calls are bitwise equal, a clip's gradient does not depend on its batch, and a zero cotangent gives an exactly zero gradient. */
int escx_dac_set_grad_precision(escx_dac d, int mode);
int escx_dac_get_grad_precision(escx_dac d);
/* CodecMixin.padding (base.py:58-80), per handle, read at each call; on by default.  Off: every Conv1d and ConvTranspose1d runs with padding 0, as
 * the reference's chunked compress / decompress do (base.py:194-201, 259-260): a Conv1d gives floor((T - dilation (K - 1) - 1) / stride) + 1 rows, a
 * ConvTranspose1d (T + 1) * stride, and a ResidualUnit adds its input cropped by 3 * dilation rows on each side (dac.py:35-40).  escx_dac_num_frames,
 * escx_dac_output_samples, escx_dac_encode, escx_dac_encode_ex and escx_dac_decode honour the mode; a length that leaves any layer without a row is
 * ESCX_ERR_INVALID_ARG before anything is launched.  With the padding on, every call computes bitwise what it did before this switch existed.  The
 * packed transposed-convolution weights depend on the mode: the first call after a change re-derives the packed operands.  `on` is 0 or 1. */
int escx_dac_set_padding(escx_dac d, int on);
int escx_dac_get_padding(escx_dac d);
/* CodecMixin.get_delay (base.py:82-106): (l_in - l_out) / 2 of the whole model's receptive field, whatever the padding mode; -1 for a null handle. */
int escx_dac_delay(escx_dac d);
/* CodecMixin.get_output_length (base.py:108-123): samples out of encoder + decoder for n_samples in, every convolution without padding, floored at
 * every layer, whatever the padding mode.  The reference evaluates it at 0 too, so the result may be negative. */
int escx_dac_output_length(escx_dac d, int n_samples);
/* One pass of CodecMixin.compress's chunked loop (base.py:197, 203-214) as one batch: escx_dac_encode_ex (no per-clip counts, no snapshots) on
 * B = rows * n_chunks windows of L = n_samples that are never materialised on the host.  Window c of signal row r (batch index r * n_chunks + c) holds
 * signal[r][c * hop + j - lead] at sample j and 0 where that index falls outside [0, n_signal): with lead = escx_dac_delay this is the reference's
 * zero_pad(delay, delay), its slice [c * hop, c * hop + n_samples) and the right zero-pad of a short last slice.  A pass that starts at chunk c0 passes
 * lead = delay - c0 * hop.  signal_dev is (rows, n_signal) fp32; the outputs are escx_dac_encode's for that batch.  The padding mode is the handle's
 * (the reference switches it off for this loop). */
int escx_dac_encode_chunks(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* signal_dev, int rows, int64_t n_signal, int n_chunks,
                           int n_samples, int hop, int64_t lead, int n_quantizers, float* z_dev, int64_t* codes_dev, float* latents_dev, float* losses_dev,
                           void* stream);
/* ---- Latent gradient through the decoder (eval mode, padding on) -------------------------------------------------------------------------------
 * d audio / d z of DAC.decode (baselines/descript/dac/model/dac.py:249-266) for a frozen codec inside a larger autograd graph: the decoder is
 * Decoder.forward (dac.py:115-145) over DecoderBlock (dac.py:94-112: Snake1d, WNConvTranspose1d, three ResidualUnits) and ResidualUnit
 * (dac.py:24-41: x + conv1(snake(conv7(snake(x))))), with Snake1d and the weight-normalised layers of nn/layers.py:9-33.  The encoder and the quantiser are not
 * differentiated here; the decoder's parameter gradients are escx_dac_decode_backward_params below.  With the handle's padding off every entry point below returns ESCX_ERR_UNSUPPORTED (the
 * chunked path needs no gradients).  DESIGN.md section 13.3 has the launch sequence and the tape layout. */
/* Floats of the activation tape of one padded decode of batch x n_frames (dac.py:249-266): a 64-float header, the input of every convolution
 * that follows a Snake (each DecoderBlock's ConvTranspose input, each ResidualUnit's x and h, dac.py:24-41, 94-112) as channels-last maps, and
 * the audio.  0 when the geometry decodes to nothing or an argument is bad; ESCX_ERR_UNSUPPORTED with the padding off. */
int64_t escx_dac_decode_tape_floats(escx_dac d, int batch, int n_frames);
/* DAC.decode (dac.py:249-266) with the maps a backward needs kept: the launch sequence of escx_dac_decode - same kernels, operands and order, in
 * fp32 and in bf16x3 - with those maps written to the caller's tape_dev (tape_floats = escx_dac_decode_tape_floats, 16-byte aligned) instead of
 * the handle's reused scratch; a ResidualUnit (dac.py:35-41) writes its sum to the next map instead of back into x.  audio_dev is bitwise what
 * escx_dac_decode returns.  The tape lives in caller memory and records (params_version, batch, n_frames): any number of tapes may be alive at
 * once and the handle keeps no per-graph state. */
int escx_dac_decode_tape(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, int batch, int n_frames, float* audio_dev,
                         float* tape_dev, int64_t tape_floats, void* stream);
/* d_z (B, D, T) = (d audio / d z)^T d_audio for the decode that wrote tape_dev (dac.py:249-266 differentiated; d_audio_dev is (B, samples)):
 * tanh (dac.py:138), then per layer in reverse the transposed convolution of the output gradient times the derivative of the Snake in front of
 * it (nn/layers.py:19-33), the ResidualUnit as g + conv7^T(conv1^T(g) snake'(h)) snake'(x) (dac.py:24-41), the ConvTranspose1d (dac.py:99-105) as
 * one strided convolution.  fp32 MFMA or, under escx_dac_set_grad_precision(ESCX_PRECISION_BF16X3), the split-operand form, whatever the forward's
 * mode; on transposed images of the packed forward weights (derived at the first backward of a handle and after every parameter change).  No atomics: bitwise deterministic, and a clip's d_z does not depend on its batch.
 * params_version must be the version the tape was made with: another one is ESCX_ERR_STATE with a message that says so, and a buffer that is not
 * a tape for (batch, n_frames) is ESCX_ERR_INVALID_ARG; both are found before the handle changes.  The check reads the tape's header back, so the
 * call waits for the stream once. */
int escx_dac_decode_backward(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* tape_dev, int64_t tape_floats,
                             const float* d_audio_dev, int batch, int n_frames, float* d_z_dev, void* stream);
/* ---- Parameter gradients through the decoder (eval mode, padding on) ---------------------------------------------------------------------------
 * The gradient of every decoder parameter of DAC.decode (baselines/descript/dac/model/dac.py:249-266) for the decode that wrote tape_dev, for
 * fine-tuning a decoder on frozen codes or latents: Decoder.forward (dac.py:115-145) over DecoderBlock (dac.py:94-112) and ResidualUnit
 * (dac.py:24-41) differentiated with respect to the weight-normalised layers' bias, weight_g and weight_v (nn/layers.py:5-16) and every Snake1d's
 * alpha (nn/layers.py:19-33).  It walks escx_dac_decode_backward's layers in its order; at each layer, with dY its output gradient and s its forward
 * operand (the Snaked saved map, zero outside; z for the first convolution):
 *   Conv1d            dW[co][ci][k] = sum_{b,t} dY(b, t, co) s(b, t - p + k d, ci),   db[co] = sum_{b,t} dY(b, t, co)
 *   ConvTranspose1d   dW[ci][co][k] = sum_{b,t} s(b, t, ci) dY(b, t st - p + k, co),  db likewise
 *   Snake1d           d_alpha[c] = sum_{b,t} v(b, t, c) (x sin(2 alpha x) / (alpha + 1e-9) - sin(alpha x)^2 / (alpha + 1e-9)^2),  v = conv^T(dY)
 *   weight norm       dg = <dW, v> / |v|,  dv = g / |v| (dW - <dW, v> v / |v|^2), the norm over all dimensions but the first
 * grad_flat_dev has flat_params_dev's layout (escx_dac_param_offset): the slots of every `decoder.*` parameter are OVERWRITTEN and no other float
 * is touched.  z_dev (B, D, T) is the latent the tape was made from (the tape does not hold it).  d_z_dev may be NULL; when given it is bitwise
 * what escx_dac_decode_backward writes in the same grad mode.  The weight-gradient contractions are fp32 MFMA over row slices whose partial tiles are
 * added in increasing slice order (no atomics: two calls are bitwise equal), in both precision modes and both grad modes (escx_dac_set_grad_precision
 * moves the input gradients that feed them, not the dW contraction), or the split-operand form under escx_dac_set_param_grad_precision; the slices'
 * tiles live in a handle workspace allocated at the first call (escx_dac_param_grad_workspace_floats).  Errors are escx_dac_decode_backward's and are found before the handle changes: padding off is
 * ESCX_ERR_UNSUPPORTED, a foreign or wrong-size tape ESCX_ERR_INVALID_ARG, another params_version ESCX_ERR_STATE with a message naming both, a
 * NULL grad_flat_dev or z_dev ESCX_ERR_INVALID_ARG.  DESIGN.md section 13.5 has the launch sequence, the workspace and the slice rule. */
int escx_dac_decode_backward_params(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* tape_dev, int64_t tape_floats,
                                    const float* z_dev, const float* d_audio_dev, int batch, int n_frames, float* d_z_dev, float* grad_flat_dev, void* stream);
/* Floats of the handle workspace escx_dac_decode_backward_params allocates at its first call; it depends on the configuration alone.  Under
 * escx_dac_set_param_grad_precision(ESCX_PRECISION_BF16X3) the 128 x 128 tiles' partial region, which is a second allocation made at the first
 * parameter backward in that mode and sized from the configuration alone, is counted from that backward on; in fp32 mode never. */
int64_t escx_dac_param_grad_workspace_floats(escx_dac d);
/* Row slices of the weight-gradient contraction of decoder convolution `layer` (execution order, from 0) for batch x n_frames under the current
 * escx_dac_set_param_grad_precision mode (a layer that stays on the fp32 kernel reports the fp32 rule's count in both); 0 on a bad argument. */
int escx_dac_param_grad_slices(escx_dac d, int batch, int n_frames, int layer);
/* Operand form of the weight-gradient (dW) contractions of escx_dac_decode_backward_params (dac.py:24-41, 94-145, 249-266 and nn/layers.py:5-33
 * differentiated), per handle, independent of escx_dac_set_precision and escx_dac_set_grad_precision and read when the backward runs.
 *   ESCX_PRECISION_FP32    (default) gemm_dw_kernel on v_mfma_f32_16x16x4_f32 with 48 x 48 tiles: bitwise what the library computed before this switch
 *                          existed, with the same slices, workspace, launches and allocation time.
 *   ESCX_PRECISION_BF16X3  the dW contraction of every decoder convolution with more than one input and more than one output channel on
 *                          v_mfma_f32_16x16x32_bf16 with 128 x 128 tiles of dW (64 x 128 and 32 x 128 where Np <= 64 and Np <= 32): both operands - a Conv1d's output-gradient rows and the im2col rows
 *                          of its Snaked input, a ConvTranspose1d's Snaked input rows and the strided rows of its output gradient - split EXACTLY into
 *                          three bf16 terms while they are staged, the six leading cross products accumulated in fp32, the row slices (multiples of
 *                          32 rows, at least 256 where the contraction has them, counted from the geometry alone) added in increasing order.  The
 *                          one-channel last convolution stays on the fp32 kernel.  dW keeps its layout, so the weight norm's backward and the bias /
 *                          alpha column sums (fp64 partials) are the same launches in both modes; d_z and the audio do not depend on the mode.
 *   ESCX_PRECISION_F16X2   ESCX_ERR_UNSUPPORTED: two fp16 terms need an a-priori bound on every operand and neither output gradients nor Snake outputs have one.
 * Any other value is ESCX_ERR_INVALID_ARG; a refusal leaves the mode as it was.  In both modes there are no atomics, two calls are bitwise equal and a
 * gradient that is exactly zero in fp32 mode (a pad channel, a parameter whose output gradient is zero) is exactly zero.  DESIGN.md section 13.5. */
int escx_dac_set_param_grad_precision(escx_dac d, int mode);
int escx_dac_get_param_grad_precision(escx_dac d);
/* ---- Audio gradient through the encoder and the quantiser (eval mode, padding on) ---------------------------------------------------------------
 * d (z, latents, commitment_loss) / d audio of DAC.encode (baselines/descript/dac/model/dac.py:209-247) for a frozen codec in the middle of a larger
 * autograd graph: Encoder.forward (dac.py:64-91) over EncoderBlock (dac.py:44-61: three ResidualUnits, Snake1d, strided WNConv1d) and
 * ResidualVectorQuantize.forward in eval mode (nn/quantize.py:173-198) with VectorQuantize's straight-through estimator and detached codebook
 * vector (nn/quantize.py:58-70).  The codebook loss detaches z_e and the codes are integers: neither has an audio gradient.  Parameter gradients,
 * training mode and quantiser dropout are not differentiated.  With the handle's padding off every entry point below returns
 * ESCX_ERR_UNSUPPORTED.  DESIGN.md section 13.4 has the launch sequence and the tape layout. */
/* Floats of the activation tape of one padded encode of batch x n_samples with min(n_quantizers, n_codebooks) stages (dac.py:209-247): a 64-float
 * header, the input of every convolution that follows a Snake (each ResidualUnit's x and h, dac.py:24-41; the input of each EncoderBlock's last
 * Snake, dac.py:55-58; the input of the encoder's last Snake, dac.py:82-85) as channels-last maps, then latents, codes and the per-clip stage counts
 * (quantize.py:173-198).  0 when the clip gives no frame or an argument is bad; ESCX_ERR_UNSUPPORTED with the padding off. */
int64_t escx_dac_encode_tape_floats(escx_dac d, int batch, int n_samples, int n_quantizers);
/* DAC.encode (dac.py:209-247) with what a backward needs kept: the launch sequence of escx_dac_encode_ex - same kernels, operands and order, in fp32
 * and in bf16x3 - with the encoder's maps written to the caller's tape_dev (tape_floats = escx_dac_encode_tape_floats, 16-byte aligned) instead of
 * the handle's reused scratch, and latents, codes and stage counts copied behind them.  clip_n (HOST array or NULL) is escx_dac_encode_ex's; there
 * are no snapshots.  z, codes, latents and losses are bitwise those of escx_dac_encode / escx_dac_encode_ex.  The tape lives in caller memory and
 * records (params_version, batch, n_samples, stages): any number of tapes may be alive at once and the handle keeps no per-graph state. */
int escx_dac_encode_tape(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* audio_dev, int batch, int n_samples, int n_quantizers,
                         const int32_t* clip_n, float* z_dev, int64_t* codes_dev, float* latents_dev, float* losses_dev, float* tape_dev, int64_t tape_floats,
                         void* stream);
/* d_audio (B, n_samples) = the cotangents d_z (B, D, T), d_latents (B, n * codebook_dim, T) and the DEVICE scalar d_commitment pulled back through the
 * encode that wrote tape_dev; each may be NULL (zero).  The quantiser (quantize.py:173-198 differentiated, one launch): per latent row and stage in
 * reverse, u = d_z - g_r, e = W_out^T u + d_latents_i + d_commitment * 2 (z_e_i - codebook_i[code]) / (batch * codebook_dim * T) (quantize.py:61, 64-68,
 * 189), g_r += W_in^T e (quantize.py:58, 186); a clip with its own stage count runs that many stages.  Then the encoder (dac.py:64-91 differentiated)
 * in reverse: per layer the transposed convolution of the output gradient times the derivative of the Snake in front of it (nn/layers.py:19-33), the
 * ResidualUnit as g + conv7^T(conv1^T(g) snake'(h)) snake'(x) (dac.py:24-41), the strided convolution (dac.py:55-58) as one two-tap GEMM per input
 * phase, every input row written.  fp32 MFMA, or the split-operand form under escx_dac_set_grad_precision(ESCX_PRECISION_BF16X3) (the quantiser's
 * backward is fp32 VALU in both), whatever the forward's mode; no atomics: bitwise deterministic, and without d_commitment a clip's d_audio
 * does not depend on its batch.  params_version must be the tape's: another one is ESCX_ERR_STATE with a message naming both; a buffer that is not
 * an encode tape for (batch, n_samples), a decode tape included, or has the wrong size is ESCX_ERR_INVALID_ARG; both are found before the handle
 * changes.  The check reads the tape's header back, so the call waits for the stream once. */
int escx_dac_encode_backward(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* tape_dev, int64_t tape_floats, const float* d_z_dev,
                             const float* d_latents_dev, const float* d_commitment_dev, int batch, int n_samples, float* d_audio_dev, void* stream);
/* ---- Parameter gradients through the encoder and the quantiser (eval mode, padding on) ----------------------------------------------------------
 * The gradient of every encoder parameter (bit 0 of `parts`) and every quantiser parameter (bit 1) of DAC.encode (dac.py:209-247) for the encode
 * that wrote tape_dev, for fine-tuning the whole baseline: Encoder.forward (dac.py:64-91) over EncoderBlock (dac.py:44-61) and ResidualUnit
 * (dac.py:24-41), and ResidualVectorQuantize.forward in eval mode (nn/quantize.py:173-198) over VectorQuantize.forward (nn/quantize.py:58-70),
 * differentiated with respect to the weight-normalised layers' bias, weight_g and weight_v (nn/layers.py:5-16), every Snake1d's alpha
 * (nn/layers.py:19-33) and the codebooks.  The cotangents are escx_dac_encode_backward's d_z, d_latents and d_commitment plus the DEVICE scalar
 * d_codebook on the codebook loss; each may be NULL (zero).
 * Quantiser, per latent row (b, t) and stage i < n_b in reverse, with r_0 = z_enc, z_e_i = W_in_i r_i + b_in_i, q_i = C_i[code_i],
 * r_{i+1} = r_i - (W_out_i q_i + b_out_i), u_i the cotangent of z_q_i and e_i the cotangent of z_e_i as escx_dac_encode_backward forms them:
 *   dW_out_i = sum_rows u_i q_i^T        db_out_i = sum_rows u_i                                  (quantize.py:58, 69)
 *   dW_in_i  = sum_rows e_i r_i^T        db_in_i  = sum_rows e_i                                  (quantize.py:58, 186)
 *   dC_i[c]  = d_codebook * 2 / (batch * codebook_dim * T) * sum_{rows with code_i = c, i < n_b} (q_i - z_e_i)      (quantize.py:62, 66, 189)
 * then the weight norm's backward on both projections (nn/layers.py:5-10, K = 1).  u_i and r_i are formed per row, one launch per stage, never as
 * differences of sums over rows; a code's rows are added in increasing row order and a code no row chose gets exactly zero.  The quantiser's
 * kernels are fp32 in every mode.  z_e_i is the tape's latents; z_enc, which the tape does not hold, is the encoder's last convolution run again
 * from the last taped map (one layer, the forward's launch in the forward's current escx_dac_set_precision mode); audio_dev (B, n_samples) is the
 * audio the tape was made from (the tape does not hold it either).
 * Encoder: escx_dac_encode_backward's walk in its order with its maps; at each layer escx_dac_decode_backward_params' formulas for Conv1d (the strided
 * convolution reads s(b, t st - p + k, ci)), Snake1d (v = conv^T(dY) kept by the per-phase GEMMs too) and the weight norm; the first convolution
 * contracts against the staged audio.  escx_dac_set_grad_precision and escx_dac_set_param_grad_precision are honoured by the decoder path's geometry
 * rules; column sums and the weight norm's dot products accumulate in fp64.
 * grad_flat_dev has flat_params_dev's layout: the slots of every `encoder.*` parameter (bit 0) and every `quantizer.*` parameter (bit 1) are
 * OVERWRITTEN - the quantiser stages at or past the tape's stage count with zeros - and no other float is touched.  d_audio_dev may be NULL; when
 * given it is bitwise what escx_dac_encode_backward writes in the same grad mode.  No atomics: two calls are bitwise equal.  Errors are
 * escx_dac_encode_backward's, plus ESCX_ERR_INVALID_ARG for a NULL grad_flat_dev or audio_dev and for parts outside 1..3; all are found before the
 * handle changes.  DESIGN.md section 13.7 has the launch sequence and the workspace. */
int escx_dac_encode_backward_params(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* tape_dev, int64_t tape_floats,
                                    const float* audio_dev, const float* d_z_dev, const float* d_latents_dev, const float* d_commitment_dev,
                                    const float* d_codebook_dev, int batch, int n_samples, int parts, float* d_audio_dev, float* grad_flat_dev, void* stream);
/* Row slices of the weight-gradient contraction of encoder convolution `layer` (execution order, from 0) for batch x n_samples under the current
 * escx_dac_set_param_grad_precision mode, the encoder's analogue of escx_dac_param_grad_slices; 0 on a bad argument or with the padding off.
 * escx_dac_param_grad_workspace_floats counts the encoder's and the quantiser's own workspace (the same three regions, sized over the encoder's
 * layers and the two projections from the configuration alone) from the first escx_dac_encode_backward_params of the handle on, and its
 * split-operand partial region from the first such call in that mode on. */
int escx_dac_encode_param_grad_slices(escx_dac d, int batch, int n_samples, int layer);
/* ---- The stand-alone quantiser: latent in, codes out (eval mode) -----------------------------------------------------------
 * ResidualVectorQuantize.forward on a latent the caller brings (nn/quantize.py:127-198 over VectorQuantize.forward, quantize.py:58-70), the public
 * `model.quantizer(z, n_quantizers)` of the reference: z (B, D, T) device -> z_q (B, D, T), codes (B, n, T), latents (B, n * codebook_dim, T),
 * losses[2] = (commitment_loss, codebook_loss) on the device; n = min(n_quantizers, n_codebooks).  z is staged channels-last as escx_dac_decode stages
 * it and the quantiser and loss launches are escx_dac_encode's, so every value is the one the quantiser inside escx_dac_encode computes from the same
 * map.  The quantiser is fp32 in every precision mode and has no convolution: the result depends on neither escx_dac_set_precision nor
 * escx_dac_set_padding.  ESCX_ERR_INVALID_ARG (null pointer, batch < 1, n_frames < 1, n_quantizers < 1) leaves the handle usable. */
int escx_dac_quantize(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, int batch, int n_frames, int n_quantizers,
                      float* zq_dev, int64_t* codes_dev, float* latents_dev, float* losses_dev, void* stream);
/* escx_dac_quantize with per-clip stage counts clip_n[batch] (HOST array or NULL), the per-item mask of quantize.py:181-190 with the semantics, the
 * fillers (codes -1, latents 0) and the errors of escx_dac_encode_ex's clip_n: n_quantizers is the number of code slots, in [max(clip_n), n_codebooks]. */
int escx_dac_quantize_ex(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, int batch, int n_frames, int n_quantizers,
                         const int32_t* clip_n, float* zq_dev, int64_t* codes_dev, float* latents_dev, float* losses_dev, void* stream);
/* escx_dac_quantize (quantize.py:127-198) of z (B, D, n_frames) with frame_lengths[b] in [1, n_frames] frames of clip b (HOST array), the semantics of
 * escx_dac_decode_lengths on the input and of escx_dac_encode_lengths on the outputs: nothing at or past a clip's length is read, z_q and latents
 * are 0 and codes -1 there, clip b is bitwise escx_dac_quantize of its own frames, and the losses are the mean over the clips of the single-clip
 * calls' losses.  clip_n (HOST array or NULL) is escx_dac_quantize_ex's.  An entry outside its range is ESCX_ERR_INVALID_ARG before any launch. */
int escx_dac_quantize_lengths(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, int batch, int n_frames,
                              const int32_t* frame_lengths, int n_quantizers, const int32_t* clip_n, float* zq_dev, int64_t* codes_dev, float* latents_dev,
                              float* losses_dev, void* stream);
/* d_z (B, D, T) = the cotangents d_zq (B, D, T), d_latents (B, n_codes * codebook_dim, T) and the DEVICE scalar d_commitment pulled back through
 * escx_dac_quantize / _ex (quantize.py:58-70, 173-198 under autograd: the straight-through estimator per stage, quantize.py:64-66, and the commitment
 * term against the detached codebook vector, quantize.py:61); each may be NULL (zero).  The operands are the forward's own outputs latents_dev
 * (B, n_codes * codebook_dim, T) and codes_dev (B, n_codes, T) and its stage counts (clip_n HOST array, or NULL for n_codes everywhere): there is no
 * tape.  One launch of escx_dac_encode_backward's quantiser kernel, then the (B, T, Dp) -> (B, D, T) store.  fp32 VALU, no atomics: bitwise
 * deterministic, and without d_commitment a clip's d_z does not depend on its batch.  The caller answers for params_version being the forward's
 * (esc.baselines.DAC records it and raises).  ESCX_ERR_INVALID_ARG: null latents / codes / d_z, n_codes outside [1, n_codebooks], a bad count. */
int escx_dac_quantize_backward(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* latents_dev, const int64_t* codes_dev, int batch,
                               int n_frames, int n_codes, const int32_t* clip_n, const float* d_zq_dev, const float* d_latents_dev,
                               const float* d_commitment_dev, float* d_z_dev, void* stream);
/* The gradient of every quantiser parameter of escx_dac_quantize / _ex (quantize.py:58-70, 173-198 differentiated with respect to in_proj / out_proj
 * bias, weight_g, weight_v, nn/layers.py:5-10, and the codebooks): the quantiser block of escx_dac_encode_backward_params, the same launches with the
 * same formulas, whose z_enc operand is the staged z_dev (B, D, T) the forward was given.  d_codebook is the DEVICE scalar on the codebook loss (or
 * NULL).  grad_flat_dev has flat_params_dev's layout: the slots of every `quantizer.*` parameter are OVERWRITTEN, the stages at or past n_codes with
 * zeros, and no other float is touched.  d_z_dev may be NULL; when given it is bitwise escx_dac_quantize_backward's.  The workspace is
 * escx_dac_encode_backward_params' (escx_dac_param_grad_workspace_floats counts it from the first call on).  No atomics: two calls are bitwise equal.
 * Errors are escx_dac_quantize_backward's plus ESCX_ERR_INVALID_ARG for a NULL z_dev or grad_flat_dev, found before the handle changes. */
int escx_dac_quantize_backward_params(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* z_dev, const float* latents_dev,
                                      const int64_t* codes_dev, int batch, int n_frames, int n_codes, const int32_t* clip_n, const float* d_zq_dev,
                                      const float* d_latents_dev, const float* d_commitment_dev, const float* d_codebook_dev, float* d_z_dev,
                                      float* grad_flat_dev, void* stream);
/* ResidualVectorQuantize.from_latents (quantize.py:222-255) over VectorQuantize.decode_latents (quantize.py:78-94): per-codebook latents
 * (B, n_channels, T) -> z_q (B, D, T), z_p (B, n * codebook_dim, T) and codes (B, n, T) with n = min(n_channels / codebook_dim, n_codebooks); trailing
 * channels that fill no codebook are ignored and n_channels < codebook_dim is ESCX_ERR_INVALID_ARG.  Every stage searches its own channels
 * independently - one wave per (stage, row) - with the operations of the fused quantiser's search, so the codes are bitwise those escx_dac_quantize
 * emits for the same latents; z_q and z_p are escx_dac_from_codes' launch on those codes.  A latent whose every distance is NaN gets code 0. */
int escx_dac_from_latents(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* latents_dev, int batch, int n_channels, int n_frames,
                          float* z_dev, float* zp_dev, int64_t* codes_dev, void* stream);
/* escx_dac_from_latents (quantize.py:222-255) with per-clip stage counts clip_n[batch] (HOST array or NULL, each in [1, n]): the slots at or past a
 * clip's count are not searched, hold code -1 and z_p 0 and add nothing to z_q, as in escx_dac_from_codes_ex. */
int escx_dac_from_latents_ex(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* latents_dev, int batch, int n_channels, int n_frames,
                             const int32_t* clip_n, float* z_dev, float* zp_dev, int64_t* codes_dev, void* stream);
/* escx_dac_from_latents (quantize.py:222-255) with frame_lengths[b] in [1, n_frames] frames of clip b (HOST array): the rows at or past a clip's
 * length are not read and hold z_q 0, z_p 0 and codes -1, as in escx_dac_from_codes_lengths.  clip_n (HOST array or NULL) is escx_dac_from_latents_ex's. */
int escx_dac_from_latents_lengths(escx_dac d, const float* flat_params_dev, int64_t params_version, const float* latents_dev, int batch, int n_channels,
                                  int n_frames, const int32_t* frame_lengths, const int32_t* clip_n, float* z_dev, float* zp_dev, int64_t* codes_dev,
                                  void* stream);
/* Test hook: the kernels' Snake (mode 0: x + sin(alpha x)^2 / (alpha + 1e-9), nn/layers.py:19-24) or tanh (mode 1) over n device values. */
int escx_dac_test_math(const float* x_dev, const float* alpha_dev, float* out_dev, int64_t n, int mode, void* stream);
/* Test hook of the backward of DAC.decode (dac.py:249-266): the kernels' Snake derivative (mode 0: 1 + alpha sin(2 alpha x) / (alpha + 1e-9), the
 * derivative of nn/layers.py:19-24) or the tanh derivative from the output (mode 1: 1 - y^2 of y = x_dev, dac.py:138) over n device values. */
int escx_dac_test_grad_math(const float* x_dev, const float* alpha_dev, float* out_dev, int64_t n, int mode, void* stream);

/* ---- Training losses of the DAC baseline (baselines/descript/dac/nn/loss.py:11-327) ----------------------------------------
 * MelSpectrogramLoss and MultiScaleSTFTLoss are one handle type.  A scale is a window (hop = window / 4, periodic hann, center = True with reflect
 * padding, as audiotools' STFT) and either a filterbank of n_mels rows over the window / 2 + 1 bins (row-major (n_mels, window / 2 + 1) fp32 HOST data,
 * copied at create: the caller computes it, so fmin / fmax / the mel scale cost nothing here) or n_mels = 0: no filterbank, the STFT loss.  The loss is
 *   sum over scales of  log_weight * mean |log10(clamp(x, clamp_eps)^pow) - log10(clamp(y, clamp_eps)^pow)|  +  mag_weight * mean |x - y|
 * with x / y the (mel) magnitudes of the estimate / the reference and the means over clips, frames and bins (nn.L1Loss).  A zero weight skips its term.
 * The handle owns its DFT and filterbank matrices; several handles may be alive at once and do not see each other.  ESC's own mel loss (HTK filterbanks,
 * per-clip values, one table per device) is a different loss with its own entry points above.
 * Spectra of the scales without a filterbank are accumulated in fp64 (the log term's 1 / |S| amplifies the rounding of near-empty bins).
 * Debugging knob: with ESCX_SPEC_LOSS_F32=1 in the environment when a handle is CREATED, that handle computes those spectra with the fp32 framing GEMM of
 * the filterbank scales instead (values within 2e-7, gradients up to 7.9 times float32 torch eager's error against float64: DESIGN.md 15.1 is measured
 * with it).  Not for training runs. */
#define ESCX_SPEC_LOSS_MAX_SCALES 16
typedef struct {
    int32_t n_scales;                                        /* 1 .. ESCX_SPEC_LOSS_MAX_SCALES                     */
    int32_t window[ESCX_SPEC_LOSS_MAX_SCALES];               /* positive multiples of 4, at most 4096              */
    int32_t n_mels[ESCX_SPEC_LOSS_MAX_SCALES];               /* 0 = no filterbank                                  */
    const float* filterbank[ESCX_SPEC_LOSS_MAX_SCALES];      /* host, (n_mels, window / 2 + 1); ignored for n_mels = 0 */
    float clamp_eps;                                         /* 1e-5                                               */
    float pow;                                               /* 2.0 (the 16 kHz yml: 1.0)                          */
    float mag_weight;                                        /* 1.0 (the 16 kHz yml: 0.0)                          */
    float log_weight;                                        /* 1.0                                                */
} escx_spec_loss_config;
typedef struct escx_spec_loss_s* escx_spec_loss;
/* ESCX_ERR_INVALID_ARG: null pointers, n_scales out of range, a window that is not a positive multiple of 4, n_mels < 0, a missing filterbank,
 * clamp_eps or pow not positive; ESCX_ERR_UNSUPPORTED: a window above 4096. */
int escx_spec_loss_create(const escx_spec_loss_config* cfg, int device, escx_spec_loss* out);
void escx_spec_loss_destroy(escx_spec_loss h);
/* Floats of per-stream scratch one evaluation of (batch, n_samples) uses (grow-only, shared by the handles of a stream); -1 on a bad argument. */
int64_t escx_spec_loss_workspace_floats(escx_spec_loss h, int batch, int n_samples, int want_d_est, int want_d_ref);
/* loss_dev[0] = the loss of est (B, L) against ref (B, L); d_est_dev / d_ref_dev (B, L), each optional, receive d loss / d est and d loss / d ref.  A NULL
 * gradient pointer launches nothing for that side and does not change the other side's bits.  Every argument is checked before the first launch
 * (ESCX_ERR_INVALID_ARG: null handle / signal / loss pointer, batch < 1, n_samples <= largest window / 2, another current device than the handle's).
 * No atomics, fixed summation order: two calls are bitwise equal. */
int escx_spec_loss_eval(escx_spec_loss h, const float* est_dev, const float* ref_dev, int batch, int n_samples, float* loss_dev, float* d_est_dev,
                        float* d_ref_dev, void* stream);
/* L1Loss (loss.py:11-48) over n values: loss_dev[0] = scale * sum |est - ref| (scale = 1 / n is the mean), d_est = scale * sign(est - ref) with
 * sign(0) = 0, d_ref = -d_est; both gradients optional. */
int escx_wave_l1(const float* est_dev, const float* ref_dev, int64_t n, float scale, float* loss_dev, float* d_est_dev, float* d_ref_dev, void* stream);
/* SISDRLoss (loss.py:51-139), per clip in fp64 on the fp32 samples: loss_dev (B,) and the optional unit gradients (B, L) w.r.t. the references (the
 * reference class's FIRST argument) and the estimates.  has_clip_min = 0: no clip_min; below clip_min the value is clip_min and the gradient zero. */
int escx_sisdr(const float* references_dev, const float* estimates_dev, int batch, int64_t n_samples, int scaling, int zero_mean, int has_clip_min,
               float clip_min, float* loss_dev, float* d_references_dev, float* d_estimates_dev, void* stream);

/* ---- evaluation metrics with per-clip lengths (reference: scripts/metrics.py:12-171, driven by eval_epoch, scripts/test.py:23-55) -------------------
 * A batch of clips of different lengths is zero-padded to n_samples; clip b is its first lengths_host[b] samples and gets the value of the reference's
 * call on that clip alone.  lengths_host follows the convention of the mixed-length codec calls: a HOST array of `batch` sample counts, copied by the
 * entry point; NULL = every clip has n_samples.  Nothing at or past a clip's length is read in either signal.  Every argument is checked before the
 * first launch (ESCX_ERR_INVALID_ARG; a length outside its range is named with its clip).  No floating-point atomics: two calls are bitwise equal,
 * and at equal (batch, n_samples) a clip's value does not depend on the other clips or their lengths.  Run on the current device, asynchronous on `stream`. */
/* MelSpectrogramDistance (scripts/metrics.py:96-121): out_dev[b] = sum over the 7 resolutions of
 * mean |log10(clamp(mel_raw)^2) - log10(clamp(mel_recon)^2)| over n_mels x the clip's OWN frames (1 + len[b] / hop of them, torch.stft center=True
 * reflecting about the clip's own end).  1024 < len[b] <= n_samples; the matrices are those of the mel loss above (same sample_rate rebuild rule). */
int escx_mel_distance(const float* raw_dev, const float* recon_dev, int batch, int n_samples, const int32_t* lengths_host, int sample_rate,
                      float* out_dev, void* stream);
/* SISDR (scripts/metrics.py:123-171), dB per clip over the clip's own samples (1 <= len[b] <= n_samples), fp64 accumulation in a fixed order; eps = 1e-8
 * on the projection, on the cross term and inside the log10 as in the reference; the mean of zero_mean is over len[b].  Identical signals give +inf. */
int escx_sisdr_metric(const float* ref_dev, const float* est_dev, int batch, int64_t n_samples, const int32_t* lengths_host, int scaling, int zero_mean,
                      float* out_dev, void* stream);
/* EntropyCounter.update (scripts/metrics.py:37-51): counts_dev[(s*G+g)*K + k] += number of codes == k in codes (B,S,G,T) int64; negative codes (the -1
 * filler of mixed-length / mixed-bitrate batches) are skipped, codes >= K are counted in overflow_dev[0] and nothing else.  counts and overflow int64. */
int escx_code_histogram(const int64_t* codes_dev, int B, int S, int G, int T, int K, int64_t* counts_dev, int64_t* overflow_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ESCX_H */
