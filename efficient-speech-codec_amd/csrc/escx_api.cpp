// libescx host side, part 3 of 3: the launch SEQUENCES of the inference path (one TransformerLayer, encoder, cross-scale quantiser, decoder), the derived weight images of the
// precision modes, and the C-ABI entry points that run them (include/escx.h).  Packing: escx_params.cpp; profiler: escx_profile.cpp.
// libescx C ABI implementation: handle, parameter packing, workspace, and the launch sequences of
// ESC.encode / ESC.decode / ESC.forward(eval).  Reference citations are relative to /root/reference/.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "escx_internal.h"
#include "launchers.h"

using namespace escx;

// Batch layout of a whole-path call: k parts of `per` clips (part i = clips [i * per, min((i + 1) * per, B))), each walked in passes of at most
// `pass` clips (escx_params.cpp pass_clips: the workspace sets are sized for one pass).
static void part_layout(escx_handle_s* h, int B, int T, int* k, int* per, int* pass) {
    *k = std::min(n_parts(h, B), h->n_sets);
    *pass = std::max(1, std::min(pass_clips(h, B, T), h->sets[0].shp.B));
    *per = *k <= 1 ? B : (B + *k - 1) / *k;
}

// Whole-path calls: run `part(first_clip, n_clips, stream)` once, or as two halves on two streams joined by events.
// Clips are independent end to end, so the halves never exchange data; overlapping them lets one half's kernels fill
// the CUs the other half's tail workgroups leave idle (a 36-clip layer launches only ~1.3-2.6 workgroups per CU).
template <class F>
static int run_halves(escx_handle_s* h, int B, int T, hipStream_t st, F part) {
    int k, per, pass;
    part_layout(h, B, T, &k, &per, &pass);
    auto run_part = [&](int b0, int nb, hipStream_t si) -> int {
        for (int off = 0; off < nb; off += pass) { const int r = part(b0 + off, std::min(pass, nb - off), si); if (r) return r; }
        return 0;
    };
    if (k <= 1) { use_set(h, 0); return run_part(0, B, st); }
    // Event timing stays valid under concurrency (each kernel is bracketed on its own stream); ESCX_PROF_SERIAL=1 puts the
    // parts back to back on the caller's stream when isolated per-kernel durations are wanted.
    const bool concurrent = !(h->prof && (h->prof_serial || h->prof_isolated));
    if (concurrent) ESCX_HIP(hipEventRecord(h->ev_fork, st));
    // Join guard: once a part has been enqueued on a side stream, NO error path may return before the caller's stream waits
    // for it - the caller is free to release or reuse the buffers the moment this function returns an error.  Failures between fork and join are
    // therefore collected, every started side stream is joined (event, or a blocking stream synchronise when the event cannot be recorded), and
    // only then is the first failure reported.
    int rc = 0;
    bool started[escx_handle_s::MAX_PARTS] = {};
    auto hip_fail = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == 0) { set_error("run_halves: %s: %s", what, hipGetErrorString(e)); rc = ESCX_ERR_HIP; }
        return e != hipSuccess;
    };
    // fork every side stream, then enqueue the passes ROUND-ROBIN over the parts (pass j of part 0, pass j of part 1, ...): the host feeds both streams from the
    // start instead of queueing a whole part (hundreds of launches for a 288-clip batch) before the other stream sees its first kernel
    for (int i = 1; i < k && concurrent && !rc; ++i) {
        if (i * per >= B) break;
        if (hip_fail(hipStreamWaitEvent(h->sx[i], h->ev_fork, 0), "fork wait")) break;
        started[i] = true;
    }
    for (int off = 0; off < per && !rc; off += pass)
        for (int i = 0; i < k && !rc; ++i) {
            const int b0 = i * per, nb = std::min(per, B - b0);
            if (off >= nb) continue;
            const bool side = concurrent && i > 0;
            if (side && !started[i]) continue;
            use_set(h, i);
            const int prc = part(b0 + off, std::min(pass, nb - off), side ? h->sx[i] : st);
            if (prc && !rc) rc = prc;
        }
    for (int i = 1; i < k; ++i) {
        if (!started[i]) continue;
        if (hipEventRecord(h->ev_join[i], h->sx[i]) != hipSuccess || hipStreamWaitEvent(st, h->ev_join[i], 0) != hipSuccess) {
            const hipError_t e = hipStreamSynchronize(h->sx[i]);          // cannot order the streams with an event: wait on the host instead
            hip_fail(e == hipSuccess ? hipErrorUnknown : e, "join");
        }
    }
    use_set(h, 0);
    return rc;
}

static int frames_of(escx_handle_s* h, int L) { return 1 + L / h->cfg.hop_length; }
// frame count to reserve when only the latent width is known (decode first): the largest T that maps to W
static int frames_for_width(escx_handle_s* h, int W) {
    return h->cfg.patch_t * W + h->cfg.patch_t - 1;
}

namespace {
struct TmpBuf {                      // test-path scratch for the stage-level entry points (synchronous)
    float* p = nullptr;
    ~TmpBuf() { if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); } }
    int alloc(size_t n_floats) { return hipMalloc((void**)&p, std::max<size_t>(n_floats, 1) * sizeof(float)) == hipSuccess ? 0 : -1; }
};
}  // namespace

// Fused MLP on the bf16 matrix cores with every fp32 operand split exactly into three bf16 terms (fused_mlp_x3.h): DEFAULT for every instantiated width
// (48, 80, 96, 144, 192, 384).  ESCX_MLP_X3=<max padded width> restricts it, ESCX_MLP_X3=0 = the fp32-MFMA kernel (fused_mlp.h) everywhere - the
// round-4 arithmetic, which bench.py also reports (`fp32_mfma_only`) and tests/test_gpu_parity.py keeps as an arm.
// Terms per operand of the split-operand kernels (split_terms.h): 2 (default) = two fp16 terms + power-of-two weight scales, three cross products;
// ESCX_X3_TERMS=3 = three bf16 terms, exact split, six cross products (the first round-5 form).  One switch for the MLPs, the Q / K / V projections and PatchMerge / PatchSplit.
// (round 6: the mode is a field of the handle, escx_set_precision; escx_handle_s::prec)
static int x3_nt(const escx_handle_s* h) { return h->prec == 3 ? 3 : 2; }        // terms per operand of the split images / kernels (meaningful when prec != 0)

// Waves per workgroup (4 or 8) for the fused kernels.  A wave owns `units` 16-row tiles; a workgroup's waves spread over the
// 4 SIMDs of a CU and workgroups are dealt round-robin to the 256 CUs, so the makespan in tile-times is
//   ceil(workgroups / 256) * ceil(NW / 4) * units.
// 8 waves share each weight fragment between twice as many rows (half the L2->LDS traffic) and win ties.
// `cap` = waves per SIMD the kernel's register budget allows (mlp_min_waves / attn_min_waves): at 3, an 8-wave workgroup leaves
// the third slot of every SIMD empty (one workgroup = 2 waves per SIMD, a second one does not fit), so 4-wave workgroups it is.
// Waves per workgroup of the split-operand MLP (fused_mlp_x3.h), measured at 36 clips (tools/ab.py; ms per step alone, 4 -> 8 waves):
// C = 45 1.25 -> 1.17, C = 72 0.96 -> 0.84, C = 96 1.13 -> 0.97, C = 144 1.34 -> 1.55, C = 192 0.97 -> 1.00, C = 384 1.59 -> 1.11 (8 waves cap the kernel at 256
// registers with a small spill, but put two waves on every SIMD).  Small grids keep the fp32 kernel's rule (`variant`): a wave per SIMD first.
static int mlp_x3_nw(int M, int Cp, int variant) {
    const long long tiles = (M + 15) / 16;
    if (Cp == 144 || Cp == 192) return 4;
    if (Cp == 384) return variant == 3 ? 8 : 4;
    return tiles >= 8 * 512 ? 8 : (variant == 3 ? 8 : 4);
}

static int pick_nw(long long tiles, int units, int cap = 4) {
    if (cap == 3) return 4;
    auto cost = [&](int nw) { const long long wg = (tiles / units + nw - 1) / nw; return ((wg + 255) / 256) * ((nw + 3) / 4) * units; };
    return cost(8) <= cost(4) ? 8 : 4;
}
static int mlp_cap(int Cp) { return Cp <= ESCX_MLP_OCC4 ? 4 : (Cp <= 192 ? 3 : 1); }                              // fused_mlp.h: mlp_min_waves<CP, 1>
static int attn_cap(int Cp, int tmw) { const int v = Cp * tmw; return v <= 96 ? 4 : (v <= 160 ? 3 : (v <= 192 ? 2 : 1)); }   // fused_attn.h: attn_min_waves
// Hidden split of the fused MLP (fused_mlp.h): at the deep scales a clip has so few token rows (600 / 1200 at C = 384 / 192
// for 3 s) that one wave per 16-row tile cannot fill 1024 SIMDs at serving batch sizes, so three workgroups share a row block
// and a combine pass adds their fc2 partial sums in fixed order.  The rule depends on the layer geometry only - never on the
// batch - so that a clip's arithmetic (and therefore its codes) is identical in any batch or shard it is processed in.
// The partial sums live in the (otherwise unused) hidden-activation buffer of the unfused path: needs hiddenP >= 3 * Cp.
static int mlp_hs_for(int tokens_per_clip, int HT, int Cp) { return (tokens_per_clip <= 1200 && HT % 3 == 0 && HT * 16 >= 3 * Cp) ? 3 : 1; }
// The same split over the head groups of the fused attention (partials share the buffer; an MLP always follows on the same
// stream).  Like the hidden split it would have to depend on the clip's geometry only, never on the batch (it re-associates the projection
// sum).  Measured with ESCX_ATTN_GS_TOKENS=600 (the C = 384 scale of a 3 s clip; tools/small_batch.py): one clip 3.52 -> 3.12 ms, 4 clips
// 4.30 -> 3.90, 8 clips 5.56 -> 5.19 ms, but 36 clips +0.2 .. 0.8 % and 288 clips 121.4 -> 123.5 ms in same-box A/B runs (a wave holds one window pair and is
// MFMA-bound on its own: three workgroups per pair put a small grid on three times the CUs, a full grid gains nothing and pays the
// combine).  The throughput configurations are the ones BASELINE quotes, so the split is OFF by default; all parity tests and the
// 576-clip sweep are bit-exact with it on, a latency-bound deployment can switch it on.
// Round 4: decided on parity evidence, not on the 36-clip throughput.  Oracle sweeps of BOTH settings on the same clips
// (profiles/r4_parity_sweep_*_gs_{on,off}.log): ESC-Base 576 clips - split ON 576 / 576 bit-exact, split OFF 575 / 576 (one near-tie code); ESC-Large 288
// clips - 286 / 288 either way (the same two near-tie clips).  The split is therefore ON for every batch size (geometry rule: maps of up to 600
// tokens per clip = the C = 384 scale of a 3 s clip).  Cost / gain on the day's build (tools/ab.py): 36 clips 15.79 -> 15.87 ms (+0.5 %), 8 clips
// 5.59 -> 5.18 ms, one clip 3.52 -> 3.12 ms.  ESCX_ATTN_GS_TOKENS=0 switches it off.
static int attn_gs_for(const escx_handle_s* h, int tokens_per_clip, int n_groups, int hiddenP, int Cp) { return (tokens_per_clip <= h->attn_gs_tokens && n_groups % 3 == 0 && hiddenP >= 3 * Cp) ? 3 : 1; }
static int mlp_variant_for(int M, int Cp) { return pick_nw((M + 15) / 16, 1, mlp_cap(Cp)) == 8 ? 3 : 1; }     // fused_swin.hip: 1 = (TM 1, NW 4), 3 = (TM 1, NW 8)
// The hidden-split MLP at C >= 384: 8-wave workgroups when that fills one dispatch round anyway (36-clip batches: 255 workgroups, half the
// weight DMA per wave), 4-wave ones for small grids - with 8 waves two waves share every SIMD's MFMA pipe and a 15-workgroup launch takes
// as long as a 255-workgroup one (single clip: 197 us; 4 waves: one wave per SIMD).  A wave's rows and arithmetic are the same either way.
// Measured (tools/small_batch.py, ms per encode+decode, 8-wave -> rule): B = 1 3.88 -> 3.52, B = 4 4.67 -> 4.30, B = 8 5.96 -> 5.60, B = 12 6.79 -> 6.64;
// at 8 clips per part (225 four-wave workgroups) the two forms cross over.
static int mlp_split_nw(int M, int hs) {
    const long long tiles = (M + 15) / 16;
    return ((tiles + 3) / 4) * hs <= 192 ? 4 : 8;
}
// variant of the LDS-staged fused MLP (fused_swin.hip: 1 = 4 waves, 3 = 8 waves per workgroup) for a layer's hidden split hs
static int mlp_variant_choice(int hs, int M, int Cp) {
    if (hs > 1) return (Cp >= 384 && mlp_split_nw(M, hs) == 8) ? 3 : 1;
    return mlp_variant_for(M, Cp);
}

// One TransformerLayer on padded token maps.  x_in is read-only; y receives (B, H'*W, CoutP).
// attention.py:48-91 (layer), 129-178 (block): LN1 -> pad -> roll -> windows -> attention -> reverse -> residual -> MLP.
static int run_layer(escx_handle_s* h, const Layer& L, const float* x_in, float* y, int B, int H, int W, int* Hout, hipStream_t st) {
    const int tokens = H * W, M = B * tokens;
    const int ws = h->ws, NW2 = ws * ws;
    const int Hp = rup(H, ws), Wp = rup(W, ws), slots = Hp * Wp, Ms = B * slots;
    float* cur = L.scale ? h->work : y;
    const float* src = x_in;
    int rc;
    for (size_t j = 0; j < L.blocks.size(); ++j) {
        const BlockW& bw = L.blocks[j];
        const int shift = (j % 2 == 0) ? 0 : ws / 2;                          // attention.py:29
        const int* map = nullptr;
        if (!h->len && (rc = get_map(h, H, W, shift, &map))) return rc;
        const std::string tag = h->prof ? "[C=" + std::to_string(L.C) + "]" : std::string();
        const double dM = M, dMs = Ms, dC = L.C, f4 = sizeof(float);
        bool attn_done = false;
        if (h->len) {
            // Mixed-length batch (W = Wmax): the general fused kernel on the batch-wide table of the clips' own windows (fused_attn.h LEN).  The head-group split
            // follows the padded map's tokens per clip (H * Wmax) and the waves per workgroup change no arithmetic, so a clip's result depends on Wmax and
            // the mode only.  The packed half-window kernel has no length form (the general kernel runs at H == 2); a width without a fused mode runs the unfused sequence below.
            LenMap lm;
            if ((rc = get_len_map(h, *h->len, H, shift, &lm))) return rc;
            int frc = -1;
            if (h->use_fused && h->use_fused_attn && L.attn_mode >= 0) {
                const double dW = 16.0 * lm.n_windows;
                const int nw = (L.Cp > 192 || (L.Cp == 192 && bw.x3a)) ? 4 : pick_nw(lm.n_windows, attn_windows_per_wave(L.Cp), attn_cap(L.Cp, attn_windows_per_wave(L.Cp)));
                int gs = attn_gs_for(h, tokens, L.n_groups, L.hiddenP, L.Cp);
                PROF("attn_fused_len" + tag, 2 * dW * dC * 4 * dC + 4 * dW * 16 * dC, 2 * dW * dC * f4,
                     frc = attn_fused(src, cur, L.Cp, L.C, L.attn_mode, L.n_groups, bw.ln1_g, bw.ln1_b, bw.waf, bw.baf, bw.bias_tab_f, bw.bproj,
                                      lm.dev, 0, 0, lm.n_windows, 1, lm.n_windows, shift > 0, 1.0f / std::sqrt((float)L.hd), nw, &gs, h->hid, M, st, nullptr, bw.x3a, x3_nt(h), true));
                if (frc == 0 && gs > 1)
                    PROF("attn_combine" + tag, 0, (gs + 2) * dM * L.Cp * f4, rows_combine(cur, src, h->hid, bw.bproj, M, L.Cp, gs, st));
            }
            if (frc != 0) {         // no fused mode for this width (or the fused kernels are switched off): the unfused sequence on the same table, flags to the attention core
                if (h->prof && !h->prof_recs.empty() && h->use_fused && h->use_fused_attn && L.attn_mode >= 0) h->prof_recs.pop_back();
                const int Msl = 16 * lm.n_windows;
                const double dW = Msl;
                PROF("ln1_gather" + tag, 0, 2 * dW * dC * f4, ln_rows(1, src, h->xn, bw.ln1_g, bw.ln1_b, lm.dev, Msl, 0, Msl, L.C, L.Cp, st));
                PROF("gemm_qkv" + tag, 2 * dW * dC * 3 * dC, (dW * 4 * dC + 3 * dC * dC) * f4,
                     gemm_qkv(h->xn, L.Cp, Msl, bw.wqkv, L.Nqkv, L.Cp, h->qkv, bw.bqkv, L.nH * L.hdp, 1.0f / std::sqrt((float)L.hd), st));
                int arc = 0;
                PROF("window_attn_len" + tag, 4 * dW * 16 * dC, dW * 4 * dC * f4,
                     arc = window_attention_len(h->qkv, bw.bias_tab, h->obuf, lm.n_windows, L.nH, L.hdp, L.Nqkv, L.Ko, lm.dev + 16 * lm.n_windows, shift > 0, st));
                if (arc) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "head_dim %d unsupported by the attention kernel", L.hd);
                PROF("gemm_proj" + tag, 2 * dW * dC * dC, (3 * dW * dC + dC * dC) * f4,
                     gemm_proj_scatter(h->obuf, L.Ko, Msl, bw.wproj, L.Cp, L.Ko, cur, src, bw.bproj, lm.dev, Msl, 0, st));
            }
            attn_done = true;
        } else
        if (h->use_fused && h->use_fused_attn && L.attn_mode >= 0) {
            int frc = 0;
            int nw = (L.Cp > 192 || (L.Cp == 192 && bw.x3a)) ? 4 : pick_nw(Ms / 16, attn_windows_per_wave(L.Cp), attn_cap(L.Cp, attn_windows_per_wave(L.Cp)));    // 8 waves cap the kernel at 256 VGPRs: spills above C = 192
            if (H == 2 && W % 4 == 0) nw = -(L.Cp > 192 ? 4 : pick_nw((Ms / 16 + 1) / 2, 1));    // packed half-window pairs
            const double proj_rows = nw < 0 ? dM : dMs;         // packed pairs project only the real tokens
            int gs = attn_gs_for(h, tokens, L.n_groups, L.hiddenP, L.Cp);
            PROF("attn_fused" + tag, 2 * proj_rows * dC * 4 * dC + 4 * dMs * 16 * dC, 2 * dM * dC * f4,
                 frc = attn_fused(src, cur, L.Cp, L.C, L.attn_mode, L.n_groups, bw.ln1_g, bw.ln1_b, bw.waf, bw.baf, bw.bias_tab_f, bw.bproj,
                                  map, slots, tokens, Ms / 16, Hp / 4, Wp / 4, shift > 0, 1.0f / std::sqrt((float)L.hd), nw, &gs, h->hid, M, st, nullptr, (nw > 0 || L.Cp == 384) ? bw.x3a : nullptr, x3_nt(h)));      // C = 384: the split stream exists for the packed (nw < 0) kernel only
            attn_done = (frc == 0);
            if (attn_done && gs > 1)
                PROF("attn_combine" + tag, 0, (gs + 2) * dM * L.Cp * f4, rows_combine(cur, src, h->hid, bw.bproj, M, L.Cp, gs, st));
        }
        if (!attn_done) {
        PROF("ln1_gather" + tag, 0, (dM + dMs) * dC * f4,
             ln_rows(1, src, h->xn, bw.ln1_g, bw.ln1_b, map, slots, tokens, Ms, L.C, L.Cp, st));
        PROF("gemm_qkv" + tag, 2 * dMs * dC * 3 * dC, (dMs * 4 * dC + 3 * dC * dC) * f4,
             gemm_qkv(h->xn, L.Cp, Ms, bw.wqkv, L.Nqkv, L.Cp, h->qkv, bw.bqkv, L.nH * L.hdp, 1.0f / std::sqrt((float)L.hd), st));
        int arc = 0;
        if (ws != 4)
        PROF("window_attn_any" + tag, 4 * dMs * NW2 * dC, dMs * 4 * dC * f4,
             arc = window_attention_any(h->qkv, bw.bias_tab, h->obuf, Ms / NW2, ws, L.nH, L.hd, L.hdp, L.Nqkv, L.Ko, Hp / ws, Wp / ws, shift, st));
        else
        PROF("window_attn" + tag, 4 * dMs * 16 * dC, dMs * 4 * dC * f4,
             arc = window_attention(h->qkv, bw.bias_tab, h->obuf, Ms / 16, L.nH, L.hdp, L.Nqkv, L.Ko, Hp / 4, Wp / 4, shift > 0, st));
        if (arc) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "head_dim %d unsupported by the attention kernel", L.hd);
        PROF("gemm_proj" + tag, 2 * dMs * dC * dC, (dMs * dC + 2 * dM * dC + dC * dC) * f4,
             gemm_proj_scatter(h->obuf, L.Ko, Ms, bw.wproj, L.Cp, L.Ko, cur, src, bw.bproj, map, slots, tokens, st));
        }
        if (h->use_fused) {
            int frc = 0;
            int hs = mlp_hs_for(tokens, L.hiddenP / 16, L.Cp);
            const int variant = mlp_variant_choice(hs, M, L.Cp);
            if (bw.x3w) {       // three-term bf16 split on the bf16 matrix cores (fused_mlp_x3.h); same hidden-split rule and combine
                if (h->mlp_split_fold && L.scale == 2 && j + 1 == L.blocks.size() && hs == 1 && L.sub_x3s) {      // PatchSplit in the epilogue of the layer's last MLP
                    const MlpSplit sp{reinterpret_cast<const float*>(L.sub_x3s), L.sub_g, L.sub_b, y, 2 * L.CoutP / 16, H, W, L.CoutP};
                    int src3 = -1, one = 1;
                    PROF("mlp_x3_split" + tag, 4 * dM * dC * L.hidden + 2.0 * dM * dC * 2 * L.Cout, (dM * dC + dM * 2 * L.Cout) * f4,
                         src3 = mlp_x3(cur, M, L.C, L.Cp, bw.ln2_g, bw.ln2_b, bw.b1, bw.b2, bw.x3w, L.hiddenP, mlp_x3_nw(M, L.Cp, variant), &one, nullptr, st, &sp, x3_nt(h)));
                    if (src3 == 0) { *Hout = 2 * H; return launch_ok(L.prefix.c_str()); }
                    if (h->prof && !h->prof_recs.empty()) h->prof_recs.pop_back();
                }
                int xrc = -1, xhs = hs;
                PROF("mlp_x3" + tag, 4 * dM * dC * L.hidden, 2 * dM * dC * f4,
                     xrc = mlp_x3(cur, M, L.C, L.Cp, bw.ln2_g, bw.ln2_b, bw.b1, bw.b2, bw.x3w, L.hiddenP, mlp_x3_nw(M, L.Cp, variant), &xhs, h->hid, st, nullptr, x3_nt(h)));
                if (xrc == 0) {
                    if (xhs > 1) PROF("mlp_combine" + tag, 0, (xhs + 2) * dM * L.Cp * f4, rows_combine(cur, cur, h->hid, bw.b2, M, L.Cp, xhs, st));
                    src = cur; continue;
                }
                if (h->prof && !h->prof_recs.empty()) h->prof_recs.pop_back();
            }
            // PatchSplit in the epilogue of the layer's last MLP (fused_mlp.h SPLIT): one launch and one HBM round trip of the
            // pre-split map less.  ESCX_MLP_SPLIT_FOLD=0: the separate LN + linear launch (rowgemm_fused_kernel), as before.
            if (h->mlp_split_fold && L.scale == 2 && j + 1 == L.blocks.size() && hs == 1) {
                const MlpSplit sp{L.sub_wf, L.sub_g, L.sub_b, y, 2 * L.CoutP / 16, H, W, L.CoutP};
                int sfrc = -1;
                PROF("mlp_split_fused" + tag, 4 * dM * dC * L.hidden + 2.0 * dM * dC * 2 * L.Cout, (dM * dC + dM * 2 * L.Cout) * f4,
                     sfrc = mlp_fused(cur, M, L.C, L.Cp, bw.ln2_g, bw.ln2_b, bw.w1f, bw.b1, bw.w2f, bw.b2, bw.wcf, L.hiddenP, variant, &hs, h->hid, st, nullptr, &sp));
                if (sfrc == 0) { *Hout = 2 * H; return launch_ok(L.prefix.c_str()); }
                if (h->prof && !h->prof_recs.empty()) h->prof_recs.pop_back();      // no SPLIT instantiation for this width: nothing was launched
            }
            PROF("mlp_fused" + tag, 4 * dM * dC * L.hidden, 2 * dM * dC * f4,
                 frc = mlp_fused(cur, M, L.C, L.Cp, bw.ln2_g, bw.ln2_b, bw.w1f, bw.b1, bw.w2f, bw.b2, bw.wcf, L.hiddenP, variant, &hs, h->hid, st));
            if (frc == 0 && hs > 1) PROF("mlp_combine" + tag, 0, (hs + 2) * dM * L.Cp * f4, rows_combine(cur, cur, h->hid, bw.b2, M, L.Cp, hs, st));
            if (frc == 0) { src = cur; continue; }
        }
        PROF("ln2" + tag, 0, 2 * dM * dC * f4,
             ln_rows(0, cur, h->xn, bw.ln2_g, bw.ln2_b, nullptr, tokens, tokens, M, L.C, L.Cp, st));
        PROF("gemm_fc1_gelu" + tag, 2 * dM * dC * L.hidden, (dM * (dC + L.hidden) + dC * L.hidden) * f4,
             gemm_gelu(h->xn, L.Cp, M, bw.w1, L.hiddenP, L.Cp, h->hid, bw.b1, st));
        PROF("gemm_fc2_res" + tag, 2 * dM * dC * L.hidden, (dM * (2 * dC + L.hidden) + dC * L.hidden) * f4,
             gemm_residual(h->hid, L.hiddenP, M, bw.w2, L.Cp, L.hiddenP, cur, bw.b2, cur, st));
        src = cur;
    }
    if (L.scale == 1) {
        const int H2 = (H + 1) / 2;
        const int* map;
        if ((rc = get_map(h, H, W, -1, &map))) return rc;
        int mrc = -1;
        if (h->use_fused)
            PROF("merge_fused" + (h->prof ? "[C=" + std::to_string(L.C) + "]" : std::string()), 2.0 * B * H2 * W * 2 * L.C * L.Cout, ((double)M * L.C + (double)B * H2 * W * L.Cout) * 4,
                 mrc = rowgemm_fused(2, cur, y, L.sub_g, L.sub_b, L.sub_wf, map, B * H2 * W, H2 * W, tokens, L.C, L.Cp, L.CoutP, 0, 0, 0, 0, st, L.sub_x3, x3_nt(h)));
        if (mrc != 0) {
        PROF("merge_ln", 0, 2.0 * M * L.C * 4,
             ln_rows(2, cur, h->xn, L.sub_g, L.sub_b, map, H2 * W, tokens, B * H2 * W, L.C, L.Cp, st));
        PROF("merge_gemm", 2.0 * B * H2 * W * 2 * L.C * L.Cout, (double)B * H2 * W * (2 * L.C + L.Cout) * 4,
             gemm_store(h->xn, 2 * L.Cp, B * H2 * W, L.sub_w, L.CoutP, 2 * L.Cp, y, L.CoutP, nullptr, st));
        }
        *Hout = H2;
    } else if (L.scale == 2) {
        int src2 = -1;
        if (h->use_fused)
            PROF("split_fused" + (h->prof ? "[C=" + std::to_string(L.C) + "]" : std::string()), 2.0 * M * L.C * 2 * L.Cout, (double)M * (L.C + 2 * L.Cout) * 4,
                 src2 = rowgemm_fused(1, cur, y, L.sub_g, L.sub_b, L.sub_wf, nullptr, M, tokens, tokens, L.C, L.Cp, 2 * L.CoutP, 1, H, W, L.CoutP, st, L.sub_x3, x3_nt(h)));
        if (src2 != 0) {
        PROF("split_ln", 0, 2.0 * M * L.C * 4,
             ln_rows(0, cur, h->xn, L.sub_g, L.sub_b, nullptr, tokens, tokens, M, L.C, L.Cp, st));
        PROF("split_gemm", 2.0 * M * L.C * 2 * L.Cout, (double)M * (L.C + 2 * L.Cout) * 4,
             gemm_split(h->xn, L.Cp, M, L.sub_w, 2 * L.CoutP, L.Cp, y, H, W, L.CoutP, st));
        }
        *Hout = 2 * H;
    } else {
        *Hout = H;
    }
    return launch_ok(L.prefix.c_str());
}

static int run_stft(escx_handle_s* h, const float* wave, int B, int L, int T, float* spec, hipStream_t st) {
    if (h->len) {       // mixed-length batch: L = row stride of `wave`; clip b reflects about its own last sample and the frames past 1 + L_b / hop are not computed
        PROF("stft_dft_gemm_len", 2.0 * B * T * h->cfg.win_length * 2 * h->F, ((double)B * L + (double)B * T * 2 * h->F) * 4,
             gemm_frames_len(wave, h->len->d_L, B, L, T, h->cfg.hop_length, h->left - h->n_fft / 2, h->dft_w, h->cfg.in_dim * h->Fp, h->winP, spec, st));
        return launch_ok("stft");
    }
    PROF("stft_dft_gemm", 2.0 * B * T * h->cfg.win_length * 2 * h->F, ((double)B * L + (double)B * T * 2 * h->F) * 4,
         gemm_frames(wave, B, L, T, h->cfg.hop_length, h->left - h->n_fft / 2, h->dft_w, h->cfg.in_dim * h->Fp, h->winP, spec, st));
    return launch_ok("stft");
}

static int run_patch_embed(escx_handle_s* h, const float* spec, int B, int T, int W, float* tok, hipStream_t st) {
    const escx_config& c = h->cfg;
    const int H0 = c.in_freq / c.patch_f;
    const double toks = (double)B * H0 * W;
    PROF("patch_embed_gemm", 2.0 * toks * c.in_dim * c.patch_f * c.patch_t * h->C0, ((double)B * T * 2 * h->F + toks * h->C0) * 4,
         gemm_patch(spec, B, T, c.in_dim, h->Fp, H0, W, c.patch_f, c.patch_t, h->pe_w, h->C0p, h->Kpe, tok, h->pe_b, st));
    PROF("patch_embed_ln", 0, 2 * toks * h->C0 * 4,
         ln_rows(0, tok, tok, h->pe_g, h->pe_beta, nullptr, H0 * W, H0 * W, B * H0 * W, h->C0, h->C0p, st));
    return launch_ok("patch_embed");
}

static int run_encoder(escx_handle_s* h, const Shapes& s, hipStream_t st) {     // base.py:143-158
    int rc, H = s.H0, Hn;
    if ((rc = run_patch_embed(h, h->spec, s.B, s.T, s.W, h->stageA, st))) return rc;
    if ((rc = run_layer(h, h->layers[0], h->stageA, h->enc_hs[0], s.B, H, s.W, &Hn, st))) return rc;
    for (int i = 0; i + 1 < h->n; ++i) {
        if ((rc = run_layer(h, h->layers[1 + i], h->enc_hs[i], h->enc_hs[i + 1], s.B, H, s.W, &Hn, st))) return rc;
        H = Hn;
    }
    return 0;
}

// De-quantisation tables of the product quantisers (Quant::tab, escx_internal.h): out = dec + up_proj_g(codebook_g[code]) becomes a table-row add.
// Built by pvq_up_kernel ITSELF on Ksz pseudo-vectors (vector k carries code k in every group; one "clip" of ov * Ksz frames), so a table entry is
// bit for bit what the up-projection MFMA chain produces for that code (inference only - like the folded de-embedding the tables are derived
// state: finalisation and every device-side parameter refresh mark them stale, the next inference entry rebuilds them on the caller's stream
// before the batch parts fork).  ESCX_PVQ_TABLE=0: no tables (up-projection on the MFMA, the round-4 form).
static int ensure_pvq_tables(escx_handle_s* h, hipStream_t st) {
    if (!h->pvq_tab_stale) return 0;
    const escx_config& c = h->cfg;
    const int G = c.group_size, Ksz = c.codebook_size;
    const bool on = h->pvq_table;
    // Derived buffers are allocated the first time they are wanted and KEPT (a precision switch or a parameter refresh only re-launches the pack kernels: no hipFree,
    // no device synchronisation on the way - ADVICE r5); the ACTIVE pointer says whether the launch sequence uses them.
    auto grab = [&](void** buf, size_t bytes) -> bool { return *buf || hipMalloc(buf, bytes) == hipSuccess; };
    if (on && !h->iota_codes) {
        std::vector<long long> iota((size_t)G * Ksz);
        for (int g = 0; g < G; ++g) for (int k = 0; k < Ksz; ++k) iota[(size_t)g * Ksz + k] = k;
        ESCX_HIP(hipMalloc((void**)&h->iota_codes, iota.size() * sizeof(long long)));
        ESCX_HIP(hipMemcpy(h->iota_codes, iota.data(), iota.size() * sizeof(long long), hipMemcpyHostToDevice));
    }
    for (Quant& q : h->quants) {
        if (!on || !q.tab_ok) { if (q.tab) { ESCX_HIP(hipDeviceSynchronize()); (void)hipFree(q.tab); q.tab = nullptr; } continue; }
        if (!q.tab) ESCX_HIP(hipMalloc((void**)&q.tab, (size_t)Ksz * q.Kq * sizeof(float)));
        if (pvq_up(h->iota_codes, (long long)G * Ksz, q.cbraw, G, Ksz, q.dt, 1, q.Hq, c.overlap * Ksz, q.Cp, c.overlap, q.wup, q.Kq, q.Kup, nullptr, q.tab, st) != 0) {
            ESCX_HIP(hipDeviceSynchronize()); (void)hipFree(q.tab); q.tab = nullptr;      // no up-projection kernel for this width: the engine form stays
        }
    }
    const int nt = x3_nt(h);
    const bool split_on = h->prec != 0;
    const int x3_max = split_on ? h->mlp_x3_max : 0;
    // the two-term fp16 stream of the halo-tiled de-embedding (fused_deembed.h deembed7_x2_kernel): in the two-term mode only - the three-term mode and the fp32-MFMA
    // mode keep the fp32 kernel (the latter stays bit-identical to round 4)
    {
        const bool want = x3_max > 0 && h->prec == 2 && h->deembed_halo && h->dch_w && deembed7_x2_image_bytes(h->C0p) > 0;
        h->dch_x2 = nullptr;
        if (want && grab(&h->dch_x2_buf, deembed7_x2_image_bytes(h->C0p)) && deembed7_x2_pack(h->dch_w, h->dch_x2_buf, h->C0p, st) == 0) h->dch_x2 = h->dch_x2_buf;
    }
    // the split weight images of the fused MLP (fused_mlp_x3.h)
    for (Layer& L : h->layers)
        for (BlockW& bw : L.blocks) {
            const bool want = x3_max > 0 && L.Cp <= x3_max && (L.Cp == 48 || L.Cp == 80 || L.Cp == 96 || L.Cp == 144 || L.Cp == 192 || L.Cp == 384) && L.hiddenP % 32 == 0;
            bw.x3w = nullptr;
            if (want && grab(&bw.x3w_buf, mlp_x3_bytes(L.Cp, L.hiddenP, 3)) &&         // sized for the larger (three-term) image
                mlp_x3_pack(bw.w1, bw.w2, bw.x3w_buf, L.Cp, L.hiddenP, st, nt, bw.ln2_g, bw.ln2_b, bw.b1, L.C) == 0) bw.x3w = bw.x3w_buf;
        }
    // the split Q / K / V weight streams of the fused attention (fused_attn.h X3)
    const int ax3_max = split_on ? h->attn_x3_max : 0;
    for (Layer& L : h->layers)
        for (BlockW& bw : L.blocks) {
            const bool want = ax3_max > 0 && L.Cp <= ax3_max && L.attn_mode >= 0 && h->use_fused_attn &&
                              ((L.Cp == 48 && L.attn_mode == 0) || (L.Cp == 80 && L.attn_mode != 1) || (L.Cp == 96 && L.attn_mode != 2) || (L.Cp == 144 && L.attn_mode != 2) || (L.Cp == 192 && L.attn_mode == 1) || (L.Cp == 384 && L.attn_mode == 0));      // 384: the packed H = 2 kernel only (the launcher falls back to fp32 elsewhere)
            bw.x3a = nullptr;
            if (!want || !grab(&bw.x3a_buf, attn_x3_bytes(L.Cp, L.attn_mode, L.n_groups))) continue;
            if (attn_x3_pack(bw.waf, bw.x3a_buf, L.Cp, L.attn_mode, L.n_groups, st, nt, bw.ln1_g, bw.ln1_b, L.C, bw.baf) == 0) bw.x3a = bw.x3a_buf;
        }
    // the split weight streams of PatchMerge / PatchSplit (fused_rowgemm.h rowgemm_x3_kernel)
    for (Layer& L : h->layers) {
        const int KP = L.scale == 1 ? 2 * L.Cp : L.Cp, Np = L.scale == 1 ? L.CoutP : 2 * L.CoutP;
        const bool want = split_on && h->rowgemm_x3 && L.scale != 0 && L.sub_wf && (KP == 80 || KP == 96 || KP == 144 || KP == 160 || KP == 192 || KP == 288 || KP == 384);
        L.sub_x3 = nullptr; L.sub_x3s = nullptr;
        if (!want || !grab(&L.sub_x3_buf, rowgemm_x3_bytes(KP, Np))) continue;
        if (rowgemm_x3_pack(L.sub_wf, L.sub_x3_buf, KP, Np, st, nt, L.sub_g, L.sub_b, (L.scale == 1 ? 2 : 1) * L.C) == 0) L.sub_x3 = L.sub_x3_buf;
        if (L.scale == 2 && (L.Cp == 80 || L.Cp == 96 || L.Cp == 144) && L.Cp <= x3_max && grab(&L.sub_x3s_buf, mlp_x3_split_bytes(L.Cp, Np)) &&       // PatchSplit folded into the split-operand MLP's epilogue
            mlp_x3_split_pack(L.sub_wf, L.sub_x3s_buf, L.Cp, Np, st, nt, L.sub_g, L.sub_b, L.C) == 0) L.sub_x3s = L.sub_x3s_buf;
    }
    h->pvq_tab_stale = false;
    return launch_ok("derived images");
}

// escx_set_precision / escx_get_precision (include/escx.h): the arithmetic of the K = C contractions of this handle.  Takes effect with the next call: the
// split images are derived state and are re-packed on that call's stream.
extern "C" int escx_set_precision(escx_handle h, int mode) {
    if (!h) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null handle");
    if (mode != ESCX_PRECISION_FP32 && mode != ESCX_PRECISION_BF16X3 && mode != ESCX_PRECISION_F16X2)
        ESCX_FAIL(ESCX_ERR_INVALID_ARG, "precision mode %d (0 = fp32 MFMA, 3 = three bf16 terms, 2 = two fp16 terms)", mode);
    if (mode != h->prec) { h->prec = mode; h->pvq_tab_stale = true; }
    return ESCX_OK;
}
extern "C" int escx_get_precision(escx_handle h) { return h ? h->prec : ESCX_ERR_INVALID_ARG; }

// scale of the per-vector loss terms: mse over (Tq, d) per group, mean over groups.  A mixed-length batch divides by the clip's own frame count in its
// reduction (loss_reduce_len_kernel), so the terms carry 1 / (d G) only.
static float pvq_loss_scale(const escx_handle_s* h, const Quant& q, int Tq) {
    if (h->len) return 1.0f / ((float)q.d * h->cfg.group_size);
    return 1.0f / ((float)Tq * q.d * h->cfg.group_size);
}

static int run_pvq_encode(escx_handle_s* h, const Quant& q, const float* enc, const float* dec, int B, int W, long long* codes,
                          long long bstride, float* loss, hipStream_t st) {
    const escx_config& c = h->cfg;
    const int Tq = W / c.overlap, M = B * Tq;
    const int splits = pvq_down_splits(M, q.Kq, q.Cp);
    if ((size_t)splits * M * q.Nz > h->zpart_cap) ESCX_FAIL(ESCX_ERR_STATE, "split-K scratch too small");
    const double vec = (double)c.overlap * q.Hq * q.C;
    PROF("pvq_down_gemm", 2.0 * M * vec * q.d, (double)M * vec * (dec ? 2 : 1) * 4,
         gemm_pvq_down(enc, dec, B, q.Hq, W, q.Cp, c.overlap, q.wd, q.Nz, q.Kq, h->zpart, splits, st));
    int src_rc = 0;
    PROF("pvq_search", 2.0 * M * c.group_size * c.codebook_size * q.d, ((double)c.group_size * c.codebook_size * q.d + (double)M * c.group_size * q.d) * 4,
         src_rc = pvq_search(h->zpart, splits, M, q.Nz, q.cbn, q.c2, q.cbraw, c.group_size, c.codebook_size, q.d, q.dt, Tq, codes, bstride,
                             loss, pvq_loss_scale(h, q, Tq), c.l2norm, st));
    if (src_rc) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "codebook_dim %d unsupported by the search kernel", q.d);
    return launch_ok("pvq_encode");
}

static int run_pvq_decode(escx_handle_s* h, const Quant& q, const long long* codes, long long bstride, const float* dec, int B, int W,
                          float* out, hipStream_t st) {
    const escx_config& c = h->cfg;
    const double vec = (double)c.overlap * q.Hq * q.C, Mv = (double)B * (W / c.overlap);
    const bool special = h->pvq_up_kernel;     // ESCX_PVQ_UP_KERNEL=0: the GEMM engine's generic form (A/B, fallback)
    if (q.tab && special) {          // table-row add (Quant::tab): no contraction at run time, bit-identical to the kernels below
        PROF("pvq_tab_add", 0, Mv * vec * (dec ? 3 : 2) * 4,
             pvq_tab_add(codes, bstride, q.tab, q.gq, c.group_size, c.codebook_size, B, q.Hq, W, q.Cp, c.overlap, dec, out, st));
        return launch_ok("pvq_decode");
    }
    int urc = -1;
    if (special)
        PROF("pvq_up_gemm", 2.0 * Mv * vec * q.d, Mv * vec * (dec ? 2 : 1) * 4,
             urc = pvq_up(codes, bstride, q.cbraw, c.group_size, c.codebook_size, q.dt, B, q.Hq, W, q.Cp, c.overlap, q.wup, q.Kq, q.Kup, dec, out, st));
    if (urc != 0) {
        if (special && h->prof && !h->prof_recs.empty()) h->prof_recs.pop_back();
    PROF("pvq_up_gemm", 2.0 * Mv * vec * q.d, Mv * vec * (dec ? 2 : 1) * 4,
         gemm_pvq_up(codes, bstride, q.cbraw, c.group_size, c.codebook_size, q.dt, B, q.Hq, W, q.Cp, c.overlap, q.wup, q.Kq, q.Kup, dec, out, st));
    }
    return launch_ok("pvq_decode");
}

// One stream of the cross-scale quantiser: codes = search(down(enc - dec)); when `out` is given also out = dec + up(codebook[codes]) (csrvq.py:15-21).
// Default: ONE launch (fused_pvq.h).  ESCX_PVQ_FUSED=0, or a geometry the fused kernel is not instantiated for: the three-launch form
// (split-K down-projection GEMM -> pvq_search -> pvq_up), whose arithmetic the fused kernel reproduces bit for bit (profiles/r5_pvq_ab.txt).
static int run_pvq_quantize(escx_handle_s* h, const Quant& q, const float* enc, const float* dec, int B, int W, long long* codes, long long bstride,
                            float* loss, float* out, hipStream_t st) {
    const escx_config& c = h->cfg;
    if (h->pvq_fused) {
        const int Tq = W / c.overlap, M = B * Tq;
        const double vec = (double)c.overlap * q.Hq * q.C;
        int frc = -1;
        PROF(out ? "pvq_fused" : "pvq_fused_codes", 2.0 * M * vec * q.d * (out ? 2 : 1) + 2.0 * M * c.group_size * c.codebook_size * q.d,
             (double)M * vec * ((dec ? 2 : 1) + (out ? (dec ? 2 : 1) : 0)) * 4,
             frc = pvq_fused(enc, dec, B, q.Hq, W, q.Cp, c.overlap, q.wdf, q.Nz, q.Kq, pvq_down_splits(M, q.Kq, q.Cp), pvq_down_bk(q.Cp), q.cbn, q.c2, q.cbraw,
                             c.group_size, c.codebook_size, q.d, q.dt, q.wup, q.tab, q.gq, out, codes, bstride, loss, pvq_loss_scale(h, q, Tq), c.l2norm, st));
        if (frc == 0) return launch_ok("pvq_quantize");
        if (h->prof && !h->prof_recs.empty()) h->prof_recs.pop_back();
    }
    int rc;
    if ((rc = run_pvq_encode(h, q, enc, dec, B, W, codes, bstride, loss, st))) return rc;
    if (out && (rc = run_pvq_decode(h, q, codes, bstride, dec, B, W, out, st))) return rc;
    return 0;
}

static int run_deembed(escx_handle_s* h, const float* tok, int B, int W, float* rspec, hipStream_t st) {   // scale.py:73-81
    const escx_config& c = h->cfg;
    const int H0 = c.in_freq / c.patch_f;
    if (h->len) {
        // Mixed-length batch: the convolutions zero-pad at the clip's own W_b.  The dead columns of the input are stored as zeros, the composed 7x7 runs on the
        // padded maps as it is (its interior form is exact up to column W_b - 2), and the border pass recomputes the clip's own last column with the variants.
        if (h->deembed_two_stage || c.in_dim * h->Q > 16) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "mixed-length batches run the composed de-embedding only (in_dim * patch area <= 16, ESCX_DEEMBED_TWO_STAGE unset)");
        const double tk = (double)B * H0 * W;
        PROF("deembed_zero_dead", 0, tk * h->C0p * 4, zero_dead_cols(const_cast<float*>(tok), h->len->d_W, B, H0, W, h->C0p, st));
        int hrc = -1;
        if (h->deembed_halo)
            PROF("deembed_composed7x7", 2.0 * tk * 49 * h->C0 * c.in_dim * h->Q, (tk * h->C0 + tk * c.in_dim * h->Q) * 4,
                 hrc = deembed7_fused(tok, B, H0, W, h->C0p, h->dch_w, h->dcc_b, rspec, c.patch_f, c.patch_t, c.in_dim, h->Fp, st, h->dch_x2));
        if (hrc != 0)
        PROF("deembed_composed7x7", 2.0 * tk * 49 * h->C0 * c.in_dim * h->Q, (tk * h->C0 + tk * c.in_dim * h->Q) * 4,
             gemm_deembed_composed(tok, B, H0, W, h->C0p, h->dcc_w, rspec, h->dcc_b, c.patch_f, c.patch_t, c.in_dim, h->Fp, st));
        int brc = 0;
        PROF("deembed_border_len", 0, 0,
             brc = deembed_border_len(tok, h->dcv_w, h->dcv_b, rspec, h->len->d_W, B, H0, W, h->C0, h->C0p, c.patch_f, c.patch_t, c.in_dim, h->Fp, st));
        if (brc != 0) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "mixed-length batches: no border kernel for %d de-embedding outputs", c.in_dim * h->Q);
        return launch_ok("patch_deembed");
    }
    if (!h->deembed_two_stage && c.in_dim * h->Q <= 16) {
        const double tk = (double)B * H0 * W;
        int hrc = -1;
        if (h->deembed_halo)
            PROF("deembed_composed7x7", 2.0 * tk * 49 * h->C0 * c.in_dim * h->Q, (tk * h->C0 + tk * c.in_dim * h->Q) * 4,
                 hrc = deembed7_fused(tok, B, H0, W, h->C0p, h->dch_w, h->dcc_b, rspec, c.patch_f, c.patch_t, c.in_dim, h->Fp, st, h->dch_x2));
        if (hrc != 0)
        PROF("deembed_composed7x7", 2.0 * tk * 49 * h->C0 * c.in_dim * h->Q, (tk * h->C0 + tk * c.in_dim * h->Q) * 4,
             gemm_deembed_composed(tok, B, H0, W, h->C0p, h->dcc_w, rspec, h->dcc_b, c.patch_f, c.patch_t, c.in_dim, h->Fp, st));
        int brc = 0;
        PROF("deembed_border", 0, 0,
             brc = deembed_border(tok, h->dcv_w, h->dcv_b, rspec, B, H0, W, h->C0, h->C0p, c.patch_f, c.patch_t, c.in_dim, h->Fp, st));
        if (brc == 0) return launch_ok("patch_deembed");
    }
    const double toks = (double)B * H0 * W, pix = toks * h->Q;
    PROF("deembed_conv5x5", 2.0 * toks * 25 * h->C0 * h->C0 * h->Q, (toks * h->C0 + pix * h->C0) * 4,
         gemm_conv_deembed1(tok, B, H0, W, h->C0p, h->dc1_w, h->Q * h->C0p, h->deemb, h->dc1_b, c.patch_f, c.patch_t, st));
    PROF("deembed_conv3x3", 2.0 * pix * 9 * h->C0 * c.in_dim, (pix * h->C0 + pix * c.in_dim) * 4,
         gemm_conv_spec(h->deemb, B, c.patch_t * W, c.patch_f * H0, h->C0p, h->dc2_w, rspec, h->dc2_b, h->Fp, c.in_dim, st));
    return launch_ok("patch_deembed");
}

static int run_istft(escx_handle_s* h, const float* rspec, int B, int T2, float* wave, hipStream_t st) {  // base.py:39-47
    const escx_config& c = h->cfg;
    PROF("istft_idft_gemm", 2.0 * B * T2 * c.win_length * 2 * h->F, (double)B * T2 * (2 * h->F + c.win_length) * 4,
         gemm_store(rspec, c.in_dim * h->Fp, B * T2, h->idft_w, h->winP, c.in_dim * h->Fp, h->frames, h->winP, nullptr, st));
    if (h->len) {       // mixed-length batch: each clip overlap-adds its own patch_t * W_b frames; zeros past hop * (patch_t * W_b - 1)
        PROF("istft_overlap_add_len", 0, (double)B * T2 * c.win_length * 4 + (double)B * c.hop_length * (T2 - 1) * 4,
             istft_ola_len(h->frames, h->win2, wave, h->len->d_W, c.patch_t, B, T2, h->winP, c.win_length, c.hop_length, h->left, h->n_fft / 2, c.hop_length * (T2 - 1), st));
        return launch_ok("istft");
    }
    PROF("istft_overlap_add", 0, (double)B * T2 * c.win_length * 4 + (double)B * c.hop_length * (T2 - 1) * 4,
         istft_ola(h->frames, h->win2, wave, B, T2, h->winP, c.win_length, c.hop_length, h->left, h->n_fft / 2, c.hop_length * (T2 - 1), st));
    return launch_ok("istft");
}

// frame-major padded spectrum [rows][in_dim*Fp] <-> reference-ordered [rows][in_dim][F]
static void spec_unpad(escx_handle_s* h, const float* src, float* dst, long long rows, hipStream_t st) {
    unpad_rows(src, dst, rows * h->cfg.in_dim, h->F, h->Fp, st);
}
static void spec_pad(escx_handle_s* h, const float* src, float* dst, long long rows, hipStream_t st) {
    pad_rows(src, dst, rows * h->cfg.in_dim, h->F, h->Fp, st);
}

extern "C" int escx_num_frames(escx_handle h, int n_samples) { return h ? 1 + n_samples / h->cfg.hop_length : 0; }
extern "C" int escx_output_samples(escx_handle h, int feat_w) { return h ? h->cfg.hop_length * (h->cfg.patch_t * feat_w - 1) : 0; }

// rvq+swinT handles (escx_create_rvq): the whole-path entry points below dispatch to these (defined after the mixed-stream section).
// streams: HOST per-clip counts or nullptr (= S for every clip).
static int rvq_encode(escx_handle_s* h, const float* wave, int B, int L, const int32_t* streams, int S, int64_t* codes, int* fh, int* fw, void* stream);
static int rvq_decode(escx_handle_s* h, const int64_t* codes, int B, int S, const int32_t* streams, int fh, int fw, float* wave_out, float* recon_feat, void* stream);
static int rvq_forward(escx_handle_s* h, const float* wave, const float* feat, int B, int LT, const int32_t* streams, int S, int64_t* codes, float* wave_out,
                       float* raw_feat, float* recon_feat, float* cm_loss, void* stream);

// Argument checks that several entry points share: each issues its message in one place.
static int check_count(const char* what, int S, int max, const char* suffix = "") {
    if (S < 1 || S > max) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "%s=%d outside [1, %d]%s", what, S, max, suffix);
    return 0;
}
static int check_samples(escx_handle_s* h, int L) {
    if (L <= h->n_fft / 2) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "n_samples=%d too short for reflect padding of %d", L, h->n_fft / 2);
    return 0;
}
static int fail_overlap() { ESCX_FAIL(ESCX_ERR_ASSERT, "Time dimension must be multiple of overlap"); }
static int check_feat_shape(escx_handle_s* h, const Shapes& s, int fh, int fw) {
    if (s.W != fw || s.encH[h->n - 1] != fh) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "feat_shape (%d,%d) does not match the model (%d,%d)", fh, fw, s.encH[h->n - 1], s.W);
    return 0;
}
// frames of a forward call's input: LT samples (long enough for the reflect padding) or LT frames (at least one patch)
static int input_frames(escx_handle_s* h, bool wave, int LT, int* T) {
    if (wave) { const int rc = check_samples(h, LT); *T = frames_of(h, LT); return rc; }
    if (LT < h->cfg.patch_t) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "n_frames=%d shorter than one patch", LT);
    *T = LT;
    return 0;
}

// Input of the pass [b0, b0 + nb): waveforms (B, L) through the STFT, or frame-major spectra `feat` (B, T, in_dim, F) padded, into h->spec; `raw_feat`
// (optional) receives the spectrum in the reference's order.
static int stage_input(escx_handle_s* h, const float* wave, const float* feat, int b0, int nb, int L, int T, float* raw_feat, hipStream_t st) {
    const size_t row = (size_t)T * h->cfg.in_dim * h->F;
    int rc;
    if (wave) { if ((rc = run_stft(h, wave + (size_t)b0 * L, nb, L, T, h->spec, st))) return rc; }
    else spec_pad(h, feat + b0 * row, h->spec, (long long)nb * T, st);
    if (raw_feat) spec_unpad(h, h->spec, raw_feat + b0 * row, (long long)nb * T, st);
    return 0;
}
// Output of the pass [b0, b0 + nb): h->rspec (T2 frames per clip) through the inverse STFT into wave_out; `recon_feat` (optional) receives the spectrum.
static int finish_output(escx_handle_s* h, int b0, int nb, int T2, float* wave_out, float* recon_feat, hipStream_t st) {
    const escx_config& c = h->cfg;
    int rc;
    if ((rc = run_istft(h, h->rspec, nb, T2, wave_out + (size_t)b0 * c.hop_length * (T2 - 1), st))) return rc;
    if (recon_feat) spec_unpad(h, h->rspec, recon_feat + (size_t)b0 * T2 * c.in_dim * h->F, (long long)nb * T2, st);
    return 0;
}

static int clips_over(const int* S, int B, int j) { int c = 0; while (c < B && S[c] > j) ++c; return c; }     // S non-increasing

// Stream counts of one pass of a whole-path call: the pass's clips in workspace order with S[0] >= S[1] >= ... (mixed-stream calls: MixPlan::S_ws), or
// S == nullptr and every clip carries `uniform` streams.  Stream j then runs on a PREFIX of the pass - the same kernels on a smaller batch.
namespace {
struct PassStreams {
    const int* S; int uniform;
    int over(int nb, int j) const { return S ? clips_over(S, nb, j) : (j < uniform ? nb : 0); }      // of the pass's first nb clips, those that carry stream j
};
}  // namespace

// csrvq.py:131-158: stream j runs on the clips that carry it; the refinement after it and the decoder block that feeds stream j + 1 only on those that
// carry stream j + 1 as well (csrvq.py:151: a clip's last stream only emits codes).
static int run_csvq_encode(escx_handle_s* h, const Shapes& s, PassStreams ps, long long* codes, long long bstride, hipStream_t st) {
    const int n = h->n;
    const long long sstride = (long long)h->cfg.group_size * s.Tq;
    int rc, H = s.encH[n - 1], Hn;
    float* dec = h->decA; float* other = h->decB;
    int nref = ps.over(s.B, 1);                                           // clips that go on to stream 1
    if ((rc = run_pvq_quantize(h, h->quants[0], h->enc_hs[n - 1], nullptr, s.B, s.W, codes, bstride, nullptr, nref ? dec : nullptr, st))) return rc;
    for (int i = 0; nref > 0; ++i) {
        const int nq = nref;                                              // clips that carry stream i + 1
        nref = ps.over(nq, i + 2);                                        // ... and stream i + 2: they need the refinement and block i
        if ((rc = run_pvq_quantize(h, h->quants[i + 1], h->enc_hs[n - 1 - i], dec, nq, s.W, codes + (i + 1) * sstride, bstride, nullptr, nref ? dec : nullptr, st))) return rc;
        if (!nref) break;
        if ((rc = run_layer(h, h->layers[n + i], dec, other, nref, H, s.W, &Hn, st))) return rc;
        std::swap(dec, other); H = Hn;
    }
    return 0;
}

// csrvq.py:160-183 + codecs.py:83-94: stream i + 1 is de-quantised and added in place on the clips that carry it; the others keep `dec` (the reference's
// pass-through).  Every decoder block runs on the whole pass.  codes == nullptr with no refinement streams ({nullptr, 1}): the bottleneck map is in
// h->decA already and the walk is Decoder.forward (base.py:195-203: blocks, post_nn, PatchDeEmbed), the rvq codec's decoder.
static int run_csvq_decode(escx_handle_s* h, const long long* codes, long long bstride, int B, PassStreams ps, int Hb, int W, float* rspec, hipStream_t st) {
    const int n = h->n;
    const long long sstride = (long long)h->cfg.group_size * (W / h->cfg.overlap);
    int rc, H = Hb, Hn;
    float* dec = h->decA; float* other = h->decB;
    if (codes && (rc = run_pvq_decode(h, h->quants[0], codes, bstride, nullptr, B, W, dec, st))) return rc;
    for (int i = 0; i + 1 < n; ++i) {
        const int nq = ps.over(B, i + 1);
        if (nq && (rc = run_pvq_decode(h, h->quants[i + 1], codes + (i + 1) * sstride, bstride, dec, nq, W, dec, st))) return rc;
        if ((rc = run_layer(h, h->layers[n + i], dec, other, B, H, W, &Hn, st))) return rc;
        std::swap(dec, other); H = Hn;
    }
    if ((rc = run_layer(h, h->layers[2 * n - 1], dec, other, B, H, W, &Hn, st))) return rc;
    return run_deembed(h, other, B, W, rspec, st);
}

// csrvq.py:97-129 in eval mode + codecs.py:83-94: stream 0, then (stream i + 1, block i) pairs; stream i + 1 quantises the clips that carry it, the
// others pass through.  slot_clips[j] = the clips that ran stream slot j; its per-vector commitment terms go to loss + j * G * s.B * Tq as
// [G][slot_clips[j] * Tq] (loss may be null) and are reduced per clip by the caller (no atomics).
static int run_csvq_forward(escx_handle_s* h, const Shapes& s, PassStreams ps, long long* codes, long long bstride, float* loss, int slot_clips[8],
                            float* rspec, hipStream_t st) {
    const int n = h->n;
    const long long sstride = (long long)h->cfg.group_size * s.Tq;
    const size_t lslot = (size_t)sstride * s.B;
    int rc, H = s.encH[n - 1], Hn;
    float* dec = h->decA; float* other = h->decB;
    std::fill(slot_clips, slot_clips + 8, 0);
    slot_clips[0] = s.B;
    if ((rc = run_pvq_quantize(h, h->quants[0], h->enc_hs[n - 1], nullptr, s.B, s.W, codes, bstride, loss, dec, st))) return rc;
    for (int i = 0; i + 1 < n; ++i) {
        const int nq = ps.over(s.B, i + 1);
        if (nq) {
            if ((rc = run_pvq_quantize(h, h->quants[i + 1], h->enc_hs[n - 1 - i], dec, nq, s.W, codes + (i + 1) * sstride, bstride, loss ? loss + (size_t)(i + 1) * lslot : nullptr, dec, st))) return rc;
            slot_clips[i + 1] = nq;
        }
        if ((rc = run_layer(h, h->layers[n + i], dec, other, s.B, H, s.W, &Hn, st))) return rc;
        std::swap(dec, other); H = Hn;
    }
    if ((rc = run_layer(h, h->layers[2 * n - 1], dec, other, s.B, H, s.W, &Hn, st))) return rc;
    return run_deembed(h, other, s.B, s.W, rspec, st);
}
static int slots_used(const int* slot_clips) { int k = 0; while (k < 8 && slot_clips[k]) ++k; return k; }     // a uniform pass: slots 0 .. min(S, n) - 1

extern "C" int escx_encode(escx_handle h, const float* wave, int B, int L, int S, int64_t* codes, int* fh, int* fw, void* stream) {
    if (h && h->kind == 1) return rvq_encode(h, wave, B, L, nullptr, S, codes, fh, fw, stream);
    int rc = check_ready(h); if (rc) return rc;
    if (!wave || !codes) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    if ((rc = check_count("num_streams", S, h->cfg.max_streams))) return rc;
    if ((rc = check_samples(h, L))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, frames_of(h, L), &s))) return rc;
    const long long cstride = (long long)S * h->cfg.group_size * s.Tq;
    if ((rc = ensure_pvq_tables(h, (hipStream_t)stream))) return rc;
    rc = run_halves(h, B, s.T, (hipStream_t)stream, [&](int b0, int nb, hipStream_t st) -> int {
        Shapes sp = s; sp.B = nb; int r;
        if ((r = run_stft(h, wave + (size_t)b0 * L, nb, L, sp.T, h->spec, st))) return r;
        if ((r = run_encoder(h, sp, st))) return r;
        return run_csvq_encode(h, sp, {nullptr, S}, (long long*)codes + b0 * cstride, cstride, st);
    });
    if (rc) return rc;
    if (fh) *fh = s.encH[h->n - 1];
    if (fw) *fw = s.W;
    return ESCX_OK;
}

extern "C" int escx_decode(escx_handle h, const int64_t* codes, int B, int S, int fh, int fw, float* wave_out, float* recon_feat,
                           void* stream) {
    if (h && h->kind == 1) return rvq_decode(h, codes, B, S, nullptr, fh, fw, wave_out, recon_feat, stream);
    int rc = check_infer_ready(h); if (rc) return rc;
    if (!codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    if ((rc = check_count("codes.size(1)", S, c.max_streams))) return rc;
    if (fw < 1 || fw % c.overlap) return fail_overlap();
    Shapes s; if ((rc = ensure_ws(h, B, frames_for_width(h, fw), &s))) return rc;
    if ((rc = check_feat_shape(h, s, fh, fw))) return rc;
    const int T2 = c.patch_t * fw;
    const long long cstride = (long long)S * c.group_size * (fw / c.overlap);
    if ((rc = ensure_pvq_tables(h, (hipStream_t)stream))) return rc;
    rc = run_halves(h, B, s.T, (hipStream_t)stream, [&](int b0, int nb, hipStream_t st) -> int {
        int r;
        if ((r = run_csvq_decode(h, (const long long*)codes + b0 * cstride, cstride, nb, {nullptr, S}, fh, fw, h->rspec, st))) return r;
        if ((r = finish_output(h, b0, nb, T2, wave_out, recon_feat, st))) return r;
        return launch_ok("decode");
    });
    return rc;
}

// codecs.py:30-66 in eval mode.  Exactly one of `wave` (B, L) and `feat` (B, T, in_dim, F: the reference's x_feat (B,F,T,2)
// permuted to frame-major) is given; with `feat` the STFT is skipped (codecs.py:33-34).
static int forward_impl(escx_handle h, const float* wave, const float* feat, int B, int LT, int S, int64_t* codes, float* wave_out,
                        float* raw_feat, float* recon_feat, float* cm_loss, void* stream) {
    if (h && h->kind == 1) return rvq_forward(h, wave, feat, B, LT, nullptr, S, codes, wave_out, raw_feat, recon_feat, cm_loss, stream);
    int rc = check_infer_ready(h); if (rc) return rc;
    if ((!wave && !feat) || !codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    if ((rc = check_count("num_streams", S, c.max_streams))) return rc;
    int T; if ((rc = input_frames(h, wave != nullptr, LT, &T))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, T, &s))) return rc;
    if (s.W % c.overlap) return fail_overlap();
    const int G = c.group_size, T2 = c.patch_t * s.W;
    const long long bstride = (long long)S * G * s.Tq;
    if ((rc = ensure_pvq_tables(h, (hipStream_t)stream))) return rc;
    return run_halves(h, B, s.T, (hipStream_t)stream, [&](int b0, int nb, hipStream_t st) -> int {
        Shapes sp = s; sp.B = nb; int r;
        if ((r = stage_input(h, wave, feat, b0, nb, LT, sp.T, raw_feat, st))) return r;
        if ((r = run_encoder(h, sp, st))) return r;
        float* loss = cm_loss ? h->loss_terms : nullptr;
        int slot_clips[8];
        if ((r = run_csvq_forward(h, sp, {nullptr, S}, (long long*)codes + b0 * bstride, bstride, loss, slot_clips, h->rspec, st))) return r;
        if ((r = finish_output(h, b0, nb, T2, wave_out, recon_feat, st))) return r;
        if (cm_loss) loss_reduce(loss, slots_used(slot_clips), G, nb * sp.Tq, sp.Tq, cm_loss + b0, st);
        return launch_ok("forward");
    });
}

extern "C" int escx_forward(escx_handle h, const float* wave, int B, int L, int S, int64_t* codes, float* wave_out, float* raw_feat,
                            float* recon_feat, float* cm_loss, void* stream) {
    if (!wave) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    return forward_impl(h, wave, nullptr, B, L, S, codes, wave_out, raw_feat, recon_feat, cm_loss, stream);
}

extern "C" int escx_forward_feat(escx_handle h, const float* feat, int B, int T, int S, int64_t* codes, float* wave_out, float* recon_feat,
                                 float* cm_loss, void* stream) {
    if (!feat) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    return forward_impl(h, nullptr, feat, B, T, S, codes, wave_out, nullptr, recon_feat, cm_loss, stream);
}

// ------------------------------------------------------------------------------------------------
// Mixed-stream batches: escx_encode_streams / escx_decode_streams / escx_forward_streams (include/escx.h).  Clip b carries its own stream
// count S_b.  A clip's codes and audio do not depend on the batch it runs in, streams are a prefix of the S = max_streams codes, and
// untransmitted streams pass through (csrvq.py:174-177), so every clip gets exactly what a uniform call at its S_b returns.
// The clips are laid into WORKSPACE ORDER so that every pass of every part (run_halves) holds its clips sorted by descending S: stream j
// (and the decoder block that feeds stream j + 1) then runs on a PREFIX of the pass - the same fused kernels on a smaller batch.
// ------------------------------------------------------------------------------------------------
namespace {
struct MixPlan {
    int B = 0, Smax = 0;
    std::vector<int32_t> ints;       // [ws2b | b2ws | S in workspace order | S in caller order], uploaded as one block
    const int32_t* S_ws() const { return ints.data() + 2 * B; }
};
}  // namespace

// HOST per-clip counts, each in [1, max] (`suffix` names the bound in the message: "" = max_streams, " (num_rvqs)"); *Smax = the largest
static int check_streams(int B, const int32_t* streams, int max, const char* suffix, int* Smax) {
    if (!streams) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null streams pointer");
    if (B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d: the per-clip stream counts need at least one clip", B);
    int m = 0;
    for (int b = 0; b < B; ++b) {
        if (streams[b] < 1 || streams[b] > max) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "streams[%d]=%d outside [1, %d]%s", b, streams[b], max, suffix);
        m = std::max(m, (int)streams[b]);
    }
    *Smax = m;
    return 0;
}

// Sort the clips by S (descending, stable) and deal them round-robin over the passes of all parts, in the order run_halves enqueues them:
// each pass receives non-increasing S, and the parts (streams) get the same mix of stream counts.
static void plan_streams(escx_handle_s* h, int B, int T, const int32_t* streams, int Smax, MixPlan* p) {
    int k, per, pass;
    part_layout(h, B, T, &k, &per, &pass);
    std::vector<std::pair<int, int>> groups;           // (first workspace position, clips) of every pass
    for (int off = 0; off < per; off += pass)
        for (int i = 0; i < std::max(k, 1); ++i) {
            const int b0 = i * per, nb = std::min(per, B - b0);
            if (nb <= off) continue;
            groups.push_back({b0 + off, std::min(pass, nb - off)});
        }
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return streams[a] > streams[b]; });
    p->B = B; p->Smax = Smax;
    p->ints.assign((size_t)4 * B, 0);
    int32_t *ws2b = p->ints.data(), *b2ws = ws2b + B, *Sws = ws2b + 2 * B, *Sb = ws2b + 3 * B;
    int next = 0;
    for (int r = 0; next < B; ++r)
        for (const auto& g : groups)
            if (r < g.second && next < B) ws2b[g.first + r] = order[next++];
    for (int w = 0; w < B; ++w) { b2ws[ws2b[w]] = w; Sws[w] = streams[ws2b[w]]; }
    for (int b = 0; b < B; ++b) Sb[b] = streams[b];
}

// Bump allocation in the handle's grow-only staging buffer (mix_buf); growing synchronises the device once (earlier calls may still read it).
namespace {
struct MixBufs {
    size_t used = 0;
    std::vector<std::pair<void**, size_t>> want;
    template <class T> void add(T** p, size_t n) { want.push_back({reinterpret_cast<void**>(p), n * sizeof(T)}); }
};
}  // namespace
static int mix_alloc(escx_handle_s* h, MixBufs& m) {
    size_t total = 0;
    for (auto& w : m.want) total += (w.second + 255) / 256 * 256;
    if (total > h->mix_cap) {
        ESCX_HIP(hipDeviceSynchronize());
        if (h->mix_buf) { (void)hipFree(h->mix_buf); h->mix_buf = nullptr; h->mix_cap = 0; }
        ESCX_HIP(hipMalloc(&h->mix_buf, total));
        h->mix_cap = total;
    }
    char* base = static_cast<char*>(h->mix_buf);
    for (auto& w : m.want) { *w.first = w.second ? base : nullptr; base += (w.second + 255) / 256 * 256; }
    return 0;
}

static int upload_plan(escx_handle_s* h, const MixPlan& p, int32_t* dev, hipStream_t st) {
    ESCX_HIP(hipMemcpyAsync(dev, p.ints.data(), p.ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    return 0;
}

extern "C" int escx_encode_streams(escx_handle h, const float* wave, int B, int L, const int32_t* streams, int64_t* codes, int* fh, int* fw,
                                   void* stream) {
    if (h && h->kind == 1) return rvq_encode(h, wave, B, L, streams, 0, codes, fh, fw, stream);
    int rc = check_ready(h); if (rc) return rc;
    if (!wave || !codes) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    int Smax = 0; if ((rc = check_streams(B, streams, h->cfg.max_streams, "", &Smax))) return rc;
    if ((rc = check_samples(h, L))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, frames_of(h, L), &s))) return rc;
    MixPlan p; plan_streams(h, B, s.T, streams, Smax, &p);
    const int GT = h->cfg.group_size * s.Tq;
    const long long cstride = (long long)Smax * GT;
    int32_t* maps; float* wave_ws; long long* codes_ws;
    MixBufs mb; mb.add(&maps, p.ints.size()); mb.add(&wave_ws, (size_t)B * L); mb.add(&codes_ws, (size_t)B * cstride);
    if ((rc = mix_alloc(h, mb))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    if ((rc = upload_plan(h, p, maps, st))) return rc;
    PROF("mix_gather", 0, 2.0 * B * L * 4, rows_permute(wave, wave_ws, maps, B, L, st));
    rc = run_halves(h, B, s.T, st, [&](int b0, int nb, hipStream_t sti) -> int {
        Shapes sp = s; sp.B = nb; int r;
        if ((r = run_stft(h, wave_ws + (size_t)b0 * L, nb, L, sp.T, h->spec, sti))) return r;
        if ((r = run_encoder(h, sp, sti))) return r;
        return run_csvq_encode(h, sp, {p.S_ws() + b0, 0}, codes_ws + b0 * cstride, cstride, sti);
    });
    if (rc) return rc;
    PROF("mix_scatter", 0, 2.0 * B * cstride * 8, codes_permute(codes_ws, cstride, (long long*)codes, maps + B, maps + 3 * B, B, Smax, GT, st));
    if ((rc = launch_ok("encode_streams"))) return rc;
    if (fh) *fh = s.encH[h->n - 1];
    if (fw) *fw = s.W;
    return ESCX_OK;
}

extern "C" int escx_decode_streams(escx_handle h, const int64_t* codes, int B, int Smax_in, const int32_t* streams, int fh, int fw, float* wave_out,
                                   float* recon_feat, void* stream) {
    if (h && h->kind == 1) return rvq_decode(h, codes, B, Smax_in, streams, fh, fw, wave_out, recon_feat, stream);
    int rc = check_infer_ready(h); if (rc) return rc;
    if (!codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    int Smax = 0; if ((rc = check_streams(B, streams, c.max_streams, "", &Smax))) return rc;
    if (Smax_in < Smax || Smax_in > c.max_streams) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "codes.size(1)=%d: must lie in [max(streams)=%d, %d]", Smax_in, Smax, c.max_streams);
    if (fw < 1 || fw % c.overlap) return fail_overlap();
    Shapes s; if ((rc = ensure_ws(h, B, frames_for_width(h, fw), &s))) return rc;
    if ((rc = check_feat_shape(h, s, fh, fw))) return rc;
    MixPlan p; plan_streams(h, B, s.T, streams, Smax, &p);
    const int T2 = c.patch_t * fw, out_len = c.hop_length * (T2 - 1), GT = c.group_size * (fw / c.overlap);
    const long long in_stride = (long long)Smax_in * GT, cstride = (long long)Smax * GT, frow = (long long)T2 * c.in_dim * h->F;
    int32_t* maps; long long* codes_ws; float *wave_ws, *recon_ws = nullptr;
    MixBufs mb; mb.add(&maps, p.ints.size()); mb.add(&codes_ws, (size_t)B * cstride); mb.add(&wave_ws, (size_t)B * out_len);
    if (recon_feat) mb.add(&recon_ws, (size_t)B * frow);
    if ((rc = mix_alloc(h, mb))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    if ((rc = upload_plan(h, p, maps, st))) return rc;
    // workspace-order codes: only slots below S_b are read from the caller's tensor (the rest is filled with -1 and never read either)
    PROF("mix_gather", 0, 2.0 * B * cstride * 8, codes_permute((const long long*)codes, in_stride, codes_ws, maps, maps + 2 * B, B, Smax, GT, st));
    rc = run_halves(h, B, s.T, st, [&](int b0, int nb, hipStream_t sti) -> int {
        int r;
        if ((r = run_csvq_decode(h, codes_ws + b0 * cstride, cstride, nb, {p.S_ws() + b0, 0}, fh, fw, h->rspec, sti))) return r;
        if ((r = finish_output(h, b0, nb, T2, wave_ws, recon_ws, sti))) return r;
        return launch_ok("decode_streams");
    });
    if (rc) return rc;
    PROF("mix_scatter", 0, 2.0 * B * out_len * 4, rows_permute(wave_ws, wave_out, maps + B, B, out_len, st));
    if (recon_feat) PROF("mix_scatter", 0, 2.0 * B * frow * 4, rows_permute(recon_ws, recon_feat, maps + B, B, frow, st));
    return launch_ok("decode_streams");
}

// codecs.py:30-66 in eval mode with per-clip stream counts; forward_impl is the uniform form.  Exactly one of `wave` / `feat` is given.
extern "C" int escx_forward_streams(escx_handle h, const float* wave, const float* feat, int B, int LT, const int32_t* streams, int64_t* codes,
                                    float* wave_out, float* raw_feat, float* recon_feat, float* cm_loss, void* stream) {
    if (h && h->kind == 1) return rvq_forward(h, wave, feat, B, LT, streams, 0, codes, wave_out, raw_feat, recon_feat, cm_loss, stream);
    int rc = check_infer_ready(h); if (rc) return rc;
    if ((!wave == !feat) || !codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer (exactly one of wave / feat, codes and wave_out are required)");
    const escx_config& c = h->cfg;
    int Smax = 0; if ((rc = check_streams(B, streams, c.max_streams, "", &Smax))) return rc;
    int T; if ((rc = input_frames(h, wave != nullptr, LT, &T))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, T, &s))) return rc;
    if (s.W % c.overlap) return fail_overlap();
    MixPlan p; plan_streams(h, B, s.T, streams, Smax, &p);
    const int n = h->n, G = c.group_size, GT = G * s.Tq;
    const long long cstride = (long long)Smax * GT;
    const int T2 = c.patch_t * s.W, out_len = c.hop_length * (T2 - 1);
    const long long in_row = wave ? (long long)LT : (long long)s.T * c.in_dim * h->F, raw_row = (long long)s.T * c.in_dim * h->F, rec_row = (long long)T2 * c.in_dim * h->F;
    int32_t* maps; float *in_ws, *wave_ws, *raw_ws = nullptr, *recon_ws = nullptr, *loss_ws = nullptr; long long* codes_ws;
    MixBufs mb; mb.add(&maps, p.ints.size()); mb.add(&in_ws, (size_t)B * in_row); mb.add(&codes_ws, (size_t)B * cstride); mb.add(&wave_ws, (size_t)B * out_len);
    if (raw_feat) mb.add(&raw_ws, (size_t)B * raw_row);
    if (recon_feat) mb.add(&recon_ws, (size_t)B * rec_row);
    if (cm_loss) mb.add(&loss_ws, (size_t)B);
    if ((rc = mix_alloc(h, mb))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    if ((rc = upload_plan(h, p, maps, st))) return rc;
    PROF("mix_gather", 0, 2.0 * B * in_row * 4, rows_permute(wave ? wave : feat, in_ws, maps, B, in_row, st));
    const int32_t* Sdev = maps + 2 * B;
    rc = run_halves(h, B, s.T, st, [&](int b0, int nb, hipStream_t st) -> int {
        Shapes sp = s; sp.B = nb; int r;
        if ((r = stage_input(h, wave ? in_ws : nullptr, in_ws, b0, nb, LT, sp.T, raw_ws, st))) return r;
        if ((r = run_encoder(h, sp, st))) return r;
        float* loss = cm_loss ? h->loss_terms : nullptr;
        int slot_clips[8];
        if ((r = run_csvq_forward(h, sp, {p.S_ws() + b0, 0}, codes_ws + b0 * cstride, cstride, loss, slot_clips, h->rspec, st))) return r;
        if ((r = finish_output(h, b0, nb, T2, wave_ws, recon_ws, st))) return r;
        // every clip is reduced over its own slots
        if (cm_loss) PROF("loss_reduce_streams", 0, (double)nb * Smax * GT * 4, loss_reduce_streams(loss, (long long)GT * nb, Sdev + b0, n, slot_clips, G, sp.Tq, nb, loss_ws + b0, st));
        return launch_ok("forward_streams");
    });
    if (rc) return rc;
    PROF("mix_scatter", 0, 2.0 * B * cstride * 8, codes_permute(codes_ws, cstride, (long long*)codes, maps + B, maps + 3 * B, B, Smax, GT, st));
    PROF("mix_scatter", 0, 2.0 * B * out_len * 4, rows_permute(wave_ws, wave_out, maps + B, B, out_len, st));
    if (raw_feat) PROF("mix_scatter", 0, 2.0 * B * raw_row * 4, rows_permute(raw_ws, raw_feat, maps + B, B, raw_row, st));
    if (recon_feat) PROF("mix_scatter", 0, 2.0 * B * rec_row * 4, rows_permute(recon_ws, recon_feat, maps + B, B, rec_row, st));
    if (cm_loss) PROF("mix_scatter", 0, 8.0 * B, rows_permute(loss_ws, cm_loss, maps + B, B, 1, st));
    return launch_ok("forward_streams");
}

// ------------------------------------------------------------------------------------------------
// Mixed-length batches: escx_encode_lengths / escx_decode_lengths / escx_forward_lengths (include/escx.h).  Clip b has L_b samples, i.e. W_b latent
// columns, and gets what the plain call on x[b, :L_b] alone computes: the batch keeps the padded layout (B, H * Wmax, Cp), every row-wise kernel runs on
// it unchanged, and the stages that are coupled along time (STFT framing, window attention, de-embedding borders, overlap-add, loss reduction) read the
// per-clip tables (len_kernels.h, fused_attn.h LEN).  The batch runs as ONE part on the caller's stream, and every variant choice is made from Wmax and the
// precision mode - never from B or the other lengths - so that a clip's result is a function of its own samples, L_b, Wmax, num_streams and the mode.
// ------------------------------------------------------------------------------------------------
namespace {
struct LenGuard {                   // the context is visible to the launch sequences for the duration of the call only
    escx_handle_s* h;
    LenGuard(escx_handle_s* h_, const LenCtx* c) : h(h_) { h->len = c; }
    ~LenGuard() { h->len = nullptr; }
};
}  // namespace

static int len_common_checks(escx_handle_s* h, int B, const int32_t* v, const char* what) {
    if (h->kind == 1) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "mixed-length batches are not implemented for the rvq+swinT codec (RVQCodecs)");
    if (h->ws != 4) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "mixed-length batches are implemented for window_size 4 only (this model: %d)", h->ws);
    if (!v) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null %s pointer", what);
    if (B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch=%d: the per-clip %s need at least one clip", B, what);
    return 0;
}
static int check_one_set(escx_handle_s* h, int B, int T) {      // the batch runs as one part: workspace set 0 has to hold all of it
    const auto& w = h->sets[0].shp;
    if (w.B < B || w.T < T) ESCX_FAIL(ESCX_ERR_STATE, "workspace set holds %d clips of %d frames, the batch needs %d of %d", w.B, w.T, B, T);
    return 0;
}

// samples per clip -> latent widths; every L_b in (n_fft / 2, Lx], every W_b a multiple of `overlap`
static int plan_lengths(escx_handle_s* h, int B, int Lx, const int32_t* lengths, LenCtx* lc, int* Lmax) {
    const escx_config& c = h->cfg;
    lc->B = B; lc->W.assign(B, 0); lc->Wmax = 0; *Lmax = 0;
    for (int b = 0; b < B; ++b) {
        const int L = lengths[b];
        if (L <= h->n_fft / 2 || L > Lx) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "lengths[%d]=%d outside (%d, %d] (reflect padding of %d, row length %d)", b, L, h->n_fft / 2, Lx, h->n_fft / 2, Lx);
        const int W = frames_of(h, L) / c.patch_t;
        if (W < 1 || W % c.overlap) ESCX_FAIL(ESCX_ERR_ASSERT, "Time dimension must be multiple of overlap (clip %d: %d samples give %d latent frames)", b, L, W);
        lc->W[b] = W; lc->Wmax = std::max(lc->Wmax, W); *Lmax = std::max(*Lmax, L);
    }
    return 0;
}

// uploads [W_b | L_b] into the staging buffer (after `extra` bytes of other staging the caller asked for through mb)
static int upload_lengths(escx_handle_s* h, MixBufs& mb, LenCtx* lc, const int32_t* lengths, hipStream_t st) {
    int32_t* tab = nullptr;
    mb.add(&tab, (size_t)2 * lc->B);
    int rc = mix_alloc(h, mb); if (rc) return rc;
    ESCX_HIP(hipMemcpyAsync(tab, lc->W.data(), (size_t)lc->B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    lc->d_W = tab;
    if (lengths) { ESCX_HIP(hipMemcpyAsync(tab + lc->B, lengths, (size_t)lc->B * sizeof(int32_t), hipMemcpyHostToDevice, st)); lc->d_L = tab + lc->B; }
    return 0;
}

extern "C" int escx_encode_lengths(escx_handle h, const float* wave, int B, int Lx, const int32_t* lengths, int S, int64_t* codes, int* fh, int* fw, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if ((rc = len_common_checks(h, B, lengths, "lengths"))) return rc;
    if (!wave || !codes) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    if ((rc = check_count("num_streams", S, c.max_streams))) return rc;
    LenCtx lc; int Lmax = 0;
    if ((rc = plan_lengths(h, B, Lx, lengths, &lc, &Lmax))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, frames_of(h, Lmax), &s, B))) return rc;
    if ((rc = check_one_set(h, B, s.T))) return rc;
    hipStream_t st = (hipStream_t)stream;
    MixBufs mb; if ((rc = upload_lengths(h, mb, &lc, lengths, st))) return rc;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    use_set(h, 0);
    LenGuard guard(h, &lc);
    if ((rc = run_stft(h, wave, B, Lx, s.T, h->spec, st))) return rc;
    if ((rc = run_encoder(h, s, st))) return rc;
    if ((rc = run_csvq_encode(h, s, {nullptr, S}, (long long*)codes, (long long)S * c.group_size * s.Tq, st))) return rc;
    PROF("codes_mask_len", 0, 8.0 * B * S * c.group_size * s.Tq, codes_mask_len((const long long*)codes, (long long*)codes, lc.d_W, c.overlap, B, S * c.group_size, s.Tq, -1, st));
    if ((rc = launch_ok("encode_lengths"))) return rc;
    if (fh) *fh = s.encH[h->n - 1];
    if (fw) *fw = s.W;
    return ESCX_OK;
}

// widths per clip for decode: each a positive multiple of `overlap`, at most fw
static int plan_widths(escx_handle_s* h, int B, int fw, const int32_t* widths, LenCtx* lc) {
    lc->B = B; lc->W.assign(widths, widths + B); lc->Wmax = fw;
    for (int b = 0; b < B; ++b) {
        if (widths[b] < 1 || widths[b] > fw) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "frame_lengths[%d]=%d outside [1, %d]", b, widths[b], fw);
        if (widths[b] % h->cfg.overlap) ESCX_FAIL(ESCX_ERR_ASSERT, "Time dimension must be multiple of overlap (clip %d: %d latent frames)", b, widths[b]);
    }
    return 0;
}

extern "C" int escx_decode_lengths(escx_handle h, const int64_t* codes, int B, int S, const int32_t* widths, int fh, int fw, float* wave_out, float* recon_feat,
                                   void* stream) {
    int rc = check_infer_ready(h); if (rc) return rc;
    if ((rc = len_common_checks(h, B, widths, "frame_lengths"))) return rc;
    if (!codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    if ((rc = check_count("codes.size(1)", S, c.max_streams))) return rc;
    if (fw < 1 || fw % c.overlap) return fail_overlap();
    LenCtx lc;
    if ((rc = plan_widths(h, B, fw, widths, &lc))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, frames_for_width(h, fw), &s, B))) return rc;
    if ((rc = check_one_set(h, B, s.T))) return rc;
    if ((rc = check_feat_shape(h, s, fh, fw))) return rc;
    const int T2 = c.patch_t * fw, Tq = fw / c.overlap;
    hipStream_t st = (hipStream_t)stream;
    long long* codes_ws = nullptr;
    MixBufs mb; mb.add(&codes_ws, (size_t)B * S * c.group_size * Tq);
    if ((rc = upload_lengths(h, mb, &lc, nullptr, st))) return rc;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    use_set(h, 0);
    LenGuard guard(h, &lc);
    // the clip's own code frames are copied; the slots past them are not read (the copy holds code 0 there, which feeds dead tokens only)
    PROF("codes_mask_len", 0, 16.0 * B * S * c.group_size * Tq, codes_mask_len((const long long*)codes, codes_ws, lc.d_W, c.overlap, B, S * c.group_size, Tq, 0, st));
    if ((rc = run_csvq_decode(h, codes_ws, (long long)S * c.group_size * Tq, B, {nullptr, S}, fh, fw, h->rspec, st))) return rc;
    if ((rc = run_istft(h, h->rspec, B, T2, wave_out, st))) return rc;
    if (recon_feat) PROF("unpad_len", 0, 2.0 * B * T2 * c.in_dim * h->F * 4, unpad_rows_len(h->rspec, recon_feat, lc.d_W, 1, c.patch_t, c.hop_length, B, T2, c.in_dim, h->F, h->Fp, st));
    return launch_ok("decode_lengths");
}

// codecs.py:30-66 in eval mode on a mixed-length batch (forward_impl is the uniform form): raw_feat (B, Tmax, in_dim, F) with Tmax = 1 + max(L_b) / hop
extern "C" int escx_forward_lengths(escx_handle h, const float* wave, int B, int Lx, const int32_t* lengths, int S, int64_t* codes, float* wave_out,
                                    float* raw_feat, float* recon_feat, float* cm_loss, void* stream) {
    int rc = check_infer_ready(h); if (rc) return rc;
    if ((rc = len_common_checks(h, B, lengths, "lengths"))) return rc;
    if (!wave || !codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    if ((rc = check_count("num_streams", S, c.max_streams))) return rc;
    LenCtx lc; int Lmax = 0;
    if ((rc = plan_lengths(h, B, Lx, lengths, &lc, &Lmax))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, frames_of(h, Lmax), &s, B))) return rc;
    if ((rc = check_one_set(h, B, s.T))) return rc;
    hipStream_t st = (hipStream_t)stream;
    MixBufs mb; if ((rc = upload_lengths(h, mb, &lc, lengths, st))) return rc;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    use_set(h, 0);
    LenGuard guard(h, &lc);
    const int G = c.group_size, T2 = c.patch_t * s.W;
    const long long bstride = (long long)S * G * s.Tq;
    long long* cd = (long long*)codes;
    if ((rc = run_stft(h, wave, B, Lx, s.T, h->spec, st))) return rc;
    if (raw_feat) PROF("unpad_len", 0, 2.0 * B * s.T * c.in_dim * h->F * 4, unpad_rows_len(h->spec, raw_feat, lc.d_L, 0, c.patch_t, c.hop_length, B, s.T, c.in_dim, h->F, h->Fp, st));
    if ((rc = run_encoder(h, s, st))) return rc;
    float* loss = cm_loss ? h->loss_terms : nullptr;
    int slot_clips[8];
    if ((rc = run_csvq_forward(h, s, {nullptr, S}, cd, bstride, loss, slot_clips, h->rspec, st))) return rc;
    if ((rc = run_istft(h, h->rspec, B, T2, wave_out, st))) return rc;
    if (recon_feat) PROF("unpad_len", 0, 2.0 * B * T2 * c.in_dim * h->F * 4, unpad_rows_len(h->rspec, recon_feat, lc.d_W, 1, c.patch_t, c.hop_length, B, T2, c.in_dim, h->F, h->Fp, st));
    const int n_slots = slots_used(slot_clips);
    const size_t lslot = (size_t)G * B * s.Tq;
    if (cm_loss) PROF("loss_reduce_len", 0, (double)n_slots * lslot * 4, loss_reduce_len(loss, lc.d_W, c.overlap, n_slots, G, B, s.Tq, cm_loss, st));
    PROF("codes_mask_len", 0, 8.0 * B * bstride, codes_mask_len(cd, cd, lc.d_W, c.overlap, B, S * G, s.Tq, -1, st));
    return launch_ok("forward_lengths");
}

// ------------------------------------------------------------------------------------------------
// rvq+swinT (RVQCodecs, codecs.py:96-181): the ESC encoder, ONE product-residual quantiser at the bottleneck (fused_prvq.h: one launch per batch
// part, per-clip stage counts read on the device) and the plain decoder (base.py:161-203: every decoder block, post_nn, PatchDeEmbed).  Nothing
// of the decoder depends on the stage count, so a mixed-count batch needs no clip permutation: the per-clip counts go to the quantiser only.
// ------------------------------------------------------------------------------------------------
static int run_prvq(escx_handle_s* h, const float* enc, const long long* codes_in, int B, int W, long long* codes, long long bstride, const int* clip_S,
                    int S, float* loss, long long lslot, float* out, hipStream_t st) {
    const escx_config& c = h->cfg;
    const Quant& q = h->quants[0];
    const int Tq = W / c.overlap, M = B * Tq;
    const double vec = (double)c.overlap * q.Hq * q.C, G = c.group_size;
    int rc = -1;
    PROF(codes_in ? "prvq_decode" : (out ? "prvq_fused" : "prvq_fused_codes"),
         codes_in ? 2.0 * M * vec * q.d : 2.0 * M * vec * q.d * (out ? 2 : 1) + 2.0 * M * S * G * c.codebook_size * q.d,
         (double)M * vec * ((codes_in ? 0 : 1) + (out ? 1 : 0)) * 4,
         rc = prvq_fused(enc, codes_in, B, q.Hq, W, q.Cp, c.overlap, q.wdf, q.Nz, q.Kq, pvq_down_splits(M, q.Kq, q.Cp), pvq_down_bk(q.Cp), q.cbn, q.c2, q.cbraw,
                         c.group_size, c.codebook_size, q.d, q.dt, q.wup, codes, bstride, clip_S, S, S, loss, lslot, 1.0f / ((float)Tq * q.d * c.group_size),
                         c.l2norm, out, st));
    if (rc) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "rvq quantiser: geometry not covered (codebook_dim %d, %d groups)", q.d, c.group_size);
    return launch_ok("prvq");
}

// Decoder.forward (base.py:195-203) on the bottleneck map h->decA: blocks, post_nn, PatchDeEmbed -> rspec (the decode walk without quantiser streams)
static int run_plain_decoder(escx_handle_s* h, int B, int Hb, int W, float* rspec, hipStream_t st) {
    return run_csvq_decode(h, nullptr, 0, B, {nullptr, 1}, Hb, W, rspec, st);
}

// stage counts of an rvq call: per clip (streams != nullptr) in [1, num_rvqs], or one S in [1, num_rvqs]; *Smax = the code slots per clip
static int rvq_counts(escx_handle_s* h, int B, const int32_t* streams, int S, int* Smax) {
    if (streams) return check_streams(B, streams, h->num_rvqs, " (num_rvqs)", Smax);
    *Smax = S;
    return check_count("num_streams", S, h->num_rvqs, " (num_rvqs)");
}

// per-clip counts on the device (the handle's grow-only staging buffer), or nullptr for a uniform call
static int rvq_upload(escx_handle_s* h, int B, const int32_t* streams, const int** dev, hipStream_t st) {
    *dev = nullptr;
    if (!streams) return 0;
    int32_t* d = nullptr;
    MixBufs mb; mb.add(&d, (size_t)B);
    int rc = mix_alloc(h, mb); if (rc) return rc;
    ESCX_HIP(hipMemcpyAsync(d, streams, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st));
    *dev = d;
    return 0;
}

static int rvq_encode(escx_handle_s* h, const float* wave, int B, int L, const int32_t* streams, int S, int64_t* codes, int* fh, int* fw, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!wave || !codes) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    int Smax = 0; if ((rc = rvq_counts(h, B, streams, S, &Smax))) return rc;
    if ((rc = check_samples(h, L))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, frames_of(h, L), &s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int* Sdev; if ((rc = rvq_upload(h, B, streams, &Sdev, st))) return rc;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    const long long cstride = (long long)Smax * h->cfg.group_size * s.Tq;
    rc = run_halves(h, B, s.T, st, [&](int b0, int nb, hipStream_t sti) -> int {
        Shapes sp = s; sp.B = nb; int r;
        if ((r = run_stft(h, wave + (size_t)b0 * L, nb, L, sp.T, h->spec, sti))) return r;
        if ((r = run_encoder(h, sp, sti))) return r;
        return run_prvq(h, h->enc_hs[h->n - 1], nullptr, nb, sp.W, (long long*)codes + b0 * cstride, cstride, Sdev ? Sdev + b0 : nullptr, Smax, nullptr, 0, nullptr, sti);
    });
    if (rc) return rc;
    if (fh) *fh = s.encH[h->n - 1];
    if (fw) *fw = s.W;
    return ESCX_OK;
}

// S = codes.size(1); streams (optional) = per-clip counts, each <= S (slots at or past a clip's count are never read)
static int rvq_decode(escx_handle_s* h, const int64_t* codes, int B, int S, const int32_t* streams, int fh, int fw, float* wave_out, float* recon_feat, void* stream) {
    int rc = check_infer_ready(h); if (rc) return rc;
    if (!codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    const escx_config& c = h->cfg;
    if ((rc = check_count("codes.size(1)", S, h->num_rvqs, " (num_rvqs)"))) return rc;
    int Smax = 0; if ((rc = rvq_counts(h, B, streams, S, &Smax))) return rc;
    if (Smax > S) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "codes.size(1)=%d: must be at least max(streams)=%d", S, Smax);
    if (fw < 1 || fw % c.overlap) return fail_overlap();
    Shapes s; if ((rc = ensure_ws(h, B, frames_for_width(h, fw), &s))) return rc;
    if ((rc = check_feat_shape(h, s, fh, fw))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int* Sdev; if ((rc = rvq_upload(h, B, streams, &Sdev, st))) return rc;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    const int T2 = c.patch_t * fw;
    const long long cstride = (long long)S * c.group_size * (fw / c.overlap);
    return run_halves(h, B, s.T, st, [&](int b0, int nb, hipStream_t sti) -> int {
        int r;
        if ((r = run_prvq(h, nullptr, (const long long*)codes + b0 * cstride, nb, fw, nullptr, cstride, Sdev ? Sdev + b0 : nullptr, S, nullptr, 0, h->decA, sti))) return r;
        if ((r = run_plain_decoder(h, nb, fh, fw, h->rspec, sti))) return r;
        if ((r = finish_output(h, b0, nb, T2, wave_out, recon_feat, sti))) return r;
        return launch_ok("rvq_decode");
    });
}

// codecs.py:130-146 in eval mode; exactly one of wave (LT = n_samples) / feat (LT = n_frames)
static int rvq_forward(escx_handle_s* h, const float* wave, const float* feat, int B, int LT, const int32_t* streams, int S, int64_t* codes, float* wave_out,
                       float* raw_feat, float* recon_feat, float* cm_loss, void* stream) {
    int rc = check_infer_ready(h); if (rc) return rc;
    if ((!wave == !feat) || !codes || !wave_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer (exactly one of wave / feat, codes and wave_out are required)");
    const escx_config& c = h->cfg;
    int Smax = 0; if ((rc = rvq_counts(h, B, streams, S, &Smax))) return rc;
    int T; if ((rc = input_frames(h, wave != nullptr, LT, &T))) return rc;
    Shapes s; if ((rc = ensure_ws(h, B, T, &s))) return rc;
    if (s.W % c.overlap) return fail_overlap();
    hipStream_t st = (hipStream_t)stream;
    const int* Sdev; if ((rc = rvq_upload(h, B, streams, &Sdev, st))) return rc;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    const int G = c.group_size, T2 = c.patch_t * s.W;
    const long long cstride = (long long)Smax * G * s.Tq;
    return run_halves(h, B, s.T, st, [&](int b0, int nb, hipStream_t sti) -> int {
        Shapes sp = s; sp.B = nb; int r;
        if ((r = stage_input(h, wave, feat, b0, nb, LT, sp.T, raw_feat, sti))) return r;
        if ((r = run_encoder(h, sp, sti))) return r;
        // per-vector commitment terms of stage s go to loss_terms[s][G][nb * Tq] (0 past a clip's own count); reduced per clip in a fixed order
        const long long lslot = (long long)G * nb * sp.Tq;
        float* loss = cm_loss ? h->loss_terms : nullptr;
        if ((r = run_prvq(h, h->enc_hs[h->n - 1], nullptr, nb, sp.W, (long long*)codes + b0 * cstride, cstride, Sdev ? Sdev + b0 : nullptr, Smax, loss, lslot, h->decA, sti))) return r;
        if ((r = run_plain_decoder(h, nb, sp.encH[h->n - 1], sp.W, h->rspec, sti))) return r;
        if ((r = finish_output(h, b0, nb, T2, wave_out, recon_feat, sti))) return r;
        if (cm_loss) PROF("loss_reduce", 0, (double)lslot * Smax * 4, loss_reduce(loss, Smax, G, nb * sp.Tq, sp.Tq, cm_loss + b0, sti));
        return launch_ok("rvq_forward");
    });
}

// ------------------------------------------------------------------------------------------------
// stage-level entry points (reference layouts in and out)
// ------------------------------------------------------------------------------------------------
extern "C" int escx_spec_transform(escx_handle h, const float* wave, int B, int L, float* spec, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!wave || !spec || B < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    if ((rc = check_samples(h, L))) return rc;
    const int T = frames_of(h, L);
    TmpBuf t; if (t.alloc((size_t)B * T * h->cfg.in_dim * h->Fp)) ESCX_FAIL(ESCX_ERR_HIP, "hipMalloc failed");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_stft(h, wave, B, L, T, t.p, st))) return rc;
    spec_unpad(h, t.p, spec, (long long)B * T, st);
    return launch_ok("spec_transform");
}

extern "C" int escx_audio_reconstruct(escx_handle h, const float* spec, int B, int T, float* wave, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (!spec || !wave || B < 1 || T < 2) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument (need at least 2 frames)");
    TmpBuf ts, tf;
    if (ts.alloc((size_t)B * T * h->cfg.in_dim * h->Fp) || tf.alloc((size_t)B * T * h->winP)) ESCX_FAIL(ESCX_ERR_HIP, "hipMalloc failed");
    hipStream_t st = (hipStream_t)stream;
    const escx_config& c = h->cfg;
    spec_pad(h, spec, ts.p, (long long)B * T, st);
    gemm_store(ts.p, c.in_dim * h->Fp, B * T, h->idft_w, h->winP, c.in_dim * h->Fp, tf.p, h->winP, nullptr, st);
    istft_ola(tf.p, h->win2, wave, B, T, h->winP, c.win_length, c.hop_length, h->left, h->n_fft / 2, c.hop_length * (T - 1), st);
    return launch_ok("audio_reconstruct");
}

extern "C" int escx_patch_embed(escx_handle h, const float* spec, int B, int T, float* tokens, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    const escx_config& c = h->cfg;
    const int W = T / c.patch_t, H0 = c.in_freq / c.patch_f;
    if (!spec || !tokens || B < 1 || W < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    TmpBuf ts, tt;
    if (ts.alloc((size_t)B * T * c.in_dim * h->Fp) || tt.alloc((size_t)B * H0 * W * h->C0p)) ESCX_FAIL(ESCX_ERR_HIP, "hipMalloc failed");
    hipStream_t st = (hipStream_t)stream;
    spec_pad(h, spec, ts.p, (long long)B * T, st);
    if ((rc = run_patch_embed(h, ts.p, B, T, W, tt.p, st))) return rc;
    unpad_rows(tt.p, tokens, (long long)B * H0 * W, h->C0, h->C0p, st);
    return launch_ok("patch_embed");
}

// stage-level calls run the whole batch on set 0, so ask for a workspace whose HALF holds B clips
static int stage_ws_for_w(escx_handle_s* h, int B, int W, Shapes* s) {
    int rc = ensure_ws(h, h->parts * B, frames_for_width(h, W), s, B);
    if (!rc) s->B = B;
    return rc;
}

extern "C" int escx_transformer_layer(escx_handle h, int layer_id, const float* x, int B, int H, int W, float* y, int* H_out, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (layer_id < 0 || layer_id >= 2 * h->n) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "layer_id out of range");
    const Layer& L = h->layers[layer_id];
    Shapes s; if ((rc = stage_ws_for_w(h, B, W, &s))) return rc;
    if ((size_t)H > (size_t)2 * s.H0) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "H too large for this model");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    int Hn;
    // stage buffers are sized for the largest map of the model; H*Cp never exceeds that for valid (layer, H) pairs
    const size_t need = (size_t)B * H * W * L.Cp, cap = std::max<size_t>((size_t)B * s.H0 * s.W * h->C0p, 1);
    size_t big = 0; for (int i = 0; i < h->n; ++i) big = std::max(big, (size_t)B * s.encH[i] * s.W * rup(h->cfg.h_dims[i], 16));
    if (need > std::max(cap, big)) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "(H=%d, W=%d) is larger than any map of this layer", H, W);
    pad_rows(x, h->stageA, (long long)B * H * W, L.C, L.Cp, st);
    if ((rc = run_layer(h, L, h->stageA, h->stageB, B, H, W, &Hn, st))) return rc;
    unpad_rows(h->stageB, y, (long long)B * Hn * W, L.scale ? L.Cout : L.C, L.scale ? L.CoutP : L.Cp, st);
    if (H_out) *H_out = Hn;
    return launch_ok("transformer_layer");
}

extern "C" int escx_pvq_encode(escx_handle h, int sid, const float* enc, const float* dec, int B, int W, int64_t* codes, int64_t bstride,
                               void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (h->kind != 0) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "escx_pvq_encode: the cross-scale quantisers do not exist on an rvq handle (escx_rvq_encode / escx_rvq_decode)");
    if (sid < 0 || sid >= h->cfg.max_streams) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "stream_id out of range");
    if (W % h->cfg.overlap) return fail_overlap();
    const Quant& q = h->quants[sid];
    Shapes s; if ((rc = stage_ws_for_w(h, B, W, &s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * q.Hq * W;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    pad_rows(enc, h->stageA, rows, q.C, q.Cp, st);
    if (dec) pad_rows(dec, h->stageB, rows, q.C, q.Cp, st);
    return run_pvq_quantize(h, q, h->stageA, dec ? h->stageB : nullptr, B, W, (long long*)codes, bstride, nullptr, nullptr, st);
}

extern "C" int escx_pvq_decode(escx_handle h, int sid, const int64_t* codes, int64_t bstride, const float* dec, int B, int W, float* out,
                               void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (h->kind != 0) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "escx_pvq_decode: the cross-scale quantisers do not exist on an rvq handle (escx_rvq_encode / escx_rvq_decode)");
    if (sid < 0 || sid >= h->cfg.max_streams) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "stream_id out of range");
    if (W % h->cfg.overlap) return fail_overlap();
    const Quant& q = h->quants[sid];
    Shapes s; if ((rc = stage_ws_for_w(h, B, W, &s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * q.Hq * W;
    if ((rc = ensure_pvq_tables(h, st))) return rc;
    if (dec) pad_rows(dec, h->stageB, rows, q.C, q.Cp, st);
    if ((rc = run_pvq_decode(h, q, (const long long*)codes, bstride, dec ? h->stageB : nullptr, B, W, h->stageA, st))) return rc;
    unpad_rows(h->stageA, out, rows, q.C, q.Cp, st);
    return launch_ok("pvq_decode");
}

// ProductResidualVectorQuantize.encode / eval forward on bottleneck tokens in the reference layout (include/escx.h)
extern "C" int escx_rvq_encode(escx_handle h, const float* tokens, int B, int W, int S, int64_t* codes, float* zq_out, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (h->kind != 1) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "escx_rvq_encode needs an rvq handle (escx_create_rvq)");
    if (!tokens || !codes) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    if (B < 1 || W < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch and W must be positive");
    if ((rc = check_count("num_streams", S, h->num_rvqs, " (num_rvqs)"))) return rc;
    if (W % h->cfg.overlap) return fail_overlap();
    const Quant& q = h->quants[0];
    Shapes s; if ((rc = stage_ws_for_w(h, B, W, &s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long rows = (long long)B * q.Hq * W;
    pad_rows(tokens, h->stageA, rows, q.C, q.Cp, st);
    if ((rc = run_prvq(h, h->stageA, nullptr, B, W, (long long*)codes, (long long)S * h->cfg.group_size * (W / h->cfg.overlap), nullptr, S, nullptr, 0,
                       zq_out ? h->stageB : nullptr, st))) return rc;
    if (zq_out) unpad_rows(h->stageB, zq_out, rows, q.C, q.Cp, st);
    return launch_ok("rvq_encode");
}

// ProductResidualVectorQuantize.decode (include/escx.h)
extern "C" int escx_rvq_decode(escx_handle h, const int64_t* codes, int B, int S, int W, float* tokens_out, void* stream) {
    int rc = check_ready(h); if (rc) return rc;
    if (h->kind != 1) ESCX_FAIL(ESCX_ERR_UNSUPPORTED, "escx_rvq_decode needs an rvq handle (escx_create_rvq)");
    if (!codes || !tokens_out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    if (B < 1 || W < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "batch and W must be positive");
    if ((rc = check_count("codes.size(1)", S, h->num_rvqs, " (num_rvqs)"))) return rc;
    if (W % h->cfg.overlap) return fail_overlap();
    const Quant& q = h->quants[0];
    Shapes s; if ((rc = stage_ws_for_w(h, B, W, &s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_prvq(h, nullptr, (const long long*)codes, B, W, nullptr, (long long)S * h->cfg.group_size * (W / h->cfg.overlap), nullptr, S, nullptr, 0,
                       h->stageA, st))) return rc;
    unpad_rows(h->stageA, tokens_out, (long long)B * q.Hq * W, q.C, q.Cp, st);
    return launch_ok("rvq_decode");
}

extern "C" int escx_patch_deembed(escx_handle h, const float* tokens, int B, int W, float* spec, void* stream) {
    int rc = check_infer_ready(h); if (rc) return rc;
    Shapes s; if ((rc = stage_ws_for_w(h, B, W, &s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    pad_rows(tokens, h->stageA, (long long)B * s.H0 * W, h->C0, h->C0p, st);
    if ((rc = run_deembed(h, h->stageA, B, W, h->rspec, st))) return rc;
    spec_unpad(h, h->rspec, spec, (long long)B * h->cfg.patch_t * W, st);
    return launch_ok("patch_deembed");
}

extern "C" int escx_debug_mlp_trace(unsigned long long* dev_buf) { mlp_set_trace(dev_buf); return 0; }
extern "C" int escx_test_fastdiv(int n, int d) { return test_fastdiv(n, d); }
extern "C" int escx_test_math(const float* x, float* y, int64_t n, int which, void* stream) {
    test_math(x, y, n, which, (hipStream_t)stream);
    return launch_ok("test_math");
}
extern "C" int escx_test_copy_rows(const float* src, float* dst, int64_t rows, int row_floats, void* stream) {
    if (!src || !dst || rows < 1 || row_floats < 4 || row_floats % 4) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    test_copy_rows(src, dst, rows, row_floats, (hipStream_t)stream);
    return launch_ok("test_copy_rows");
}
extern "C" int escx_codes_pack10(const int64_t* codes, uint8_t* out, int64_t n, void* stream) {
    if (!codes || !out || n < 0) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    codes_pack10((const long long*)codes, out, n, (hipStream_t)stream);
    return launch_ok("codes_pack10");
}
extern "C" int escx_codes_unpack10(const uint8_t* in, int64_t* codes, int64_t n, void* stream) {
    if (!codes || !in || n < 0) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    codes_unpack10(in, (long long*)codes, n, (hipStream_t)stream);
    return launch_ok("codes_unpack10");
}
// Ragged 10-bit packing of a mixed-stream batch: clip b's first streams[b] * gt codes of (batch, smax, gt), compacted in clip order.
static int ragged_offsets(int B, int Smax, int64_t gt, const int32_t* streams, hipStream_t st, const long long** off_dev, long long* n) {
    if (!streams || B < 1 || Smax < 1 || gt < 1) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "bad argument");
    std::vector<long long> off((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
        if (streams[b] < 1 || streams[b] > Smax) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "streams[%d]=%d outside [1, %d]", b, streams[b], Smax);
        off[b + 1] = off[b] + (long long)streams[b] * gt;
    }
    long long* d = reinterpret_cast<long long*>(stream_scratch(st, 2, 2 * off.size()));
    if (!d) ESCX_FAIL(ESCX_ERR_HIP, "scratch allocation failed");
    ESCX_HIP(hipMemcpyAsync(d, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    *off_dev = d; *n = off[B];
    return 0;
}
extern "C" int escx_codes_pack10_streams(const int64_t* codes, int B, int Smax, int64_t gt, const int32_t* streams, uint8_t* out, void* stream) {
    if (!codes || !out) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long* off; long long n; int rc;
    if ((rc = ragged_offsets(B, Smax, gt, streams, st, &off, &n))) return rc;
    codes_pack10_streams((const long long*)codes, out, off, B, (long long)Smax * gt, n, st);
    return launch_ok("codes_pack10_streams");
}
extern "C" int escx_codes_unpack10_streams(const uint8_t* in, int B, int Smax, int64_t gt, const int32_t* streams, int64_t* codes, void* stream) {
    if (!codes || !in) ESCX_FAIL(ESCX_ERR_INVALID_ARG, "null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long* off; long long n; int rc;
    if ((rc = ragged_offsets(B, Smax, gt, streams, st, &off, &n))) return rc;
    codes_unpack10_streams(in, (long long*)codes, off, B, (long long)Smax * gt, st);
    return launch_ok("codes_unpack10_streams");
}
extern "C" int escx_codes_narrow(const int64_t* codes, int16_t* out, int64_t n, void* stream) {
    codes_narrow((const long long*)codes, (short*)out, n, (hipStream_t)stream);
    return launch_ok("codes_narrow");
}
extern "C" int escx_codes_widen(const int16_t* in, int64_t* codes, int64_t n, void* stream) {
    codes_widen((const short*)in, (long long*)codes, n, (hipStream_t)stream);
    return launch_ok("codes_widen");
}

