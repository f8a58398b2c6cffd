// Launchers for the fused (wave-autonomous, register-resident) Swin kernels.
#include "fused_attn.h"
#include "fused_mlp.h"
#include "fused_mlp_x3.h"
#include <atomic>
#include "fused_rowgemm.h"
#include "fused_deembed.h"
#include "launchers.h"

namespace escx {

template <int CP, int TM>
static void launch_mlp(const MlpArgs& a, hipStream_t s) {
    const int waves = (a.M + 16 * TM - 1) / (16 * TM);
    ESCX_LAUNCH((mlp_fused_kernel<CP, TM>), dim3((waves + 3) / 4), dim3(256), 0, s, a);
}

template <int CP, int TM, int NW>
static void launch_mlp_lds(const MlpArgs& a, hipStream_t s) {
    const int rows = 16 * TM * NW;
    const int hs = a.HS > 1 ? a.HS : 1;
    ESCX_LAUNCH((mlp_fused_lds_kernel<CP, TM, NW>), dim3(((a.M + rows - 1) / rows) * hs), dim3(64 * NW), 0, s, a);
}

// variant: 0 = wave-autonomous; otherwise LDS-staged, one row tile per wave: 1 = 4 waves, 3 = 8 waves per workgroup
template <int CP>
static int launch_mlp_lds_variant(int variant, const MlpArgs& a, hipStream_t s) {
    switch (variant) {
        case 1: launch_mlp_lds<CP, 1, 4>(a, s); return 0;
        case 3: launch_mlp_lds<CP, 1, 8>(a, s); return 0;
        default: return -1;
    }
}

static unsigned long long* g_mlp_trace = nullptr;      // debug only (phase-trace builds of the attention kernels): 8 x u64 per wave, see fused_attn.h
void mlp_set_trace(unsigned long long* p) { g_mlp_trace = p; }
unsigned long long* debug_trace_buffer() { return g_mlp_trace; }

void rows_combine(float* dst, const float* src, const float* partial, const float* bias, long long M, int Cp, int n, hipStream_t s) {
    const long long n4 = M * Cp / 4;
    ESCX_LAUNCH(rows_combine_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dst, src, partial, bias, M, Cp, n);
}

// *hs: requested hidden split in, split actually used out (> 1: x is untouched, partial[hs][M][Cp] is filled, the caller runs rows_combine)
template <int CP, int NW>
static void launch_mlp_split(const MlpArgs& a, hipStream_t s) {
    const int rows = 16 * NW;
    ESCX_LAUNCH((mlp_fused_lds_kernel<CP, 1, NW, true>), dim3((a.M + rows - 1) / rows), dim3(64 * NW), 0, s, a);
}

int mlp_fused(float* x, int M, int C, int Cp, const float* gamma, const float* beta, const float* w1f, const float* b1,
              const float* w2f, const float* b2, const float* wcf, int hiddenP, int variant, int* hs_io, float* partial, hipStream_t s, float* out,
              const MlpSplit* split) {
    if (split) {        // PatchSplit in the epilogue: the widths whose MLP is not hidden-split (ESC: C = 144, 96, 72), plain 4- / 8-wave variants
        const int hs0 = hs_io ? *hs_io : 1;
        if (hs0 > 1 || out || (variant != 1 && variant != 3) || (split->NT & 1) || !(Cp == 80 || Cp == 96 || Cp == 144)) return ESCX_COMB_UNSUPPORTED;
        MlpArgs a{x, gamma, beta, reinterpret_cast<const f32x4*>(w1f), b1, reinterpret_cast<const f32x4*>(w2f), b2,
                  reinterpret_cast<const f32x4*>(wcf), M, C, hiddenP / 16, 1e-5f, 1, nullptr, nullptr,
                  reinterpret_cast<const f32x4*>(split->wf), split->gamma, split->beta, split->out, split->NT, split->H, split->W, split->C2p};
        const bool nw8 = variant == 3;
        switch (Cp) {
            case 80: if (nw8) launch_mlp_split<80, 8>(a, s); else launch_mlp_split<80, 4>(a, s); return 0;
            case 96: if (nw8) launch_mlp_split<96, 8>(a, s); else launch_mlp_split<96, 4>(a, s); return 0;
            case 144: if (nw8) launch_mlp_split<144, 8>(a, s); else launch_mlp_split<144, 4>(a, s); return 0;
        }
        return ESCX_COMB_UNSUPPORTED;
    }
    int hs = hs_io ? *hs_io : 1;
    const bool lds_width = Cp == 48 || Cp == 80 || Cp == 96 || Cp == 144 || Cp == 192 || Cp == 384;
    if (hs > 1 && (variant <= 0 || variant > 3 || !lds_width || !partial || (hiddenP / 16) % hs)) hs = 1;
    if (hs_io) *hs_io = hs;
    MlpArgs a{x, gamma, beta, reinterpret_cast<const f32x4*>(w1f), b1, reinterpret_cast<const f32x4*>(w2f), b2,
              reinterpret_cast<const f32x4*>(wcf), M, C, hiddenP / 16, 1e-5f, hs, partial, out,
              nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
    if (out && hs > 1) return -1;       // a separate output: plain epilogues only (no hidden split)
    if (variant > 0) {
        switch (Cp) {
            case 48: return launch_mlp_lds_variant<48>(variant, a, s);
            case 80: return launch_mlp_lds_variant<80>(variant, a, s);
            case 96: return launch_mlp_lds_variant<96>(variant, a, s);
            case 144: return launch_mlp_lds_variant<144>(variant, a, s);
            case 192: return launch_mlp_lds_variant<192>(variant, a, s);
            case 384: return launch_mlp_lds_variant<384>(variant, a, s);
            default: break;     // fall through to the wave-autonomous kernel
        }
    }
    switch (Cp) {
        case 16: launch_mlp<16, 4>(a, s); return 0;
        case 32: launch_mlp<32, 4>(a, s); return 0;
        case 48: launch_mlp<48, 4>(a, s); return 0;
        case 64: launch_mlp<64, 4>(a, s); return 0;
        case 80: launch_mlp<80, 4>(a, s); return 0;
        case 96: launch_mlp<96, 2>(a, s); return 0;
        case 112: launch_mlp<112, 2>(a, s); return 0;
        case 128: launch_mlp<128, 2>(a, s); return 0;
        case 144: launch_mlp<144, 2>(a, s); return 0;
        case 160: launch_mlp<160, 2>(a, s); return 0;
        case 192: launch_mlp<192, 2>(a, s); return 0;
        case 256: launch_mlp<256, 1>(a, s); return 0;
        case 288: launch_mlp<288, 1>(a, s); return 0;
        case 384: launch_mlp<384, 1>(a, s); return 0;
        default: return -1;
    }
}

// ---- fused MLP, fp32 operands split into three bf16 terms (fused_mlp_x3.h) ----
// nt = 3: three bf16 terms per operand (exact split); nt = 2: two fp16 terms + per-matrix power-of-two scales in a 32-byte trailer (fused_mlp_x3.h)
// nt = 2 also carries the pre-scaled fc1 bias [hiddenP] and LayerNorm gamma / beta [Cp] each behind the trailer (mlp_x3_prescale_kernel)
static size_t mlp_x3_frag_bytes(int Cp, int hiddenP, int nt) { return (size_t)(hiddenP / 32) * mlp_x3_frags(Cp, nt) * 1024; }
size_t mlp_x3_bytes(int Cp, int hiddenP, int nt) { return mlp_x3_frag_bytes(Cp, hiddenP, nt) + 48 + (nt == 2 ? (size_t)(hiddenP + 2 * Cp) * sizeof(float) : 0); }

int mlp_x3_pack(const float* w1, const float* w2, void* image, int Cp, int hiddenP, hipStream_t s, int nt, const float* gamma, const float* beta, const float* b1, int C) {
    if (Cp % 16 || hiddenP % 32 || (nt != 2 && nt != 3)) return -1;
    if (nt == 2 && (!gamma || !beta || !b1)) return -1;             // the two-term image holds scaled copies of all three
    char* tail = reinterpret_cast<char*>(image) + mlp_x3_frag_bytes(Cp, hiddenP, nt);
    const int KS = (Cp + 31) / 32, KK = Cp / 16;
    const long long total = (long long)(hiddenP / 32) * (2 * KS + KK) * 64;
    if (nt == 2) {
        unsigned* mx = reinterpret_cast<unsigned*>(tail);
        if (hipMemsetAsync(mx, 0, 16, s) != hipSuccess) return -1;
        const long long n = (long long)hiddenP * Cp;
        ESCX_LAUNCH(absmax_bits_kernel, dim3((unsigned)std::min<long long>(256, (n + 255) / 256)), dim3(256), 0, s, w1, n, mx);
        ESCX_LAUNCH(absmax_bits_kernel, dim3((unsigned)std::min<long long>(256, (n + 255) / 256)), dim3(256), 0, s, w2, n, mx + 1);
        ESCX_LAUNCH(rownorm2_max_bits_kernel, dim3((unsigned)((hiddenP + 3) / 4)), dim3(256), 0, s, w1, hiddenP, Cp, Cp, mx + 2);      // range rule: bound of the fc1 outputs
    }
    ESCX_LAUNCH(mlp_x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w1, w2, reinterpret_cast<bf16x8*>(image), Cp, hiddenP, KS, KK, nt, gamma, beta, b1, C);
    if (nt == 2) ESCX_LAUNCH(mlp_x3_prescale_kernel, dim3((unsigned)((hiddenP + 2 * Cp + 255) / 256)), dim3(256), 0, s, reinterpret_cast<bf16x8*>(tail), gamma, beta, b1, Cp, hiddenP);
    return 0;
}

template <int CP, int NW, int NT = 3>
static void launch_mlp_x3(const MlpArgs& a, hipStream_t s) {
    auto kern = mlp_x3_kernel<CP, NW, false, NT>;
    constexpr int lds = 2 * mlp_x3_stage_frags(CP, NT) * 1024;
    if constexpr (lds > 48 * 1024) {            // function attributes are per device: one flag per device
        static std::atomic<unsigned> done{0};
        int dev = 0; (void)hipGetDevice(&dev);
        const unsigned bit = 1u << (dev & 31);
        if (!(done.load(std::memory_order_relaxed) & bit)) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); done.fetch_or(bit, std::memory_order_relaxed); }
    }
    const int hs = a.HS > 1 ? a.HS : 1;
    ESCX_LAUNCH(kern, dim3(((a.M + 16 * NW - 1) / (16 * NW)) * hs), dim3(64 * NW), lds, s, a);
}


// 32-byte trailer as rowgemm_x3_bytes: the allocation has the three-term size for both forms (set_precision re-packs in place); the two-term image (mlp_x3_split_tfy fragments
// per output tile) fills its head and the trailer {bits of max |w|}, {2^-k / sy, 2^k sy, sy, 0} stays at the allocation's end.  mlp_x3_split_trailer is the one definition.
size_t mlp_x3_split_bytes(int Cp, int Np) { return (size_t)(Np / 16) * mlp_x3_split_tfy(Cp, 3) * 1024 + 32; }
static char* mlp_x3_split_trailer(const void* image, int Cp, int Np) { return reinterpret_cast<char*>(const_cast<void*>(image)) + mlp_x3_split_bytes(Cp, Np) - 32; }
int mlp_x3_split_pack(const float* wf, void* image, int Cp, int Np, hipStream_t s, int nt, const float* gamma, const float* beta, int C) {
    if (nt != 2 && nt != 3) return -1;
    if (nt == 2 && (!gamma || !beta)) return -1;                    // the range rule needs the PatchSplit norm
    const int KK = Cp / 16, NT = Np / 16;
    const long long total = (long long)NT * ((KK + 1) / 2) * 64;
    char* tail = mlp_x3_split_trailer(image, Cp, Np);
    if (nt == 2) {
        if (hipMemsetAsync(tail, 0, 16, s) != hipSuccess) return -1;
        const long long n = (long long)NT * KK * 64 * 4;
        ESCX_LAUNCH(absmax_bits_kernel, dim3((unsigned)std::min<long long>(256, (n + 255) / 256)), dim3(256), 0, s, wf, n, reinterpret_cast<unsigned*>(tail));
    }
    ESCX_LAUNCH(mlp_x3_split_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(wf), reinterpret_cast<bf16x8*>(image), NT, KK,
                nt, mlp_x3_split_tfy(Cp, nt), reinterpret_cast<bf16x8*>(tail), gamma, beta, Cp, C);
    return 0;
}

template <int CP, int NW, int NT = 3>
static void launch_mlp_x3_split(const MlpArgs& a, hipStream_t s) {
    auto kern = mlp_x3_kernel<CP, NW, true, NT>;
    constexpr int lds = 2 * mlp_x3_stage_frags(CP, NT) * 1024;
    if constexpr (lds > 48 * 1024) {
        static std::atomic<unsigned> done{0};
        int dev = 0; (void)hipGetDevice(&dev);
        const unsigned bit = 1u << (dev & 31);
        if (!(done.load(std::memory_order_relaxed) & bit)) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); done.fetch_or(bit, std::memory_order_relaxed); }
    }
    ESCX_LAUNCH(kern, dim3((a.M + 16 * NW - 1) / (16 * NW)), dim3(64 * NW), lds, s, a);
}

// *hs_io: requested hidden split in, split used out (> 1: x untouched, partial[hs][M][Cp] filled, the caller runs rows_combine) - as mlp_fused
// split: PatchSplit in the epilogue (split->wf = the image of mlp_x3_split_pack); ESCX_COMB_UNSUPPORTED when the width has no such instantiation
int mlp_x3(float* x, int M, int C, int Cp, const float* gamma, const float* beta, const float* b1, const float* b2, const void* image, int hiddenP, int nw, int* hs_io, float* partial,
           hipStream_t s, const MlpSplit* split, int nt, float* out) {
    if (!image || hiddenP % 32 || (nt != 2 && nt != 3)) return -1;
    if (out && (split || (hs_io && *hs_io > 1))) return -1;             // out-of-place: the plain form only (training forward: x1 -> x2)
    if (split) {
        if ((hs_io && *hs_io > 1) || !split->wf || !(Cp == 80 || Cp == 96 || Cp == 144)) return ESCX_COMB_UNSUPPORTED;
        MlpArgs a{};
        a.x = x; a.gamma = gamma; a.beta = beta; a.b1 = b1; a.b2 = b2; a.M = M; a.C = C; a.HT = hiddenP / 16; a.eps = 1e-5f; a.HS = 1; a.x3_w = image;
        a.sp_wf = reinterpret_cast<const f32x4*>(split->wf); a.sp_gamma = split->gamma; a.sp_beta = split->beta; a.sp_out = split->out;
        a.sp_NT = split->NT; a.sp_H = split->H; a.sp_W = split->W; a.sp_C2p = split->C2p;
        if (nt == 2) a.sp_scale = reinterpret_cast<const float*>(mlp_x3_split_trailer(split->wf, Cp, 16 * split->NT) + 16);
        switch (Cp) {
#define ESCX_X3S_CASE(CPV) case CPV: if (nt == 2) { if (nw == 8) launch_mlp_x3_split<CPV, 8, 2>(a, s); else launch_mlp_x3_split<CPV, 4, 2>(a, s); } \
                           else { if (nw == 8) launch_mlp_x3_split<CPV, 8>(a, s); else launch_mlp_x3_split<CPV, 4>(a, s); } return 0;
            ESCX_X3S_CASE(80) ESCX_X3S_CASE(96) ESCX_X3S_CASE(144)
#undef ESCX_X3S_CASE
        }
        return ESCX_COMB_UNSUPPORTED;
    }
    int hs = hs_io ? *hs_io : 1;
    if (hs > 1 && (!partial || (hiddenP / 32) % hs)) hs = 1;
    if (hs_io) *hs_io = hs;
    MlpArgs a{};
    a.x = x; a.gamma = gamma; a.beta = beta; a.b1 = b1; a.b2 = b2; a.M = M; a.C = C; a.HT = hiddenP / 16; a.eps = 1e-5f; a.HS = hs; a.partial = partial; a.x3_w = image; a.out = out;
#define ESCX_X3_CASE(CPV) case CPV: if (nt == 2) { if (nw == 8) launch_mlp_x3<CPV, 8, 2>(a, s); else launch_mlp_x3<CPV, 4, 2>(a, s); } \
                          else { if (nw == 8) launch_mlp_x3<CPV, 8>(a, s); else launch_mlp_x3<CPV, 4>(a, s); } return 0;
    switch (Cp) {
        ESCX_X3_CASE(48) ESCX_X3_CASE(80) ESCX_X3_CASE(96) ESCX_X3_CASE(144) ESCX_X3_CASE(192) ESCX_X3_CASE(384)
        default: return -1;
    }
#undef ESCX_X3_CASE
}

// ---- fused LN + linear for PatchMerge / PatchSplit ----

template <int KP, int SEGS>
static int launch_rowgemm(const RowGemmArgs& a, hipStream_t s) {
    if (a.x3_wf) {           // split-operand form (fused_rowgemm.h rowgemm_x3_kernel): the widths of the ESC scale changes
        if constexpr (KP == 96 || KP == 160 || KP == 192 || KP == 288 || KP == 384 || KP == 144 || KP == 80) {
            constexpr int KSx = (KP + 31) / 32, TFx = 3 * KSx, UTx = 36 / TFx >= 4 ? 4 : (36 / TFx >= 2 ? 2 : 1);          // UT from the three-term tile, for both forms
            constexpr int TMx = KP <= 96 ? 2 : 1, NWx = 4;           // one row tile per wave above K = 96: the three-term operand costs 1.5x the registers of the fp32 one
            auto kern = rowgemm_x3_kernel<KP, SEGS, TMx, NWx, UTx>;
            auto kern2 = rowgemm_x3_kernel<KP, SEGS, TMx, NWx, UTx, 2>;
            constexpr int lds = 2 * UTx * TFx * 1024, lds2 = 2 * UTx * 2 * KSx * 1024;        // the two-term stream is dense: 2 KS fragments per output tile
            if constexpr (lds > 48 * 1024) {
                static std::atomic<unsigned> done{0};
                int dev = 0; (void)hipGetDevice(&dev);
                const unsigned bit = 1u << (dev & 31);
                if (!(done.load(std::memory_order_relaxed) & bit)) {
                    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
                    (void)hipFuncSetAttribute((const void*)kern2, hipFuncAttributeMaxDynamicSharedMemorySize, lds2);
                    done.fetch_or(bit, std::memory_order_relaxed);
                }
            }
            if (a.x3_scale) ESCX_LAUNCH(kern2, dim3((a.M + 16 * TMx * NWx - 1) / (16 * TMx * NWx), 1), dim3(64 * NWx), lds2, s, a);
            else ESCX_LAUNCH(kern, dim3((a.M + 16 * TMx * NWx - 1) / (16 * TMx * NWx), 1), dim3(64 * NWx), lds, s, a);
            return 0;
        }
    }
    constexpr int KK = KP / 16;
    constexpr int UT = KK <= 6 ? 4 : (KK <= 12 ? 2 : 1);
    constexpr int TM = KP <= 192 ? 2 : 1;
    constexpr int NW = 4;
    const int rows = 16 * TM * NW;
    // ONE output-column chunk (fused_rowgemm.h; bit-identical for every chunking).  MEASURED (round 3, B = 36): targets of 3072 / 6144 waves make the
    // merge + split kernels 3 % / 8 % SLOWER alone (1.333 -> 1.379 / 1.452 ms per step) and the step 2 - 2.6 % slower: these kernels are not short of
    // waves, the re-done gather + LayerNorm costs more than the extra occupancy returns.
    RowGemmArgs b = a;
    b.nt_chunk = (a.NT + UT - 1) / UT * UT;                       // whole stages
    const int chunks = (a.NT + b.nt_chunk - 1) / b.nt_chunk;
    ESCX_LAUNCH((rowgemm_fused_kernel<KP, SEGS, TM, NW, UT>), dim3((a.M + rows - 1) / rows, chunks), dim3(64 * NW), 0, s, b);
    return 0;
}

// 32-byte trailer: the two-term (nt = 2) form keeps max |w| and its power-of-two scales there (fused_attn.h attn_x3_pack_kernel).  The allocation has the
// three-term size; the two-term image (2 KS fragments per output tile) fills its first two thirds and the trailer stays at the allocation's end.
size_t rowgemm_x3_bytes(int KP, int Np) { return (size_t)(Np / 16) * 3 * ((KP + 31) / 32) * 1024 + 32; }
static char* rowgemm_x3_trailer(const void* image, int KP, int Np) { return reinterpret_cast<char*>(const_cast<void*>(image)) + rowgemm_x3_bytes(KP, Np) - 32; }
int rowgemm_x3_pack(const float* wf, void* image, int KP, int Np, hipStream_t s, int nt, const float* gamma, const float* beta, int C) {
    const int KK = KP / 16, KS = (KP + 31) / 32, NT = Np / 16;
    const long long total = (long long)NT * (KS > KK ? KS : KK) * 64;
    if (nt == 2) {
        unsigned* mx = reinterpret_cast<unsigned*>(rowgemm_x3_trailer(image, KP, Np));
        (void)hipMemsetAsync(mx, 0, 16, s);
        const long long n = (long long)NT * KK * 64 * 4;
        ESCX_LAUNCH(absmax_bits_kernel, dim3((unsigned)std::min<long long>(256, (n + 255) / 256)), dim3(256), 0, s, wf, n, mx);
    }
    ESCX_LAUNCH(attn_x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(wf), reinterpret_cast<bf16x8*>(image),
                       reinterpret_cast<bf16x8*>(rowgemm_x3_trailer(image, KP, Np)), NT, 1, KK, KS, (nt == 2 ? 2 : 3) * KS, 0u, nt == 2 ? 2 : 3, gamma, beta, KP, C, (const float*)nullptr, 0, 0, 0);         // no paired tail: rowgemm_x3_kernel keeps the zero-padded last step
    return 0;
}

int rowgemm_fused(int segs, const float* x, float* out, const float* gamma, const float* beta, const float* wf, const int* map, int M,
                  int rows_per_clip, int src_rows_per_clip, int C, int Cp, int Np, int split, int H, int W, int C2p, hipStream_t s,
                  const void* x3_wf, int x3_nt) {
    const int KP = segs * Cp;
    RowGemmArgs a{x, out, gamma, beta, reinterpret_cast<const f32x4*>(wf), map, M, rows_per_clip, src_rows_per_clip, C, Cp, Np / 16,
                  split, H, W, C2p, 1e-5f, Np / 16, x3_wf,
                  (x3_wf && x3_nt == 2) ? reinterpret_cast<const float*>(rowgemm_x3_trailer(x3_wf, KP, Np) + 16) : nullptr};
    if (segs == 1) {
        switch (KP) {
            case 16: return launch_rowgemm<16, 1>(a, s);
            case 48: return launch_rowgemm<48, 1>(a, s);
            case 80: return launch_rowgemm<80, 1>(a, s);
            case 96: return launch_rowgemm<96, 1>(a, s);
            case 144: return launch_rowgemm<144, 1>(a, s);
            case 192: return launch_rowgemm<192, 1>(a, s);
            case 384: return launch_rowgemm<384, 1>(a, s);
            default: return -1;
        }
    }
    switch (KP) {
        case 32: return launch_rowgemm<32, 2>(a, s);
        case 96: return launch_rowgemm<96, 2>(a, s);
        case 160: return launch_rowgemm<160, 2>(a, s);
        case 192: return launch_rowgemm<192, 2>(a, s);
        case 288: return launch_rowgemm<288, 2>(a, s);
        case 384: return launch_rowgemm<384, 2>(a, s);
        default: return -1;
    }
}

// ---- halo-tiled composed de-embedding -----------------------------------------------------------
// the two-term fp16 weight stream of deembed7_x2_kernel (fused_deembed.h), from the fp32 fragment stream; 0 bytes: no such instantiation for this width
size_t deembed7_x2_image_bytes(int Cp) { return Cp == 48 ? deembed7_x2_bytes(Cp) : 0; }
int deembed7_x2_pack(const float* wfrag, void* image, int Cp, hipStream_t s) {
    if (Cp != 48) return -1;
    const int nsteps = de2_steps(Cp);
    unsigned* mx = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(image) + deembed7_x2_bytes(Cp) - 32);
    if (hipMemsetAsync(mx, 0, 32, s) != hipSuccess) return -1;
    const long long n = (long long)49 * (Cp / 16) * 64 * 4;
    ESCX_LAUNCH(absmax_bits_kernel, dim3((unsigned)std::min<long long>(256, (n + 255) / 256)), dim3(256), 0, s, wfrag, n, mx);
    ESCX_LAUNCH(deembed7_x2_pack_kernel, dim3((nsteps * 64 + 255) / 256), dim3(256), 0, s, reinterpret_cast<const f32x4*>(wfrag), reinterpret_cast<bf16x8*>(image), Cp, nsteps);
    return 0;
}

int deembed7_fused(const float* tok, int B, int H, int W, int Cp, const float* wfrag, const float* bias, float* out, int pf, int pt,
                   int in_dim, int Fp, hipStream_t s, const void* x2_image) {
    DeembedArgs a{tok, reinterpret_cast<const f32x4*>(wfrag), bias, out, B, H, W, pf, pt, in_dim, Fp, in_dim * pf * pt};
    if (a.n_out > 16) return -1;
    const int grid = B * ((H + 7) / 8) * ((W + 31) / 32);
    if (x2_image && Cp == 48) {                 // two fp16 terms, contraction flattened over the 49 taps (the spectrum feeds the ISTFT only)
        auto kern = deembed7_x2_kernel<48>;
        constexpr int lds = 2 * 14 * 38 * (48 + 8) * 2 + 2 * 8 * 2 * 1024;
        static std::atomic<unsigned> done{0};
        int dev = 0; (void)hipGetDevice(&dev);
        const unsigned bit = 1u << (dev & 31);
        if (!(done.load(std::memory_order_relaxed) & bit)) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds); done.fetch_or(bit, std::memory_order_relaxed); }
        ESCX_LAUNCH(kern, dim3(grid), dim3(512), lds, s, a, reinterpret_cast<const bf16x8*>(x2_image));
        return 0;
    }
    switch (Cp) {               // LDS: (8+6) x (32+6) pixels x (Cp+4) dwords + two 7-tap weight stages <= 160 KiB
        case 16: ESCX_LAUNCH(deembed7_kernel<16>, dim3(grid), dim3(512), 0, s, a); return 0;
        case 32: ESCX_LAUNCH(deembed7_kernel<32>, dim3(grid), dim3(512), 0, s, a); return 0;
        case 48: ESCX_LAUNCH(deembed7_kernel<48>, dim3(grid), dim3(512), 0, s, a); return 0;
        default: return -1;
    }
}

// ---- fused window attention --------------------------------------------------------------------
// Paired head groups of the two-term stream (fused_attn.h attn_x3_pack_kernel): 0 = single groups, 1 = groups (2 i, 2 i + 1) share a stream unit and their projection MFMAs,
// 2 = the two halves of every MODE 2 group do.  Geometry only - one rule for the packer, the launcher and every batch.  An even group count leaves every workgroup of the
// head-group split (thirds) whole pairs.  Odd counts (C = 45: 3 groups) stay single; so does C = 384 (packed kernel: at the register limit, not built).
// attn_x3_fused: the (width, head mapping) pairs that have split-operand instantiations of attn_fused_kernel (the ESC configurations); only those ever read a paired image,
// so the pairing rule is tied to the same list (everything else runs the float32 kernel on the float32 stream).
static constexpr bool attn_x3_fused(int Cp, int mode) {
    return (Cp == 48 && mode == 0) || (Cp == 80 && (mode == 0 || mode == 2)) || (Cp == 96 && mode != 2) || (Cp == 144 && mode != 2) || (Cp == 192 && mode == 1);
}
static int attn_x3_pairing(int Cp, int mode, int n_groups) { return (!attn_x3_fused(Cp, mode) || Cp < 80) ? 0 : (mode == 2 ? 2 : (n_groups % 2 == 0 ? 1 : 0)); }

// LEN: the length-table instantiations (fused_attn.h; mixed-length batches).  Same rules, same register budgets, same streams as the plain ones.
template <int CP, int MODE, int NW, bool LEN = false>
static int launch_attn(const AttnArgs& a, hipStream_t s, bool pair) {
    constexpr int UT = CP <= 96 ? 4 : (CP <= 192 ? 2 : 1);
    constexpr int TMW = attn_windows_per_wave(CP);
    const int per_block = TMW * NW;
    const int gs = a.GS > 1 ? a.GS : 1;
    if (a.tape_qkv) {
        if constexpr (LEN) return ESCX_COMB_UNSUPPORTED;               // training forward (TAPE instantiations for the memory-bound widths; the deep scales keep their GEMMs)
        if constexpr (CP == 16 || CP == 48 || CP == 80 || CP == 96) {      // C = 144 / 192 measured: no gain over their GEMM sequence (62.5 vs 62.3-62.6 ms per step)
            if (gs == 1) {
                ESCX_LAUNCH((attn_fused_kernel<CP, MODE, UT, TMW, NW, true>), dim3((a.n_windows + per_block - 1) / per_block), dim3(64 * NW), 0, s, a);
                return 0;
            }
        }
        return ESCX_COMB_UNSUPPORTED;
    }
    // split-operand (3 x bf16) Q / K / V projections: the (width, head mapping) pairs of the ESC configurations
    if constexpr (attn_x3_fused(CP, MODE)) {
        if (a.x3_wf) {
            auto kern = attn_fused_kernel<CP, MODE, UT, TMW, NW, false, true, 3, false, LEN>;
            auto kern2 = attn_fused_kernel<CP, MODE, UT, TMW, NW, false, true, 2, false, LEN>;        // two fp16 terms (split_terms.h)
            constexpr int lds = 2 * UT * attn_x3_tf(CP) * 1024, lds2 = 2 * UT * attn_x3_tf(CP, 2) * 1024;      // the two-term stream is dense
            if constexpr (lds > 48 * 1024) {
                static std::atomic<unsigned> done{0};
                int dev = 0; (void)hipGetDevice(&dev);
                const unsigned bit = 1u << (dev & 31);
                if (!(done.load(std::memory_order_relaxed) & bit)) {
                    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
                    (void)hipFuncSetAttribute((const void*)kern2, hipFuncAttributeMaxDynamicSharedMemorySize, lds2);
                    done.fetch_or(bit, std::memory_order_relaxed);
                }
            }
            if constexpr (CP >= 80) {
                if (a.x3_scale && pair) {
                    auto kern2p = attn_fused_kernel<CP, MODE, UT, TMW, NW, false, true, 2, true, LEN>;
                    if constexpr (lds2 > 48 * 1024) {
                        static std::atomic<unsigned> donep{0};
                        int dev = 0; (void)hipGetDevice(&dev);
                        const unsigned bit = 1u << (dev & 31);
                        if (!(donep.load(std::memory_order_relaxed) & bit)) { (void)hipFuncSetAttribute((const void*)kern2p, hipFuncAttributeMaxDynamicSharedMemorySize, lds2); donep.fetch_or(bit, std::memory_order_relaxed); }
                    }
                    ESCX_LAUNCH(kern2p, dim3(((a.n_windows + per_block - 1) / per_block) * gs), dim3(64 * NW), lds2, s, a);
                    return 0;
                }
            }
            if (pair) return -1;            // a paired image has no single walk
            if (a.x3_scale) ESCX_LAUNCH(kern2, dim3(((a.n_windows + per_block - 1) / per_block) * gs), dim3(64 * NW), lds2, s, a);
            else ESCX_LAUNCH(kern, dim3(((a.n_windows + per_block - 1) / per_block) * gs), dim3(64 * NW), lds, s, a);
            return 0;
        }
    }
    ESCX_LAUNCH((attn_fused_kernel<CP, MODE, UT, TMW, NW, false, false, 3, false, LEN>), dim3(((a.n_windows + per_block - 1) / per_block) * gs), dim3(64 * NW), 0, s, a);
    return 0;
}

template <int CP, bool LEN = false>
static int launch_attn_cp(int mode, int nw, const AttnArgs& a, hipStream_t s, bool pair) {
    if (nw == 8) {
        switch (mode) {
            case 0: return launch_attn<CP, 0, 8, LEN>(a, s, pair);
            case 1: return launch_attn<CP, 1, 8, LEN>(a, s, pair);
            case 2: return launch_attn<CP, 2, 8, LEN>(a, s, pair);
        }
    } else {
        switch (mode) {
            case 0: return launch_attn<CP, 0, 4, LEN>(a, s, pair);
            case 1: return launch_attn<CP, 1, 4, LEN>(a, s, pair);
            case 2: return launch_attn<CP, 2, 4, LEN>(a, s, pair);
        }
    }
    return -1;
}

template <int CP, int NW>
static int launch_attn_packed(const AttnArgs& a, hipStream_t s) {
    constexpr int UT = CP <= 96 ? 4 : (CP <= 192 ? 2 : 1);
    const int pairs = (a.n_windows + 1) / 2;
    const int gs = a.GS > 1 ? a.GS : 1;
    if constexpr (CP == 384 && NW == 4) {        // split-operand Q / K / V projections (ESC's bottom scale)
        if (a.x3_wf) {
            auto kern = attn_packed_kernel<CP, UT, NW, true>;
            auto kern2 = attn_packed_kernel<CP, UT, NW, true, 2>;
            constexpr int lds = 2 * UT * attn_x3_tf(CP) * 1024, lds2 = 2 * UT * attn_x3_tf(CP, 2) * 1024;
            static std::atomic<unsigned> done{0};
            int dev = 0; (void)hipGetDevice(&dev);
            const unsigned bit = 1u << (dev & 31);
            if (!(done.load(std::memory_order_relaxed) & bit)) {
                (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
                (void)hipFuncSetAttribute((const void*)kern2, hipFuncAttributeMaxDynamicSharedMemorySize, lds2);
                done.fetch_or(bit, std::memory_order_relaxed);
            }
            if (a.x3_scale) ESCX_LAUNCH(kern2, dim3(((pairs + NW - 1) / NW) * gs), dim3(64 * NW), lds2, s, a);
            else ESCX_LAUNCH(kern, dim3(((pairs + NW - 1) / NW) * gs), dim3(64 * NW), lds, s, a);
            return 0;
        }
    }
    ESCX_LAUNCH((attn_packed_kernel<CP, UT, NW>), dim3(((pairs + NW - 1) / NW) * gs), dim3(64 * NW), 0, s, a);
    return 0;
}

// The allocation has the three-term size for both forms (set_precision re-packs in place): the dense two-term image (attn_x3_tf(Cp, 2) fragments per tile)
// fills its front, and the two-term form's 48-byte trailer (three maxima, scales: fused_attn.h attn_x3_pack_kernel) closes the allocation either way.
size_t attn_x3_bytes(int Cp, int mode, int n_groups) { return (size_t)n_groups * (mode == 2 ? 8 : 4) * attn_x3_tf(Cp) * 1024 + 48; }
static char* attn_x3_trailer(const void* image, int Cp, int mode, int n_groups) { return reinterpret_cast<char*>(const_cast<void*>(image)) + attn_x3_bytes(Cp, mode, n_groups) - 48; }

// nt == 2: the two-term fp16 form of the stream (split_terms.h): weights scaled by the power of two of the block's max |w|, scales in the trailer
int attn_x3_pack(const float* waf, void* image, int Cp, int mode, int n_groups, hipStream_t s, int nt, const float* gamma, const float* beta, int C, const float* bqkv) {
    const int KK = Cp / 16, KS = attn_x3_ks(Cp), TF = attn_x3_tf(Cp, nt == 2 ? 2 : 3), TPG = mode == 2 ? 8 : 4;
    const unsigned proj_mask = mode == 2 ? ((1u << 5) | (1u << 7)) : (1u << 3);        // order of the fp32 stream: [Q, K, V, P] / [Q_lo, K_lo, Q_hi, K_hi, V_lo, P_lo, V_hi, P_hi]
    const int pair = nt == 2 ? attn_x3_pairing(Cp, mode, n_groups) : 0;
    const int n_tiles = n_groups * TPG;
    (void)hipMemsetAsync(image, 0, attn_x3_bytes(Cp, mode, n_groups), s);
    const long long total = (long long)n_tiles * (KS > KK ? KS : KK) * 64;
    if (nt == 2) {
        unsigned* mx = reinterpret_cast<unsigned*>(attn_x3_trailer(image, Cp, mode, n_groups));
        const long long n = (long long)n_tiles * KK * 64 * 4;
        const unsigned all = (1u << TPG) - 1, vmask = mode == 2 ? ((1u << 4) | (1u << 6)) : (1u << 2);
        const dim3 grid((unsigned)std::min<long long>(256, (n + 255) / 256));
        ESCX_LAUNCH(absmax_tiles_bits_kernel, grid, dim3(256), 0, s, waf, n, KK * 256, TPG, all & ~proj_mask, mx);
        ESCX_LAUNCH(absmax_tiles_bits_kernel, grid, dim3(256), 0, s, waf, n, KK * 256, TPG, vmask, mx + 1);
        ESCX_LAUNCH(absmax_tiles_bits_kernel, grid, dim3(256), 0, s, waf, n, KK * 256, TPG, proj_mask, mx + 2);
    }
    ESCX_LAUNCH(attn_x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const f32x4*>(waf), reinterpret_cast<bf16x8*>(image),
                       reinterpret_cast<bf16x8*>(attn_x3_trailer(image, Cp, mode, n_groups)), n_tiles, TPG, KK, KS, TF, proj_mask, nt == 2 ? 2 : 3, gamma, beta, Cp, C, bqkv, n_groups * (mode == 2 ? 6 : 3) * 16, pair,
                       x2_tail_paired(Cp, nt) ? 1 : 0);          // the paired tail step of the Q / K / V tiles (split_terms.h)
    return 0;
}

int attn_fused(const float* src, float* dst, int Cp, int C, int mode, int n_groups, const float* gamma, const float* beta,
               const float* wf, const float* bqkv, const float* bias_tab, const float* bproj, const int* map, int slots, int tokens,
               int n_windows, int nWh, int nWw, int shifted, float scale, int nw, int* gs_io, float* partial, int rows, hipStream_t s,
               const AttnTape* tape, const void* x3_wf, int x3_nt, bool len_tables) {
    int gs = gs_io ? *gs_io : 1;        // head-group split: same in/out convention as mlp_fused
    if (gs > 1 && (!partial || n_groups % gs)) gs = 1;
    const int pairing = (!tape && x3_wf && x3_nt == 2) ? attn_x3_pairing(Cp, mode, n_groups) : 0;
    if (pairing == 1 && (n_groups / gs) % 2) gs = 1;         // a workgroup's share is whole pairs
    if (gs_io) *gs_io = gs;
    AttnArgs a{src, dst, gamma, beta, reinterpret_cast<const f32x4*>(wf), bqkv, bias_tab, bproj, map, slots, tokens, n_windows,
               nWh, nWw, shifted, C, n_groups, scale, 1e-5f, gs, partial, rows, g_mlp_trace,
               tape ? tape->xn : nullptr, tape ? tape->qkv : nullptr, tape ? tape->o : nullptr, tape ? tape->ldq : 0, tape ? tape->ldo : 0,
               tape ? tape->hdp : 0, tape ? tape->nH : 0, tape ? nullptr : x3_wf,
               (!tape && x3_wf && x3_nt == 2) ? reinterpret_cast<const float*>(attn_x3_trailer(x3_wf, Cp, mode, n_groups) + 16) : nullptr};
    if (tape && nw < 0) return ESCX_COMB_UNSUPPORTED;      // the packed H = 2 form has no tape stores
    if (len_tables) {       // mixed-length batches: `map` = batch-wide slot table + per-window flags (fused_attn.h LEN); the widths of the ESC configurations; general kernel only
        if (tape || nw < 0) return ESCX_COMB_UNSUPPORTED;
        switch (Cp) {
            case 16: return launch_attn_cp<16, true>(mode, nw, a, s, pairing != 0);
            case 32: return launch_attn_cp<32, true>(mode, nw, a, s, pairing != 0);
            case 48: return launch_attn_cp<48, true>(mode, nw, a, s, pairing != 0);
            case 64: return launch_attn_cp<64, true>(mode, nw, a, s, pairing != 0);
            case 80: return launch_attn_cp<80, true>(mode, nw, a, s, pairing != 0);
            case 96: return launch_attn_cp<96, true>(mode, nw, a, s, pairing != 0);
            case 128: return launch_attn_cp<128, true>(mode, nw, a, s, pairing != 0);
            case 144: return launch_attn_cp<144, true>(mode, nw, a, s, pairing != 0);
            case 192: return launch_attn_cp<192, true>(mode, nw, a, s, pairing != 0);
            case 256: return launch_attn_cp<256, true>(mode, nw, a, s, pairing != 0);
            case 384: return launch_attn_cp<384, true>(mode, nw, a, s, pairing != 0);
            default: return -1;
        }
    }
    // H == 2 scale with no padding along W: two half-real windows share one tile (nw < 0 encodes "packing allowed", |nw| waves)
    if (nw < 0) {
        nw = -nw;
        if (mode == 0) {
#define ESCX_PACK(CPV) case CPV: return nw == 8 ? launch_attn_packed<CPV, 8>(a, s) : launch_attn_packed<CPV, 4>(a, s);
            switch (Cp) { ESCX_PACK(64) ESCX_PACK(96) ESCX_PACK(128) ESCX_PACK(192) ESCX_PACK(256) ESCX_PACK(384) default: break; }
#undef ESCX_PACK
        }
    }
    switch (Cp) {
        case 16: return launch_attn_cp<16>(mode, nw, a, s, pairing != 0);
        case 32: return launch_attn_cp<32>(mode, nw, a, s, pairing != 0);
        case 48: return launch_attn_cp<48>(mode, nw, a, s, pairing != 0);
        case 64: return launch_attn_cp<64>(mode, nw, a, s, pairing != 0);
        case 80: return launch_attn_cp<80>(mode, nw, a, s, pairing != 0);
        case 96: return launch_attn_cp<96>(mode, nw, a, s, pairing != 0);
        case 128: return launch_attn_cp<128>(mode, nw, a, s, pairing != 0);
        case 144: return launch_attn_cp<144>(mode, nw, a, s, pairing != 0);
        case 192: return launch_attn_cp<192>(mode, nw, a, s, pairing != 0);
        case 256: return launch_attn_cp<256>(mode, nw, a, s, pairing != 0);
        case 384: return launch_attn_cp<384>(mode, nw, a, s, pairing != 0);
        default: return -1;
    }
}

}  // namespace escx
