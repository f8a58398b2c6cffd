// The DAC convolutions in the exact split-operand grade (escx_dac_set_precision(d, ESCX_PRECISION_BF16X3)): the implicit GEMMs of dac_kernels.h on
// v_mfma_f32_16x16x32_bf16 with every fp32 operand split exactly into three bf16 terms (gemm_bf16.h split3_bf16x4: v = t0 + t1 + t2) and the six leading
// cross products accumulated in fp32, smallest first.  Derived from gemm_bf16_kernel<.., WB16 = true, KS = 1, NTERM = 3>; what DAC needs beyond it:
//   * N tiles of 32, 64, 96 and 128 columns (Np = rup(Cout, 16) is 16 ... 1536; a tile's columns behind Np read zero weights and are not stored);
//   * any Kp that is a multiple of 16: the weight pieces (8 bf16) behind Kp are zero, and DacConvA returns zero for a tap behind the last one, so the
//     half-empty last 32-deep step adds exact zeros;
//   * any M: rows behind M are staged as zeros and not stored; DacConvA zeroes a tap outside its own clip.
// The weights come from a three-plane bf16 image of the packed, weight-normalised fp32 weights (dac.hip refresh_w16: split3_bf16_kernel over the whole
// packed-weight region, rebuilt whenever the fp32 image is).  The activation terms are formed while the operand is staged, from the fp32 value the loader
// returns - the Snake value when Snake is on this operand - so they do not depend on where Snake was evaluated.
// Every output element sees the same sequence of MFMAs whatever the tile shape: K in steps of 32 from 0, per step the cross terms (0,2) (2,0) (1,1) (0,1)
// (1,0) (0,0) (weight term, activation term).  A row's result therefore does not depend on the batch it is computed in.
// An epilogue with CHUNKED_K (gemm_engine.h; the backward's DacGradEpi, DacGradEpiV, DacGradPhaseEpi) gets two-level accumulation: the MFMA chain
// restarts every dac_x3_chunk(Kp) steps of 32 and the chunk's sum is added to a second accumulator, so one output's chain is 6 c MFMAs plus
// Kp / (32 c) adds instead of 6 Kp / 32 MFMAs (K runs to 12288 in the decoder's backward).  The chunk length comes from Kp alone, so the order of
// one output's sum is still fixed whatever the tile and the batch.  The chunks alternate in sign: an odd chunk stages the negated activation terms
// (the split of -v is the negated split of v, so every product is the exact negative) and its sum is subtracted.  On an exactly rounding adder this
// changes nothing; measured on the MI355X the bf16 MFMA's accumulation errs to one side (a dX element's error had a negative mean as large as its
// rms, which a column sum over rows - a bias gradient - amplified to 2.1 x the float32 reference's error on DAC-Base), and the alternation makes
// the one-sided part cancel between neighbouring chunks.  The forward epilogues compile to the kernels they had before the switch.
#pragma once
#include <hip/hip_runtime.h>
#include "gemm_bf16.h"

namespace escx {

// Steps of 32 per chunk of a CHUNKED_K contraction: the largest c in {1, 2, 4, 8} with 6 c^2 <= steps, which keeps the inner chain (6 c MFMAs) no
// longer than the outer one (steps / c adds).  Kp = 12288: 384 steps, c = 8, 48 + 48.
__host__ __device__ inline int dac_x3_chunk(int Kp) {
    const int steps = (Kp + 31) / 32;
    return steps >= 384 ? 8 : steps >= 96 ? 4 : steps >= 24 ? 2 : 1;
}

template <int BM, int BN, class Loader, class Epi>
__global__ __launch_bounds__(256) void dac_x3_kernel(Loader ld, const __bf16* __restrict__ W16, size_t plane, int M, int Np, int Kp, int nblk_n, Epi ep) {
    static_assert(BM % 64 == 0 && BN % 16 == 0, "tile shape");
    constexpr int BK = 32;
    constexpr int LD = BK + 8;                 // bf16 per LDS row: 80 B, the 16 rows of a fragment read start 20 banks apart
    constexpr int TM = BM / 64, TN = BN / 16;
    constexpr int KV = BK / 4;                 // float4 per activation-tile row and K step
    constexpr int AJ = BM * KV / 256;
    constexpr int WP = BN * (BK / 8);          // 16-byte pieces (8 bf16) per weight-tile plane
    constexpr int WJ = (WP + 255) / 256;       // ... per thread (the last round is partial for 96 and 32 columns)

    __shared__ __attribute__((aligned(16))) __bf16 As[3 * BM * LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[3 * BN * LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int bm = blockIdx.x / nblk_n, bn = blockIdx.x - bm * nblk_n;
    const int m0 = bm * BM, n0 = bn * BN;

    typename Loader::Ctx ctx[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) ctx[j] = ld.make_ctx(m0 + (tid + j * 256) / KV);
    if constexpr (loader_skips_dead<Loader>::value) {      // gemm_engine.h: a tile of rows past their clips' lengths has nothing to compute
        int live = 0;
#pragma unroll
        for (int j = 0; j < AJ; ++j) live |= ld.row_live(ctx[j]);
        if (!__syncthreads_or(live)) return;
    }

    f32x4 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) acc[a][b] = zero4();
    constexpr bool CHUNKED = epi_chunked_k<Epi>::value;
    [[maybe_unused]] f32x4 tot[CHUNKED ? TN : 1][CHUNKED ? TM : 1];
    [[maybe_unused]] int left = 0;             // steps until the chunk at hand is closed
    [[maybe_unused]] int chunk = 0;
    [[maybe_unused]] float sgn = 1.0f;         // sign of the chunk at hand: +, -, +, ... from k = 0
    if constexpr (CHUNKED) {
        chunk = left = dac_x3_chunk(Kp);
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int b = 0; b < TM; ++b) tot[a][b] = zero4();
    }

    f32x4 ra[AJ];
    uint4 rw[3 * WJ];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) ra[j] = ld.load4(ctx[j], k0, 4 * ((tid + j * 256) % KV));
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
            const int i = tid + j * 256, row = i >> 2, c8 = i & 3;
            const bool ok = (WP % 256 == 0 || i < WP) && n0 + row < Np && k0 + 8 * c8 < Kp;
#pragma unroll
            for (int p = 0; p < 3; ++p)
                rw[p * WJ + j] = ok ? *reinterpret_cast<const uint4*>(W16 + p * plane + (size_t)(n0 + row) * Kp + k0 + 8 * c8) : make_uint4(0, 0, 0, 0);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < Kp; k0 += BK) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int i = tid + j * 256;
            f32x4 v = ra[j];
            if constexpr (CHUNKED) v = v * sgn;
            bf16x4 t0, t1, t2; split3_bf16x4(v, t0, t1, t2);
            *reinterpret_cast<bf16x4*>(&As[(i / KV) * LD + 4 * (i % KV)]) = t0;
            *reinterpret_cast<bf16x4*>(&As[BM * LD + (i / KV) * LD + 4 * (i % KV)]) = t1;
            *reinterpret_cast<bf16x4*>(&As[2 * BM * LD + (i / KV) * LD + 4 * (i % KV)]) = t2;
        }
#pragma unroll
        for (int j = 0; j < WJ; ++j) {
            const int i = tid + j * 256;
            if (WP % 256 == 0 || i < WP) {
#pragma unroll
                for (int p = 0; p < 3; ++p) *reinterpret_cast<uint4*>(&Bs[p * BN * LD + (i >> 2) * LD + 8 * (i & 3)]) = rw[p * WJ + j];
            }
        }
        __syncthreads();
        if (k0 + BK < Kp) fetch(k0 + BK);
        bf16x8 af3[3][TM];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int b = 0; b < TM; ++b) af3[p][b] = *reinterpret_cast<const bf16x8*>(&As[p * BM * LD + (wave * (BM / 4) + b * 16 + l15) * LD + 8 * lg]);
#pragma unroll
        for (int a = 0; a < TN; ++a) {
            bf16x8 wf3[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) wf3[p] = *reinterpret_cast<const bf16x8*>(&Bs[p * BN * LD + (a * 16 + l15) * LD + 8 * lg]);
#define ESCX_DX3(I, J) _Pragma("unroll") for (int b = 0; b < TM; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf3[I], af3[J][b], acc[a][b], 0, 0, 0);
            ESCX_DX3(0, 2) ESCX_DX3(2, 0) ESCX_DX3(1, 1) ESCX_DX3(0, 1) ESCX_DX3(1, 0) ESCX_DX3(0, 0)
#undef ESCX_DX3
        }
        if constexpr (CHUNKED) {
            if (--left == 0 || k0 + BK >= Kp) {                 // the last chunk may be short
                left = chunk;
#pragma unroll
                for (int a = 0; a < TN; ++a)
#pragma unroll
                    for (int b = 0; b < TM; ++b) { tot[a][b] += acc[a][b] * sgn; acc[a][b] = zero4(); }
                sgn = -sgn;
            }
        }
        __syncthreads();
    }
    if constexpr (CHUNKED) {
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int b = 0; b < TM; ++b) acc[a][b] = tot[a][b];
    }
#pragma unroll
    for (int b = 0; b < TM; ++b) {
        const int m = m0 + wave * (BM / 4) + b * 16 + l15;
        if (m >= M) continue;
#pragma unroll
        for (int a = 0; a < TN; ++a) {
            const int n = n0 + a * 16 + 4 * lg;
            if (n < Np) ep.store(m, n, acc[a][b], 0);
        }
    }
}

// The dispatch rule, on the layer geometry alone (never on the batch):
//   columns per tile   Np <= 32: 32;  Np <= 64: 64;  else 96 or 128, whichever pads Np less (128 on a tie)
//   rows per tile      128 when that gives at least 512 tiles (two resident workgroups per CU, twice over), else 64.  The row tile does depend on M;
//                      it changes which workgroup computes an element, not the element's arithmetic (see the head of this file).
inline int dac_x3_bn(int Np) {
    if (Np <= 32) return 32;
    if (Np <= 64) return 64;
    return (Np + 127) / 128 * 128 <= (Np + 95) / 96 * 96 ? 128 : 96;
}

//   CHUNKED_K epilogues  the second accumulator doubles the tile's accumulator registers: 128 x 96 needs 276 VGPRs (one workgroup per CU instead of two)
//                      and 128 x 128 spills 272 bytes to scratch, so 96- and 128-column tiles always take 64 rows (180 and 204 VGPRs, no scratch) and
//                      those two instantiations do not exist.
template <class Loader, class Epi>
inline void launch_dac_x3(const Loader& ld, const __bf16* W16, size_t plane, int M, int Np, int Kp, const Epi& ep, hipStream_t s) {
    constexpr bool CHUNKED = epi_chunked_k<Epi>::value;
    const int bn = dac_x3_bn(Np), nbn = (Np + bn - 1) / bn;
    const bool big = (long long)((M + 127) / 128) * nbn >= 512 && !(CHUNKED && bn > 64);
    const dim3 grid(((M + (big ? 127 : 63)) / (big ? 128 : 64)) * nbn);
#define ESCX_DX3_LAUNCH(BM, BN) hipLaunchKernelGGL((dac_x3_kernel<BM, BN, Loader, Epi>), grid, dim3(256), 0, s, ld, W16, plane, M, Np, Kp, nbn, ep)
    if (big) {
        if constexpr (!CHUNKED) { if (bn == 128) { ESCX_DX3_LAUNCH(128, 128); return; } if (bn == 96) { ESCX_DX3_LAUNCH(128, 96); return; } }
        if (bn == 64) ESCX_DX3_LAUNCH(128, 64); else ESCX_DX3_LAUNCH(128, 32);
    } else {
        if (bn == 128) ESCX_DX3_LAUNCH(64, 128); else if (bn == 96) ESCX_DX3_LAUNCH(64, 96); else if (bn == 64) ESCX_DX3_LAUNCH(64, 64); else ESCX_DX3_LAUNCH(64, 32);
    }
#undef ESCX_DX3_LAUNCH
}

// ------------------------------------------------------------------------------------------------
// The split-operand weight gradient of the narrow layers (escx_dac_set_param_grad_precision; dac.hip param_layer): gemm_bf16.h's
// gemm_dw_bf16_kernel<LdA, LdB, 3> with TA = 32 or 64 rows of dW per workgroup instead of 128, for Np <= 64, where a 128-row tile is at most
// half full.  dW[n][k] = sum_m A[m][n] B[m][k] over one slice of the rows: one workgroup = a TA x 128 tile, wave w owns the k columns
// [32 w, 32 w + 32) x all TA n.  The staging is that kernel's - a thread loads rows (m, m + 1) of four columns, splits each value into three
// bf16 terms and writes [term][column][m] into LDS - with the A side staged by the threads whose four columns lie inside the tile.  Every output
// sees that kernel's sequence of MFMAs: the rows in steps of 32 from the slice's first, per step the cross terms (0,2) (2,0) (1,1) (0,1) (1,0)
// (0,0), so for the same slices the two kernels give the same bits.  Rows behind the slice and columns behind Np / Kp are staged as zeros
// (the loaders' contract, gemm_bf16.h) and not stored.
// ------------------------------------------------------------------------------------------------
template <int TA, class LdA, class LdB>
__global__ __launch_bounds__(256) void dac_dw_x3_kernel(LdA la, LdB lb, int M, int Np, int Kp, int nblk_k, int m_per_slice, float* __restrict__ part) {
    static_assert(TA == 32 || TA == 64, "rows of dW per workgroup");
    constexpr int TB = 128, MS = 32, LD = MS + 8, NB = TA / 16;
    __shared__ __attribute__((aligned(16))) __bf16 At[3 * TA * LD];
    __shared__ __attribute__((aligned(16))) __bf16 Bt[3 * TB * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
    const int mp = lane & 15, cq = 4 * (4 * wave + (lane >> 4));          // staging role: row pair mp of the step, columns cq .. cq + 3 (B: and + 64)
    const int bn = blockIdx.x / nblk_k, bk = blockIdx.x - bn * nblk_k;
    const int n0 = bn * TA, k0 = bk * TB;
    const int mbeg = blockIdx.y * m_per_slice, mend = min(M, mbeg + m_per_slice);
    const bool stage_a = cq < TA;               // TA = 64: everybody; TA = 32: waves 0 and 1

    f32x4 acc[2][NB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = zero4();
    f32x4 ra[2] = {zero4(), zero4()}, rb[2][2];                         // [row of the pair], [column group][row of the pair]
    auto fetch = [&](int m0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int m = m0 + 2 * mp + r;
            const typename LdB::Ctx cb = lb.make_ctx(m < mend ? m : M);         // rows behind the slice (or the matrix) read as zero
#pragma unroll
            for (int j = 0; j < 2; ++j) rb[j][r] = lb.load4(cb, k0 + 64 * j + cq, 0);
            if (stage_a) { const typename LdA::Ctx ca = la.make_ctx(m < mend ? m : M); ra[r] = la.load4(ca, n0 + cq, 0); }
        }
    };
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    auto stage = [](__bf16* img, int rows, int col, int mp2, f32x4 v0, f32x4 v1) {      // rows m, m + 1 of four columns -> three planes of [column][m]
        bf16x4 t0[3], t1[3];
        split3_bf16x4(v0, t0[0], t0[1], t0[2]); split3_bf16x4(v1, t1[0], t1[1], t1[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bf16x2 pr; pr[0] = t0[p][e]; pr[1] = t1[p][e];
                *reinterpret_cast<unsigned*>(&img[p * rows * LD + (col + e) * LD + mp2]) = __builtin_bit_cast(unsigned, pr);
            }
    };
    if (mbeg < mend) fetch(mbeg);
    for (int m0 = mbeg; m0 < mend; m0 += MS) {
        if (stage_a) stage(At, TA, cq, 2 * mp, ra[0], ra[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) stage(Bt, TB, 64 * j + cq, 2 * mp, rb[j][0], rb[j][1]);
        __syncthreads();
        if (m0 + MS < mend) fetch(m0 + MS);
        bf16x8 af3[3][NB];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int b = 0; b < NB; ++b) af3[p][b] = *reinterpret_cast<const bf16x8*>(&At[p * TA * LD + (16 * b + l15) * LD + 8 * lg]);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            bf16x8 wf3[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) wf3[p] = *reinterpret_cast<const bf16x8*>(&Bt[p * TB * LD + (32 * wave + 16 * a + l15) * LD + 8 * lg]);
#define ESCX_DD3(I, J) _Pragma("unroll") for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf3[I], af3[J][b], acc[a][b], 0, 0, 0);
            ESCX_DD3(0, 2) ESCX_DD3(2, 0) ESCX_DD3(1, 1) ESCX_DD3(0, 1) ESCX_DD3(1, 0) ESCX_DD3(0, 0)
#undef ESCX_DD3
        }
        __syncthreads();
    }
    float* pt = part + (size_t)blockIdx.y * Np * Kp;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int n = n0 + 16 * b + l15;
        if (n >= Np) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int k = k0 + 32 * wave + 16 * a + 4 * lg;
            if (k < Kp) st4(pt + (size_t)n * Kp + k, acc[a][b]);
        }
    }
}

// Rows of dW per workgroup of the split-operand weight gradient, from Np alone: 32 and 64 where one tile holds all of Np, else gemm_dw_bf16_kernel's 128
inline int dac_dw_x3_rows(int Np) { return Np <= 32 ? 32 : (Np <= 64 ? 64 : 128); }

template <class LdA, class LdB>
inline void launch_dac_dw_x3(const LdA& la, const LdB& lb, int M, int Np, int Kp, int slices, int m_per_slice, float* part, hipStream_t s) {
    const int ta = dac_dw_x3_rows(Np), nbk = (Kp + 127) / 128;
    const dim3 grid(((Np + ta - 1) / ta) * nbk, slices);
    if (ta == 32) hipLaunchKernelGGL((dac_dw_x3_kernel<32, LdA, LdB>), grid, dim3(256), 0, s, la, lb, M, Np, Kp, nbk, m_per_slice, part);
    else if (ta == 64) hipLaunchKernelGGL((dac_dw_x3_kernel<64, LdA, LdB>), grid, dim3(256), 0, s, la, lb, M, Np, Kp, nbk, m_per_slice, part);
    else hipLaunchKernelGGL((gemm_dw_bf16_kernel<LdA, LdB, 3>), grid, dim3(256), 0, s, la, lb, M, Np, Kp, nbk, m_per_slice, part, (float*)nullptr);
}

}  // namespace escx
