// gemm256f8.hpp — the 256x256 pipelined NT GEMM of gemm256.hpp on OCP FP8 (e4m3) operands and the FP8 matrix
// cores (BASELINE.json configs[4]: "fp8 ViT-B/32 weights on CDNA4 fp8 MFMA"):
//     C[m][n] = a_scale[m] * w_scale[n] * sum_k A8[m][k] W8[n][k]  (+ bias, epilogues as gemm256)
// A8 = activations quantised per ROW (clipmi quantize_rows_fp8_kernel: scale = max|row| / 448, RNE), W8 = weights
// quantised per OUTPUT CHANNEL at pack time. Products of two e4m3 values are exact in f32 and the MFMA accumulates
// in f32, so the result equals an f32 matmul of the dequantised operands up to summation order.
//
// This file holds the FP8 operand policy only; schedule, LDS geometry and epilogue are g256_tile's (gemm256.hpp): a
// K-tile is 128 fp8 values instead of 64 bf16. Each 16-byte fragment a lane reads
// holds 16 consecutive k; v_mfma_f32_16x16x32_fp8_fp8 takes 8 per lane, so every fragment pair feeds TWO MFMAs (low
// halves, high halves): the k subsets of the two differ but agree between A and W, which is all a dot product
// needs. The non-scaled FP8 MFMA runs at the bf16 rate (MI355X_MICROARCH.md, matrix-core table): this path halves
// operand bytes, not MFMA cycles; the 2x rate needs the block-scaled (MX) forms.
// Requires N % 256 == 0, K % 128 == 0, K >= 256.
#pragma once
#include "gemm256.hpp"

namespace clipmi {

typedef long i64x2v __attribute__((ext_vector_type(2)));
typedef int i32x8v __attribute__((ext_vector_type(8)));

// BSA ("block-scaled A", round 3): the activations carry one e8m0 scale per 32 consecutive k (the MX format; written by
// the PRODUCING kernel's epilogue or by quantize_rows_fp8mx_kernel - a row scale would need the whole row before the first
// byte can be written, a 32-block is local to any column tile) in g.a_bscale [rows padded to 256][K / 32]. The scaled MFMA
// takes it as its per-lane scale operand, so the block scales cost no
// matrix cycles; the tile's 256 x K/32 scale bytes arrive once by LDS-DMA behind the K-tile buffers. a_scale is unused.
// Which k a lane's scale reaches was measured (tools/bsa_probe.py): the instruction orders its 128 k as [first 16 bytes of
// lane groups 0..3 | second 16 bytes of groups 0..3], cuts THAT into four blocks of 32 and takes block s's scale from lane
// group s - so with this kernel's fragment layout (a lane holds the 16-byte chunks fg and 4 + fg of the 128-byte row) the
// hardware's block s is k = 32 s .. 32 s + 31 of the K-tile, and lane (fr, fg) supplies the scale of (row fr, block fg).
template <bool MX, bool BSA_>
struct G256F8 {
    static_assert(!BSA_ || MX, "block scales need the scaled MFMA form");
    static constexpr bool F8 = true, BSA = BSA_;
    static constexpr int ES = 1;
    typedef i64x2v frag;
    static __device__ __forceinline__ size_t a_pitch(const GemmArgs& g) { return (size_t)g.K; }
    // the MFMA slot body (gemm256.hpp runs it per k-step, A row tile and W row tile of a quadrant):
    //   MX = false: 32 x v_mfma_f32_16x16x32_fp8_fp8 (low and high 8 bytes of each fragment pair; f32 accumulation of
    //               exact products; the bf16 MFMA rate)
    //   MX = true:  8 x v_mfma_scale_f32_16x16x128_f8f6f4 with UNIT block scales (e8m0 127 = 2^0) unless BSA: one instruction
    //               takes both 16-byte fragments of a lane (32 of the 128 k), twice the k per cycle. Probed on hardware
    //               (tools/probe/mfma_mx_probe.hip): the same products, summed with ~2^-15 relative error per
    //               instruction (a narrower adder than the f32 chain), far below e4m3's own 2^-4.
    static constexpr int KSTEPS = MX ? 1 : 2;
    static __device__ __forceinline__ f32x4 mma(int ks, frag b0, frag b1, frag a0, frag a1, f32x4 c, int sb) {
        if constexpr (MX) {
            typedef long i64x4v __attribute__((ext_vector_type(4)));
            const i64x4v bw = {b0.x, b0.y, b1.x, b1.y}, aw = {a0.x, a0.y, a1.x, a1.y};
            return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_bit_cast(i32x8v, bw), __builtin_bit_cast(i32x8v, aw), c, 0, 0, 0,
                                                                    0x7f7f7f7f, 0, BSA ? sb : 0x7f7f7f7f);
        } else {
            const frag bq = ks ? b1 : b0, aq = ks ? a1 : a0;
            c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(bq.x, aq.x, c, 0, 0, 0);
            return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(bq.y, aq.y, c, 0, 0, 0);
        }
    }
    // BSA: the tile's scale bytes [256][K / 32] to LDS behind the K-tile buffers, 1 KiB per wave and piece
    static __device__ __forceinline__ void scale_dma(const GemmArgs& g, char* smem, int m0, int wave, int lane) {
        const int KB32 = g.K >> 5;
        const unsigned char* sg = g.a_bscale + (size_t)m0 * KB32 + lane * 16;
        for (int pc = wave; pc < (KB32 >> 2); pc += 8)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sg + pc * 1024),
                                             (__attribute__((address_space(3))) void*)(smem + G256_LDS + pc * 1024), 16, 0, 0);
    }
    static __device__ __forceinline__ f32x4 w_scale(const GemmArgs& g, int n) { return *reinterpret_cast<const f32x4*>(g.w_scale + n); }
    static __device__ __forceinline__ float a_scale(const GemmArgs& g, int m) { return BSA ? 1.0f : g.a_scale[m]; }
    static __device__ __forceinline__ f32x4 scaled(f32x4 c, f32x4 w, float a) { return c * (w * a); }

    // QuickGELU forms with g.out_bscale: the rows leave as e4m3 + MX block scales (the next GEMM's A operand) instead of bf16:
    // gemm.hpp mx_pack_bf16x8, the bytes the persistent kernel's storers and quantize_rows_fp8mx_kernel write.
    // v = 8 bf16 of row m from column `col` on. False: g.out_bscale is not set, the row leaves as bf16.
    static __device__ __forceinline__ bool store_row_mx(const GemmArgs& g, const uint4& v, int m, int col, int lane) {
        if (!g.out_bscale) return false;
        unsigned sb_;
        const uint2 q8_ = mx_pack_bf16x8(v, sb_);
        if (m < g.M) {
            *reinterpret_cast<uint2*>(static_cast<unsigned char*>(g.out) + (size_t)m * g.N + col) = q8_;
            if ((lane & 3) == 0) g.out_bscale[(size_t)m * (g.N >> 5) + (col >> 5)] = (unsigned char)sb_;
        }
        return true;
    }
    // EPI_BIAS_RESID_LN8: the new residual row also leaves as e4m3 + MX block scales (A operand of the next LN-folded FP8
    // GEMM) with its 256-column statistics partial; a wave holds the whole segment (4 columns per lane): gemm.hpp
    // ln8_row_segment, shared with rows_mx_stats_kernel. Rows past M are computed (wave-wide shuffles) and dropped.
    static __device__ __forceinline__ void store_row_ln8(const GemmArgs& g, const f32x4& v, int m, int n0, int lane) {
        unsigned p4_, sb_;
        float sm_, sq_;
        ln8_row_segment(v, p4_, sb_, sm_, sq_);
        if (m < g.M) {
            *reinterpret_cast<unsigned*>(g.x8 + (size_t)m * g.N + n0 + lane * 4) = p4_;
            if ((lane & 7) == 0) g.x8_bs[(size_t)m * (g.N >> 5) + ((n0 + lane * 4) >> 5)] = (unsigned char)sb_;
            if (lane == 0) *reinterpret_cast<f32x2*>(g.ln_part + ((size_t)m * (g.N >> 8) + (n0 >> 8)) * 2) = f32x2{sm_, sq_};
        }
    }
};

template <int EPI, bool MX, bool BSA = false>
__global__ void __launch_bounds__(512, 2) gemm256f8_nt_kernel(GemmArgs g) {
    g256_tile<EPI, G256F8<MX, BSA>>(g);
}

}  // namespace clipmi
