// i8_layout.hpp — how the coarse copies of the matrix lie in memory: stated once, for their writer (rowcopy.hip) and their
// readers (coarse_scan.hpp, topk.hip).
#pragma once
#include "common.hpp"

namespace clipmi {
namespace {

// Layout of the copy (round 3): 32-row blocks, each [E / 32 k-steps][64 lanes][16 bytes] = the A operand of
// v_mfma_i32_32x32x32_i8 as it lies in registers - lane l of k-step s holds bytes 32 s + 16 (l >> 5) .. + 15 of row
// (l & 31) of the block - so a wave reads one k-step of a block as ONE contiguous KiB. The 32 rows of a block share
// their scale (s = the block's max |x| / 127): a wave's compare then has one scale per step and becomes an integer
// test (scan_coarse_wide_kernel). meta[r] = (s_block, a_r); bmeta[block] = (s_block, max a_r of the block), stored
// behind the row meta. Rows past N in the last block are zero.
// Round 4: the copy is a PERMUTATION of the rows. Slot t of the copy holds row perm[t] (perm = null: the identity); callers
// order the rows by their largest |component| (IndexFlatIP.matrix_i8), so that the 32 rows of a block have nearly the same
// maximum and the block's scale is (almost) each row's own: the error norms a_r - and with them the coarse bound's margin -
// drop back to the per-row-scale values of round 2 (x 1.265 -> x 1.000 on unit rows; re-scored rows per query 5.8 k -> 5.1 k
// at 10 M rows). The scans work on slots; slot_rows[t] = the row a slot holds (0xffffffff for the padding slots N .. N32 - 1),
// stored behind the block meta, is read only for survivors (rescore_pairs_kernel, rescore_pairs16_kernel), which leave the lists as row ids.

// meta of the int8 copy: row entries for N rounded up to 32 rows (+32), then one (scale, largest error norm) pair per block (+1)
inline size_t i8_row_meta_entries(int64_t N) { return (size_t)((N + 31) / 32 * 32 + 32); }
inline size_t i8_block_meta_entries(int64_t N) { return (size_t)((N + 31) / 32 + 1); }
// ... and behind the block meta one u32 per slot: the row it holds (quantize_rows_i8_kernel)
inline const unsigned* i8_slot_rows(const float2* rmeta, int64_t N) {
    return reinterpret_cast<const unsigned*>(rmeta + i8_row_meta_entries(N) + i8_block_meta_entries(N));
}

// The norms of the superset bounds (||y||, ||f_q||, a_r, R_max) are UPPER bounds: the squares are summed in f64 - the square of
// an f32 neither under- nor overflows there, and E <= 768 of them lose < 2^-43 relative - and the root is rounded UP to f32.
// (An f32 sum of squares drops every component below 2^-63 - a query scaled by 2^-70 had ||y|| = 0 and no margin at all.)
__device__ __forceinline__ float norm_up(double sumsq) {
    const double nd = sqrt(sumsq);
    float nf = (float)nd;
    if ((double)nf < nd) nf = nextafterf(nf, INFINITY);           // NaN stays NaN, +inf stays +inf
    return nf;
}

// Magnitudes the f32 arithmetic of a coarse bound is proved for. Below I8_TINY the scales, products and scores of the int8 test
// approach the subnormal grid, where a rounding is an ABSOLUTE 2^-150 that the relative slack c(E) R_max ||y|| does not cover;
// the bf16 test stops earlier, at BF16_TINY: a bf16 below 2^-126 keeps fewer than 8 bits (or is flushed by the matrix core).
// A block of rows below I8_TINY is stored as zero codes with scale 1 (a_r = its rows' norms: exact, no small product);
// a query or database outside [TINY, COARSE_HUGE] gets the margin +inf (coarse_prep_kernel) and the exact fallback answers.
constexpr float I8_TINY = 0x1p-110f, BF16_TINY = 0x1p-90f, COARSE_HUGE = 0x1p110f, COARSE_HUGE_RY = 0x1p120f;

// The bf16 copy is row-major [N][E]; its elements - and the bf16 query image - are rounded to nearest even, two at a time.
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack2_bf16(float a, float b) {
    f32x2v v = {a, b};
    bf16x2v r = __builtin_convertvector(v, bf16x2v);
    return __builtin_bit_cast(unsigned, r);
}

}  // namespace
}  // namespace clipmi
