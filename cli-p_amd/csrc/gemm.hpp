// gemm.hpp — bf16 "NT" GEMM on v_mfma_f32_16x16x32_bf16 with fused epilogues (gfx950).
//
//   C[m][n] = sum_k A[m][k] * W[n][k]      A: activations bf16 [M][K], W: weights bf16 [N][K]
//
// Both operands are K-contiguous (PyTorch Linear layout), so both LDS tiles are [rows][64] bf16
// and every MFMA fragment is one 16-byte ds_read_b128. These are the GEMMs behind
// model.encode_image / encode_text (reference build-index.py:49, query-index.py:108): patch
// embedding, attention in/out projections, MLP c_fc / c_proj, final projection.
//
// Structure (v1): 128x128x64 block tile, 256 threads = 2x2 waves of 64x64, tiles staged by
// LDS-DMA (global_load_lds, 16 B/lane) into two buffers, ONE barrier per K-tile (prefetch of
// tile t+1 is in flight while tile t is multiplied). The 128-byte LDS rows are XOR-swizzled in
// 16-byte chunks (chunk ^= row & 7) — applied on the SOURCE address of the DMA and on the read
// address, never on the (lane-linear) DMA destination — which makes every ds_read_b128 lane
// group conflict-free.
//
// The MFMA is issued as D = Wfrag x Afrag, i.e. the accumulator tile is C^T: its column (lane&15)
// is the output ROW m and its 4 registers are 4 CONSECUTIVE output columns n, so the epilogue
// loads bias / residual and stores results as 8- or 16-byte vectors.
#pragma once
#include "common.hpp"
#include "gemm_plan.hpp"     // Epilogue, the epilogue predicates, SKINNY_MAX_M

namespace clipmi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
    f32x2 v = {a, b};
    bf16x2 r = __builtin_convertvector(v, bf16x2);     // v_cvt_pk_bf16_f32 (RNE, NaN-preserving)
    return __builtin_bit_cast(unsigned, r);
}

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

// x * sigmoid(1.702 x)   (OpenAI CLIP QuickGELU) = x / (1 + 2^(-1.702 log2(e) x)): one v_exp_f32
// and one v_rcp_f32 (1 ulp each; the result is rounded to bf16 right after). The transcendental pair is
// what the epilogue of the largest GEMM pays for (quarter-rate units): everything else is packed f32 math.
constexpr float QGELU_C = -2.4554669595930157f;        // -1.702 * log2(e)
__device__ __forceinline__ float quick_gelu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * QGELU_C));
}
__device__ __forceinline__ f32x4 quick_gelu4(f32x4 x) {
    const f32x4 t = x * QGELU_C;
    f32x4 e;
    e.x = __builtin_amdgcn_exp2f(t.x); e.y = __builtin_amdgcn_exp2f(t.y);
    e.z = __builtin_amdgcn_exp2f(t.z); e.w = __builtin_amdgcn_exp2f(t.w);
    const f32x4 d = e + 1.0f;
    f32x4 r;
    r.x = __builtin_amdgcn_rcpf(d.x); r.y = __builtin_amdgcn_rcpf(d.y);
    r.z = __builtin_amdgcn_rcpf(d.z); r.w = __builtin_amdgcn_rcpf(d.w);
    return x * r;
}

// ---- LN-folded linear layers ---------------------------------------------------------------------------------
// y = LayerNorm(x; gamma, beta) W^T + b, with mean / rstd the row statistics of x, equals
//     y[m][n] = rstd[m] * ( sum_k x[m][k] Wg[n][k]  -  mean[m] * colsum[n] ) + cb[n]
//     Wg = W * diag(gamma) (stored bf16),  colsum[n] = sum_k Wg[n][k],  cb[n] = sum_k beta[k] W[n][k] + b[n]
// (packed by weights.py). The residual stream is kept SPLIT: x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (two
// bf16 arrays, 4 bytes per element as f32 was, ~2^-17 relative error per update), so `hi` is at once half of the
// residual state and the A operand of the next LN-folded GEMM: the residual GEMM's store pass (EPI_BIAS_RESID_LN_F32)
// reads hi + lo, adds, writes hi + lo and the row-statistics partials of the new rows, and neither the stand-alone
// LayerNorm pass (read f32 x, write bf16 h: 200 MB per launch at B = 870, 8.5 % of the r01 encode step) nor a separate
// bf16 copy of x exists.
// Row statistics are CANONICAL so that every producer gives the same bits (batch-size invariance): per
// 256-column segment a wave holds 4 consecutive columns per lane, lane sums in a fixed order, then a butterfly
// over xor masks 32, 16, 8, 4, 2, 1; the per-segment (sum, sum of squares) pairs ARE the stored format
// (ln_part [M][K/256][2]) and consumers combine them left to right (ln_row_stats).
constexpr float LN_EPS = 1e-5f;

__device__ __forceinline__ float ln_lane_sum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ln_lane_sumsq(f32x4 v) {
    float q = v.x * v.x;
    q = __builtin_fmaf(v.y, v.y, q);
    q = __builtin_fmaf(v.z, v.z, q);
    return __builtin_fmaf(v.w, v.w, q);
}
// Lane exchanges of the statistics reductions WITHOUT the LDS crossbar (round 5; __shfl_xor is ds_bpermute_b32: an LDS round trip
// per step of a dependent chain - six of them per 32-row sub-pass of the residual producer's store pass): v_permlane32_swap /
// v_permlane16_swap exchange half-waves / 16-lane rows of two registers, DPP row_ror / row_shl / row_shr / quad_perm do the rest.
template <int CTRL>
__device__ __forceinline__ float lane_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_xor8(float v) { return lane_dpp<0x128>(v); }                 // row_ror:8
__device__ __forceinline__ float lane_xor4(float v, bool bit2) {                                    // bit2 = lane & 4
    const float up = lane_dpp<0x104>(v), dn = lane_dpp<0x114>(v);     // row_shl:4 (from lane + 4), row_shr:4 (from lane - 4)
    return bit2 ? dn : up;
}
__device__ __forceinline__ float lane_xor2(float v) { return lane_dpp<0x4E>(v); }                  // quad_perm [2,3,0,1]
__device__ __forceinline__ float lane_xor1(float v) { return lane_dpp<0xB1>(v); }                  // quad_perm [1,0,3,2]
// lanes 0-31: a + a of lane + 32; lanes 32-63: b + b of lane - 32 (the xor-32 step of two butterflies at once, each lane keeping
// the half it is responsible for); with a == b: every lane's v + v of lane ^ 32
__device__ __forceinline__ float lane_fold32(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// rows of 16 lanes: even rows a + a of lane + 16, odd rows b + b of lane - 16
__device__ __forceinline__ float lane_fold16(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// all 64 lanes end with the wave total; the xor order (32, 16, 8, 4, 2, 1) is part of the contract
__device__ __forceinline__ float ln_wave_sum(float v) {
    const bool bit2 = (__builtin_amdgcn_mbcnt_lo(~0u, 0u) & 4u) != 0;
    v = lane_fold32(v, v);
    v = lane_fold16(v, v);
    v += lane_xor8(v);
    v += lane_xor4(v, bit2);
    v += lane_xor2(v);
    v += lane_xor1(v);
    return v;
}
// (mean, rstd) from per-segment (sum, sum of squares) partials, combined left to right
__device__ __forceinline__ f32x2 ln_row_stats(const float* part, int nseg, int W) {
    // nseg <= 4 (W <= 1024); static indices only: a runtime-indexed register array would go to scratch
    float s = part[0], q = part[1];
    if (nseg > 1) { s += part[2]; q += part[3]; }
    if (nseg > 2) { s += part[4]; q += part[5]; }
    if (nseg > 3) { s += part[6]; q += part[7]; }
    const float inv = 1.0f / (float)W;
    const float mean = s * inv;
    float var = __builtin_fmaf(-mean, mean, q * inv);
    var = var > 0.f ? var : 0.f;
    return f32x2{mean, __builtin_amdgcn_rsqf(var + LN_EPS)};
}
// the LN-folded epilogue, identical in every GEMM kernel (explicit fmas: no contraction choices left to the compiler)
__device__ __forceinline__ f32x4 ln_apply(f32x4 acc, float mean, float rstd, f32x4 colsum, f32x4 cb) {
    f32x4 r;
    r.x = __builtin_fmaf(__builtin_fmaf(-mean, colsum.x, acc.x), rstd, cb.x);
    r.y = __builtin_fmaf(__builtin_fmaf(-mean, colsum.y, acc.y), rstd, cb.y);
    r.z = __builtin_fmaf(__builtin_fmaf(-mean, colsum.z, acc.z), rstd, cb.z);
    r.w = __builtin_fmaf(__builtin_fmaf(-mean, colsum.w, acc.w), rstd, cb.w);
    return r;
}
// Split residual (round 5: THREE bytes per element - VERDICT r04 item 1a): x is kept as hi = bf16(x) (round to nearest even; also
// the A operand of the LN-folded GEMMs) and an 8-bit remainder u with
//     bits(x') = (bits(hi) << 16) + (u << 8) - 0x8000,   u = clamp(round((bits(x) - (bits(hi) << 16)) / 256) + 128, 0, 255)
// - integer arithmetic on the f32 bit pattern (monotone in the magnitude for either sign, carries across binades): x' is x
// rounded to 15 mantissa bits, |x' - x| <= 2^-16 |x| (2^-15 where the remainder would need 256: 0.4 % of values), what the bf16
// pair of rounds 2-4 carried in 4 bytes. The remainder is stored BIASED (u = remainder + 128) so that joining is one byte
// permute + one subtract per value. A residual row is [W bf16 hi | W u8 remainders] = 3 W bytes: the store pass of the
// residual GEMMs moves 768 instead of 1024 bytes per row and 256-column tile each way. Four columns at a time.
__device__ __forceinline__ f32x4 split_join(uint2 hi, unsigned lo) {
    // v_perm_b32: bytes 4-7 = first operand, 0-3 = second, selector 0x0c = 0x00: [hi byte 1, hi byte 0, remainder, 0]
    return f32x4{__uint_as_float(__builtin_amdgcn_perm(hi.x, lo, 0x0504000cu) - 0x8000u),
                 __uint_as_float(__builtin_amdgcn_perm(hi.x, lo, 0x0706010cu) - 0x8000u),
                 __uint_as_float(__builtin_amdgcn_perm(hi.y, lo, 0x0504020cu) - 0x8000u),
                 __uint_as_float(__builtin_amdgcn_perm(hi.y, lo, 0x0706030cu) - 0x8000u)};
}
__device__ __forceinline__ void split_make(f32x4 o, uint2& hi, unsigned& lo) {
    hi = make_uint2(pack_bf16x2(o.x, o.y), pack_bf16x2(o.z, o.w));
    // t = remainder + 0x8080 in [0x80, 0x10080]: its byte 1 is u (round half up), 0x10000 and above clamp to 0xffff
    auto rem = [](float v, unsigned hb) -> unsigned {
        const unsigned t = (__float_as_uint(v) + 0x8080u) - hb;
        return t < 0xffffu ? t : 0xffffu;
    };
    const unsigned t0 = rem(o.x, hi.x << 16), t1 = rem(o.y, hi.x & 0xffff0000u), t2 = rem(o.z, hi.y << 16),
                   t3 = rem(o.w, hi.y & 0xffff0000u);
    lo = __builtin_amdgcn_perm(t1, t0, 0x0c0c0501u) | __builtin_amdgcn_perm(t3, t2, 0x05010c0cu);
}
// bytes of one residual row / where a row's remainders start, for row width W
__host__ __device__ constexpr size_t resid_row_bytes(int W) { return (size_t)W * 3; }
__device__ __forceinline__ const unsigned short* resid_hi(const void* x3, size_t row, int W) {
    return reinterpret_cast<const unsigned short*>(static_cast<const char*>(x3) + row * resid_row_bytes(W));
}
__device__ __forceinline__ unsigned short* resid_hi(void* x3, size_t row, int W) {
    return reinterpret_cast<unsigned short*>(static_cast<char*>(x3) + row * resid_row_bytes(W));
}
__device__ __forceinline__ const unsigned char* resid_lo(const void* x3, size_t row, int W) {
    return reinterpret_cast<const unsigned char*>(static_cast<const char*>(x3) + row * resid_row_bytes(W) + (size_t)W * 2);
}
__device__ __forceinline__ unsigned char* resid_lo(void* x3, size_t row, int W) {
    return reinterpret_cast<unsigned char*>(static_cast<char*>(x3) + row * resid_row_bytes(W) + (size_t)W * 2);
}
// MX block scales of e4m3 activations (vit_kernels.hpp quantize_rows_fp8mx_kernel, gemm256f8.hpp BSA): shared by every producer
__device__ __forceinline__ unsigned fp8mx_scale_byte(float amax) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    if (amax == 0.f) return 127u;
    return (unsigned)(e > 7 ? e - 7 : 0);
}
__device__ __forceinline__ float fp8mx_inv(unsigned sb) { return __uint_as_float((254u - sb) << 23); }
// 8 floats -> 8 e4m3 bytes (round to nearest even, saturating: v_cvt_pk_fp8_f32)
__device__ __forceinline__ uint2 fp8_pack8(const float* f) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    return make_uint2((unsigned)lo, (unsigned)hi);
}

// One wave, one 256-column segment of a residual row, four consecutive columns per lane (the layout of every whole-row store
// pass): the row's e4m3 bytes with MX block scales (a block = 8 lanes) and the segment's canonical (sum, sum of squares).
// Shared by the FP8 residual GEMM's store pass (EPI_BIAS_RESID_LN8) and rows_mx_stats_kernel (ln_pre's rows), so the bytes
// and the statistics do not depend on who produced them. Quantises the f32 values themselves (one rounding).
__device__ __forceinline__ void ln8_row_segment(f32x4 v, unsigned& packed4, unsigned& scale_byte, float& sum, float& sumsq) {
    sum = ln_wave_sum(ln_lane_sum(v));
    sumsq = ln_wave_sum(ln_lane_sumsq(v));
    float mx = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    scale_byte = fp8mx_scale_byte(mx);
    const float inv = fp8mx_inv(scale_byte);
    int pk = 0;
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(v.x * inv, v.y * inv, pk, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(v.z * inv, v.w * inv, pk, true);
    packed4 = (unsigned)pk;
}

// 8 consecutive bf16 columns per lane (one 16-byte chunk of a row's store pass), the 4 lanes of a quad = one 32-block:
// -> the 8 e4m3 bytes and the block's scale byte. The bytes quantize_rows_fp8mx_kernel makes of the same bf16 rows (block
// maximum on the bf16 MAGNITUDE BITS - 15-bit integers order as the values do - two packed 16-bit maxima, the quad's by DPP).
__device__ __forceinline__ uint2 mx_pack_bf16x8(uint4 x, unsigned& sb_out) {
    const unsigned w_[4] = {x.x, x.y, x.z, x.w};
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    u16x2 pm = __builtin_elementwise_max(
        __builtin_elementwise_max(__builtin_bit_cast(u16x2, w_[0] & 0x7fff7fffu), __builtin_bit_cast(u16x2, w_[1] & 0x7fff7fffu)),
        __builtin_elementwise_max(__builtin_bit_cast(u16x2, w_[2] & 0x7fff7fffu), __builtin_bit_cast(u16x2, w_[3] & 0x7fff7fffu)));
    unsigned mm = __builtin_bit_cast(unsigned, pm);
    mm = (mm & 0xffffu) > (mm >> 16) ? (mm & 0xffffu) : (mm >> 16);
    const unsigned m1_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mm, 0xB1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    mm = mm > m1_ ? mm : m1_;
    const unsigned m2_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mm, 0x4E, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    mm = mm > m2_ ? mm : m2_;
    const unsigned e_ = mm >> 7;
    const unsigned sb_ = mm == 0u ? 127u : (e_ > 7u ? e_ - 7u : 0u);      // = fp8mx_scale_byte(block max)
    const float inv_ = fp8mx_inv(sb_);
    float f[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const f32x2 p_ = f32x2{__uint_as_float(w_[j] << 16), __uint_as_float(w_[j] & 0xffff0000u)} * inv_;
        f[2 * j] = p_.x;
        f[2 * j + 1] = p_.y;
    }
    sb_out = sb_;
    return fp8_pack8(f);
}

struct GemmArgs {
    const unsigned short* A;   // bf16 [M][K]; rows lda_bytes apart when that is set (the hi halves of split-residual rows)
    const unsigned short* W;   // bf16 [N][K]
    const float* bias;         // [N] or nullptr
    void* out;
    int M, N, K;
    // EPI_PATCH_F32 only
    const float* pos;          // [L][N]
    int np, L;
    unsigned char* x8;         // EPI_BIAS_RESID_LN8: the new residual rows as e4m3 [M][N] ...
    unsigned char* x8_bs;      // ... and their e8m0 block scales [rows padded to 256][N / 32]
    int dbg;                   // development experiments only (tools/gemm_persist.py); 0 in every product path
    // FP8 path (gemm256f8.hpp): A and W point at e4m3 bytes; per-row / per-output-channel dequantisation scales
    const float* a_scale;      // [M]
    const float* w_scale;      // [N]
    // block-scaled activations (MX; gemm256f8.hpp BSA): one e8m0 byte per 32 consecutive k, rows padded to 256
    const unsigned char* a_bscale;   // consumer: [ceil(M / 256) * 256][K / 32]
    unsigned char* out_bscale;       // producer epilogues that emit e4m3 + block scales: [..][N / 32]
    // LN-folded layers: consumers (EPI_LN_*) read ln_part_in [M][K/256][2] (per-segment sum / sum of squares of the
    // f32 rows whose hi halves are A) and colsum [N] (bias = cb); the producer (EPI_BIAS_RESID_LN_F32) updates the
    // split residual x3 (rows of [N bf16 hi | N u8 lo]: split_join / split_make above) and writes ln_part [M][N/256][2];
    // tmp_f32 [M][N]: scratch for the producer's non-persistent form (GEMM into tmp, then split_stats_kernel)
    const float* ln_part_in;
    const float* colsum;
    void* x3;
    float* ln_part;
    float* tmp_f32;
    unsigned lda_bytes;        // 0: A rows are K elements apart; LN-folded consumers pass resid_row_bytes(K)
    // M <= 128 rows (one prompt, one image: gemm_skinny.hpp; round 5). The skinny residual producer updates the split rows IN
    // PLACE (each wave owns its 16 columns of 16 rows) and leaves the statistics as the canonical tree's LEAVES - (sum, sum of
    // squares) of every 4-column group, ln_leaf [M][N / 4][2] - instead of a split / statistics pass of its own; the skinny
    // LN-folded consumer behind it (ln_leaf_in set, ln_part_in ignored) runs the tree. One launch less per residual GEMM in a chain of
    // ~4-us launches, the same statistics bits as the tiled kernels' (batch-size invariance).
    float* ln_leaf;
    const float* ln_leaf_in;
};
// elements (bf16) between two A rows
__host__ __device__ inline size_t gemm_lda(const GemmArgs& g) { return g.lda_bytes ? (size_t)g.lda_bytes / 2 : (size_t)g.K; }

// Tile order shared by both GEMM kernels. (1) XCD split: hardware deals workgroups round-robin over
// the 8 XCDs (b and b+8 share an L2), so each XCD gets a CONTIGUOUS range of the logical order.
// (2) Inside that order tiles are blocked GM row-panels x GN column-panels, so the ~32 tiles an XCD runs
// at once share GM A panels and GN W panels and the weight matrix is swept once per GM row-panels
// instead of once per ~3 (r01 PMC: c_fc read 195 MB per launch with plain n-fastest order vs 38 MB
// algorithmic). Bijective for any grid; placement only affects speed.
__device__ __forceinline__ void gemm_tile_coords(int bid, int nwg, int mtiles, int ntn, int GM, int GN, int& bm, int& bn) {
    const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
    const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
    const int per_super = GM * ntn;
    const int sr = tile / per_super;
    const int r = tile - sr * per_super;
    const int left = mtiles - sr * GM;
    const int gm = left < GM ? left : GM;
    const int full = ntn / GN;
    int ng = r / (gm * GN);
    ng = ng < full ? ng : full;
    const int r2 = r - ng * gm * GN;
    const int gn = (ntn - ng * GN) < GN ? (ntn - ng * GN) : GN;
    const int mi = r2 / gn;
    bm = sr * GM + mi;
    bn = ng * GN + (r2 - mi * gn);
}

constexpr int GEMM_BM = 128, GEMM_BN = 128, GEMM_BK = 64;
constexpr int GEMM_TILE_BYTES = GEMM_BM * GEMM_BK * 2;          // 16 KiB per operand tile
constexpr int GEMM_LDS_BYTES = 4 * GEMM_TILE_BYTES;             // A,B x 2 buffers = 64 KiB

template <int EPI>
__global__ void __launch_bounds__(256) gemm_bf16_nt_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;       // 2x2 waves, each 64 (m) x 64 (n)
    const int fr = lane & 15, fg = lane >> 4;

    const int ntn = g.N / GEMM_BN;
    int bm, bn;
    gemm_tile_coords(blockIdx.x, gridDim.x, (g.M + GEMM_BM - 1) / GEMM_BM, ntn, 8, 8, bm, bn);
    const int m0 = bm * GEMM_BM, n0 = bn * GEMM_BN;
    const int K = g.K;

    // --- LDS-DMA staging: each wave-instruction moves 8 rows x 128 B. Wave w owns rows
    // [32w, 32w+32) of both tiles: 4 instructions per operand per K-tile.
    const int srow = lane >> 3;          // row within the 8-row piece
    const int spos = lane & 7;           // 16-byte chunk position in the LDS row
    const unsigned short* a_src[4];
    const unsigned short* w_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wave * 32 + i * 8 + srow;
        const int chunk = spos ^ (row & 7);                 // swizzle on the SOURCE (rule: DMA dest is lane-linear)
        int am = m0 + row;
        am = am < g.M ? am : g.M - 1;                        // M tail: duplicate the last row, masked in the epilogue
        a_src[i] = g.A + (size_t)am * gemm_lda(g) + chunk * 8;
        w_src[i] = g.W + (size_t)(n0 + row) * K + chunk * 8;
    }
    auto stage = [&](int kt, int buf) {
        char* abase = smem + buf * (2 * GEMM_TILE_BYTES) + wave * 32 * 128;
        char* bbase = abase + GEMM_TILE_BYTES;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + kt * GEMM_BK),
                                             (__attribute__((address_space(3))) void*)(abase + i * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w_src[i] + kt * GEMM_BK),
                                             (__attribute__((address_space(3))) void*)(bbase + i * 1024), 16, 0, 0);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment read offsets: row (16*t + fr) of the wave's 64-row slice, logical chunk 4*ks + fg
    const int sw = fr & 7;
    const int a_off = (wm * 64 + fr) * 128;
    const int b_off = GEMM_TILE_BYTES + (wn * 64 + fr) * 128;
    const int c0 = ((0 + fg) ^ sw) * 16, c1 = ((4 + fg) ^ sw) * 16;

    const int nk = K / GEMM_BK;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of tile kt have landed
        __syncthreads();                                      // ... everyone's have; tile kt-1 is fully consumed
        if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        const char* base = smem + (kt & 1) * (2 * GEMM_TILE_BYTES);
        bf16x8 af[4][2], wf[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            af[t][0] = *reinterpret_cast<const bf16x8*>(base + a_off + t * 2048 + c0);
            af[t][1] = *reinterpret_cast<const bf16x8*>(base + a_off + t * 2048 + c1);
            wf[t][0] = *reinterpret_cast<const bf16x8*>(base + b_off + t * 2048 + c0);
            wf[t][1] = *reinterpret_cast<const bf16x8*>(base + b_off + t * 2048 + c1);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nt][ks], af[mt][ks], acc[mt][nt], 0, 0, 0);
    }

    // --- epilogue: lane holds, per (mt, nt): row m = ..+fr, columns n = ..+4*fg+{0,1,2,3}.
    // Bias loaded once per lane; the residual read-modify-write is software-pipelined (see gemm256.hpp).
    f32x4 bz[4], cs[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wn * 64 + nt * 16 + 4 * fg;
        bz[nt] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        if (epi_is_ln(EPI)) cs[nt] = *reinterpret_cast<const f32x4*>(g.colsum + n);
    }
    constexpr bool RMW = (EPI == EPI_BIAS_RESID_F32) || (EPI == EPI_PATCH_F32);
    auto row_of = [&](int mt, size_t& orow, const float*& addrow, bool& valid) {
        const int m = m0 + wm * 64 + mt * 16 + fr;
        valid = m < g.M;
        const int mc = valid ? m : g.M - 1;
        orow = (size_t)mc;
        addrow = nullptr;
        if (EPI == EPI_PATCH_F32) {
            const int b_ = mc / g.np, p_ = mc - b_ * g.np;
            orow = (size_t)b_ * g.L + 1 + p_;
            addrow = g.pos + (size_t)(1 + p_) * g.N;
        } else if (EPI == EPI_BIAS_RESID_F32) {
            addrow = static_cast<const float*>(g.out) + orow * g.N;
        }
    };
    f32x4 cur[4], nxt[4];
    if (RMW) {
        size_t orow; const float* addrow; bool valid;
        row_of(0, orow, addrow, valid);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) cur[nt] = *reinterpret_cast<const f32x4*>(addrow + n0 + wn * 64 + nt * 16 + 4 * fg);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        size_t orow; const float* addrow; bool valid;
        row_of(mt, orow, addrow, valid);
        if (RMW && mt + 1 < 4) {
            size_t orow2; const float* addrow2; bool valid2;
            row_of(mt + 1, orow2, addrow2, valid2);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) nxt[nt] = *reinterpret_cast<const f32x4*>(addrow2 + n0 + wn * 64 + nt * 16 + 4 * fg);
        }
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const int n = n0 + wn * 64 + nt * 16 + 4 * fg;
            f32x4 v;
            if (epi_is_ln(EPI)) {
                const int nseg = g.K >> 8;
                const f32x2 st = ln_row_stats(g.ln_part_in + orow * 2 * nseg, nseg, g.K);
                v = ln_apply(acc[mt][nt], st.x, st.y, cs[nt], bz[nt]);
            } else {
                v = acc[mt][nt] + bz[nt];
            }
            if (epi_is_bf16_out(EPI)) {
                if (epi_is_qgelu(EPI)) {
                    v = quick_gelu4(v);
                }
                if (valid)
                    *reinterpret_cast<uint2*>(static_cast<unsigned short*>(g.out) + orow * g.N + n) =
                        make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
            } else {
                if (RMW) v += cur[nt];
                if (valid) *reinterpret_cast<f32x4*>(static_cast<float*>(g.out) + orow * g.N + n) = v;
            }
        }
        if (RMW) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) cur[nt] = nxt[nt];
        }
    }
}

// host-side launcher (defined in gemm.hip)
// Measurement probe (bench.py roofline), passed down by the caller that wants it (nullptr everywhere else: the
// library keeps no mutable state of its own): every launch whose epilogue is `epi` (or its LN-folded twin) is
// bracketed by a pair of HIP events on its own stream.
struct GemmProbe {
    static constexpr int MAX = 96;
    static constexpr int EPI_ATTENTION = 100;     // pseudo-epilogue of a probed attention launch (mode 2: the kernel in front of out_proj)
    int epi = -1, n = 0;
    // mode 0: events from hipExtLaunchKernel (the dispatch's own begin / end) around the launches whose epilogue matches
    //         `epi`; mode 1: the same plus a plain event record in front (`pre`: completion of everything before);
    //         mode 2: begin / end events around EVERY GEMM launch (for completion-to-completion differences)
    int mode = 0;
    hipEvent_t ev[2 * MAX];
    hipEvent_t pre[MAX];
    int epi_of[MAX];          // the epilogue that really ran (EPI_LN_* when the tower folds its LayerNorms)
    int kernel_of[MAX];       // 0 gemm_bf16_nt_kernel (128^2), 1 gemm256_bf16_nt_kernel, 2 gemm256p_bf16_nt_kernel
    int k_of[MAX];            // the launch's K (out_proj and c_proj share an epilogue and differ in K)
    static int base_of(int e) {
        return e == EPI_LN_BIAS_BF16 ? EPI_BIAS_BF16 : e == EPI_LN_BIAS_QGELU_BF16 ? EPI_BIAS_QGELU_BF16 :
               e == EPI_BIAS_RESID_LN_F32 ? EPI_BIAS_RESID_F32 : e;
    }
    bool wants(int e) const { return n < MAX && (mode == 2 || base_of(e) == epi); }
    // called by the launchers right before a probed launch; returns the slot
    int begin(int e, int kernel, hipStream_t st, int K = 0) {
        epi_of[n] = e;
        kernel_of[n] = kernel;
        k_of[n] = K;
        if (mode == 1) (void)hipEventRecord(pre[n], st);
        return n++;
    }
};

int launch_gemm_algo(const GemmArgs& g, int epi, int algo, hipStream_t st, GemmProbe* probe = nullptr);
int launch_gemm_fp8(const GemmArgs& g, int epi, hipStream_t st, int mx = 1);      // gemm256f8.hpp: e4m3 operands + scales
bool gemm_resid_writes_leaves(int M, int N, int K);   // the residual GEMM of this shape runs on the skinny kernel and can take ln_leaf
bool gemm_fp8_emits_mx(int M, int N, int K);     // the QuickGELU form of this shape can write e4m3 + MX block scales (out_bscale)
// vit_kernels.hip: f32 rows -> split residual rows x3 ([W bf16 hi | W u8 lo] each) + canonical statistics partials
// [M][W/256][2]; with `add` (the non-persistent form of EPI_BIAS_RESID_LN_F32) the rows are add[m][:] + x3[m][:], updated in place
int launch_split_stats(const float* x_or_add, bool add, void* x3, float* part, int M, int W, hipStream_t st);

}  // namespace clipmi
