// attention.hpp — the four attention kernels of the CLIP towers (gfx950) and the pieces they share. Included by
// vit_kernels.hip only (launch_attention, clipmi_dbg_attention).
#pragma once
#include "vit_kernels.hpp"

namespace clipmi {

// ---------------------------------------------------------------------------------------------
// Fused attention for short sequences (L <= 16*NT; ViT-B/32: L = 50, text: L = 77), head dim 64.
// One wave per (sequence, head). qkv bf16 [B*L][3W] (q | k | v, head h at columns 64h..64h+63
// of each third) -> out bf16 [B*L][W].
//
// S^T = K Q^T is computed with the KEY on the accumulator rows and the QUERY on its column
// (lane & 15): the softmax reduction over keys is then 4*NT in-lane values plus two xor-shuffles,
// and the P^T accumulator registers ARE the B operand of O^T = V^T P^T with no data movement
// (k-slot j of lane group g is key 16*(2s + (j>>2)) + 4g + (j&3), for both operands).
// K and Q fragments come straight from global memory (16 B per lane); V goes through a per-wave
// LDS tile and is read transposed with ds_read_b64_tr_b16 (TR = 1) or 2-byte reads (TR = 0).
// Scores, softmax and normalisation are f32; P and the output are rounded to bf16.
// ---------------------------------------------------------------------------------------------
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---- the pieces the kernels below share (all registers, all inlined) ----

// V fragment of one 32-key step and one 16-d tile (the A operand of O^T = V^T P^T): two ds_read_b64_tr_b16 of the row-major
// V tile. 16-lane group fg reads the 4-key x 16-d block at keys 4 fg .. + 3 of a key tile; lane i of the group supplies the
// address of key (i >> 2), d 4 (i & 3) and receives d = i. a0 / a1: this lane's address in the step's two key tiles.
__device__ __forceinline__ bf16x8 attn_v_frag(const char* a0, const char* a1) {
    const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0));
    const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a1));
    const s16x8 t = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
    return __builtin_bit_cast(bf16x8, t);
}

// P fragment of one 32-key step (the B operand): the step's two score tiles of one query tile, rounded to bf16
__device__ __forceinline__ bf16x8 attn_p_frag(f32x4 lo, f32x4 hi) {
    const uint4 u = make_uint4(pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w));
    return __builtin_bit_cast(bf16x8, u);
}

// Softmax of one query column of a short sequence, in place (f32): s[kt][r] is key 16 kt + 4 fg + r against query qi.
// Scale 1/8, mask (keys >= L; CAUSAL: keys > qi), max, exp, sum, 1 / sum.
template <int NT, bool CAUSAL>
__device__ __forceinline__ void attn_softmax_column(f32x4 (&s)[NT], int qi, int L, int fg) {
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int ki = kt * 16 + 4 * fg + r;
            float x = s[kt][r] * 0.125f;
            if (ki >= L || (CAUSAL && ki > qi)) x = -INFINITY;
            s[kt][r] = x;
            mx = fmaxf(mx, x);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(s[kt][r] - mx);     // key 0 is never masked: mx is finite
            s[kt][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) s[kt] *= inv;
}

// One 16-query tile of the ViT-B/32 shape (49 <= L <= 52: 4 key tiles, no mask): scores against the four K tiles, the
// softmax column, and the two 32-key steps of O^T = V^T P^T into o[dt] (rows = d 16 dt + 4 fg + r, column = the query).
// krow: this lane's V row in each key tile (rows >= 52 redirected to row 51: weight 0, finite filler); vcol: the tile's
// base + this lane's d offset.
__device__ __forceinline__ void attn52_tile(const bf16x8 (&kf)[4][2], bf16x8 q0, bf16x8 q1, const int (&krow)[4],
                                            const char* vcol, int L, int fg, f32x4 (&o)[4]) {
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][0], q0, a, 0, 0, 0);
        a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][1], q1, a, 0, 0, 0);
        s[kt] = a;
    }
    attn_softmax_column<4, false>(s, 0, L, fg);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const bf16x8 pf = attn_p_frag(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const bf16x8 vf = attn_v_frag(vcol + krow[2 * ks] * 128 + dt * 32, vcol + krow[2 * ks + 1] * 128 + dt * 32);
            o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
        }
    }
}

// One query's 64 output columns as bf16: the lane holds d 16 dt + 4 fg .. + 3 of tile dt, dst points at column 4 fg of the
// row. Four 8-byte stores. (attention_flash_kernel keeps its own copy with the 1 / l factor: through this function its
// multiplies came out with swapped operands and three more s_nop - profiles/attention_one_tile_resources.txt.)
__device__ __forceinline__ void attn_store_row(unsigned short* dst, f32x4 o0, f32x4 o1, f32x4 o2, f32x4 o3) {
    const f32x4 o[4] = {o0, o1, o2, o3};
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf16x2(o[dt].x, o[dt].y), pack_bf16x2(o[dt].z, o[dt].w));
}

// attention_kernel (the comment at the top): all NT x NT score tiles of a (sequence, head) at once in one wave
template <int NT, bool CAUSAL, bool TR>
__global__ void __launch_bounds__(256) attention_kernel(const unsigned short* __restrict__ qkv,
                                                        unsigned short* __restrict__ out, int B, int L, int heads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = (NT + 1) / 2;            // 32-key steps of the second product
    constexpr int ROWS = KS * 32;               // V rows staged (>= 16*NT), zero-weight beyond L
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int W = heads * 64;
    const long long item = (long long)blockIdx.x * 4 + wave;      // (b, h)
    if (item >= (long long)B * heads) return;                       // wave-uniform; no block barriers below
    const int b = (int)(item / heads), h = (int)(item - (long long)b * heads);
    const unsigned short* base = qkv + (size_t)b * L * 3 * W + h * 64;
    const size_t rs = (size_t)3 * W;                                // row stride (elements)
    char* vt = smem + wave * (ROWS * 128);

    // ---- stage V rows [0, ROWS) of this head: 8 rows x 128 B per wave-instruction
#pragma unroll
    for (int i = 0; i < ROWS / 8; ++i) {
        int row = i * 8 + (lane >> 3);
        const int srcrow = row < L ? row : L - 1;
        const uint4 d = *reinterpret_cast<const uint4*>(base + (size_t)srcrow * rs + 2 * W + (lane & 7) * 8);
        *reinterpret_cast<uint4*>(vt + row * 128 + (lane & 7) * 16) = d;
    }

    // ---- S^T tiles: acc[kt][qt], rows = keys 16kt + 4fg + r, column = query 16qt + fr
    bf16x8 kf[NT][2], qf[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int row = t * 16 + fr;
        row = row < L ? row : L - 1;
        const unsigned short* pr = base + (size_t)row * rs + fg * 8;
        qf[t][0] = *reinterpret_cast<const bf16x8*>(pr);
        qf[t][1] = *reinterpret_cast<const bf16x8*>(pr + 32);
        kf[t][0] = *reinterpret_cast<const bf16x8*>(pr + W);
        kf[t][1] = *reinterpret_cast<const bf16x8*>(pr + W + 32);
    }
    f32x4 s[NT][NT];                                                // s[qt][kt]: a query tile's column of score tiles
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int qt = 0; qt < NT; ++qt) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][0], qf[qt][0], a, 0, 0, 0);
            a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kt][1], qf[qt][1], a, 0, 0, 0);
            s[qt][kt] = a;
        }

    // ---- softmax over keys for each query column
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) attn_softmax_column<NT, CAUSAL>(s[qt], qt * 16 + fr, L, fg);

    // ---- O^T = V^T P^T: acc o[dt][qt], rows = d 16dt + 4fg + r, column = query
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this wave's V tile is in LDS
    __builtin_amdgcn_wave_barrier();
    f32x4 o[4][NT];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int qt = 0; qt < NT; ++qt) o[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        bf16x8 pf[NT];
#pragma unroll
        for (int qt = 0; qt < NT; ++qt) {
            const int k1 = 2 * ks + 1;        // an odd NT's last step has one key tile: the other half of P is zero
            pf[qt] = attn_p_frag(s[qt][2 * ks], k1 < NT ? s[qt][k1 % NT] : f32x4{0.f, 0.f, 0.f, 0.f});
        }
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            bf16x8 vf;
            if (TR) {
                const int k0 = 32 * ks + 4 * fg + (fr >> 2);
                const char* ad = vt + k0 * 128 + (dt * 16 + 4 * (fr & 3)) * 2;
                vf = attn_v_frag(ad, ad + 16 * 128);
            } else {                          // the same fragment by eight 2-byte reads: the tests' reference for the above
                unsigned short e[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int key = 16 * (2 * ks + (j >> 2)) + 4 * fg + (j & 3);
                    e[j] = *reinterpret_cast<const unsigned short*>(vt + key * 128 + (dt * 16 + fr) * 2);
                }
                const uint4 u = make_uint4(e[0] | ((unsigned)e[1] << 16), e[2] | ((unsigned)e[3] << 16),
                                           e[4] | ((unsigned)e[5] << 16), e[6] | ((unsigned)e[7] << 16));
                vf = __builtin_bit_cast(bf16x8, u);
            }
#pragma unroll
            for (int qt = 0; qt < NT; ++qt)
                o[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt], o[dt][qt], 0, 0, 0);
        }
    }

    // ---- store: lane holds 4 consecutive d for query 16qt + fr
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
        const int qi = qt * 16 + fr;
        if (qi >= L) continue;
        attn_store_row(out + ((size_t)b * L + qi) * W + h * 64 + 4 * fg, o[0][qt], o[1][qt], o[2][qt], o[3][qt]);
    }
}

// ---------------------------------------------------------------------------------------------
// attention52_kernel: the ViT-B/32 shape (49 <= L <= 52, 4 key/query tiles, no mask) with the query tiles
// walked in a LOOP instead of all at once. attention_kernel<4,...> keeps 16 score tiles + 16 output tiles +
// 16 fragments live (~120 registers with the AGPRs: 4 waves per SIMD) and stages 64 V rows per wave (32 KiB per
// workgroup: 4 workgroups per CU); its lifetime per wave is ~20 us of mostly latency, so residency is its
// throughput (tools/attn_cliff.py: steps at every 16 waves per CU). Here per query tile: 4 score tiles, softmax,
// 4 output tiles, store; K fragments loaded once, the next tile's Q fragments in flight during the current tile,
// V staged once as 52 rows (6.5 KiB per wave -> 26 KiB per workgroup, six workgroups = 24 waves per CU); keys
// >= L carry zero weight and their transposed reads are redirected to row 51 (finite filler). Same arithmetic
// per (query, key, d) as attention_kernel: bit-identical output.
// ---------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256, 6) attention52_kernel(const unsigned short* __restrict__ qkv,
                                                                    unsigned short* __restrict__ out, int B, int L,
                                                                    int heads) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 4, ROWS = 52;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int W = heads * 64;
    const long long item = (long long)blockIdx.x * 4 + wave;      // (b, h)
    if (item >= (long long)B * heads) return;                       // wave-uniform; no block barriers below
    const int b = (int)(item / heads), h = (int)(item - (long long)b * heads);
    const unsigned short* base = qkv + (size_t)b * L * 3 * W + h * 64;
    const size_t rs = (size_t)3 * W;
    char* vt = smem + wave * (ROWS * 128);

    // ---- stage V rows [0, 52): 8 rows x 128 B per wave-instruction, the last one half masked
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int row = i * 8 + (lane >> 3);
        const int srcrow = row < L ? row : L - 1;                   // rows L..51: finite filler, weight 0
        const uint4 d = *reinterpret_cast<const uint4*>(base + (size_t)srcrow * rs + 2 * W + (lane & 7) * 8);
        if (row < ROWS) *reinterpret_cast<uint4*>(vt + row * 128 + (lane & 7) * 16) = d;
    }
    // ---- K fragments of all four key tiles (kept), Q fragments of tile 0
    bf16x8 kf[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int row = t * 16 + fr;
        row = row < L ? row : L - 1;
        const unsigned short* pr = base + (size_t)row * rs + W + fg * 8;
        kf[t][0] = *reinterpret_cast<const bf16x8*>(pr);
        kf[t][1] = *reinterpret_cast<const bf16x8*>(pr + 32);
    }
    auto q_ptr = [&](int qt) {
        int row = qt * 16 + fr;
        row = row < L ? row : L - 1;
        return base + (size_t)row * rs + fg * 8;
    };
    bf16x8 qn0 = *reinterpret_cast<const bf16x8*>(q_ptr(0));
    bf16x8 qn1 = *reinterpret_cast<const bf16x8*>(q_ptr(0) + 32);
    // transposed-read addresses of the two 32-key steps (see attention_kernel); key rows >= 52 -> row 51
    const int k00 = 4 * fg + (fr >> 2);
    const int krow[4] = {k00, k00 + 16, k00 + 32, (k00 + 48 < ROWS ? k00 + 48 : ROWS - 1)};
    const char* vcol = vt + (4 * (fr & 3)) * 2;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this wave's V tile is in LDS
    __builtin_amdgcn_wave_barrier();

#pragma unroll 1
    for (int qt = 0; qt < NT; ++qt) {
        const bf16x8 q0 = qn0, q1 = qn1;
        if (qt + 1 < NT) {
            qn0 = *reinterpret_cast<const bf16x8*>(q_ptr(qt + 1));
            qn1 = *reinterpret_cast<const bf16x8*>(q_ptr(qt + 1) + 32);
        }
        f32x4 o[4];
        attn52_tile(kf, q0, q1, krow, vcol, L, fg, o);
        const int qi = qt * 16 + fr;
        if (qi < L) attn_store_row(out + ((size_t)b * L + qi) * W + h * 64 + 4 * fg, o[0], o[1], o[2], o[3]);
    }
}

// ---------------------------------------------------------------------------------------------
// attention52x4_kernel: the ViT-B/32 attention (49 <= L <= 52, no mask) with ONE WORKGROUP per (image, head) and one
// 16-query tile per wave. attention52_kernel gives a whole (image, head) to one wave: 17 dependent-latency global loads
// in 64-byte pieces, then four query tiles one after the other - a wave lives ~20 us and the launch is bound by that
// residency (65 us per layer at B = 870 = 4.1 TB/s). Here the four waves stage K (64 rows, 16-byte chunks XOR-swizzled by
// row & 7 for conflict-free ds_read_b128 fragments) and V (52 rows, row-major for ds_read_b64_tr_b16) ONCE as whole
// 128-byte head rows, <= 4 loads per lane, one barrier, and each wave then runs exactly one iteration of
// attention52_kernel's query-tile loop: same MFMA sequence, same softmax: bit-identical output, a quarter of the serial
// chain. 14.5 KiB of LDS per workgroup, 8 workgroups (32 waves) per CU.
// ---------------------------------------------------------------------------------------------
template <bool OUT8>
static __global__ void __launch_bounds__(256, 5) attention52x4_kernel(const unsigned short* __restrict__ qkv,
                                                                      unsigned short* __restrict__ out, int B, int L,
                                                                      int heads, unsigned char* __restrict__ out8, unsigned char* __restrict__ out_bs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 4, ROWS = 52;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int W = heads * 64;
    const size_t rs = (size_t)3 * W;
    char* kt_ = smem;                       // K: 64 rows x 128 B, swizzled
    char* vt = smem + 64 * 128;             // V: 52 rows x 128 B
    const int srow = lane >> 3, sch = lane & 7;
    const int items = B * heads;

    // A workgroup walks items blockIdx.x, + gridDim.x, ... (the grid is sized to the chip's residency): the NEXT item's six
    // loads per lane (Q fragments, K / V staging pieces) are issued before the current item's math, so that the HBM round
    // trip of item i + 1 runs under the MFMA / softmax / LDS work of item i instead of in front of it.
    // (a macro, not a lambda: by-reference captures of the register arrays put them in scratch)
    bf16x8 q0n, q1n;
    uint4 kdn0, kdn1, vdn0, vdn1;
#define ATT52_FETCH(IT)                                                                                  \
    do {                                                                                                 \
        const int b_ = (IT) / heads, h_ = (IT) - b_ * heads;                                             \
        const unsigned short* base_ = qkv + (size_t)b_ * L * 3 * W + h_ * 64;                            \
        int qrow_ = wave * 16 + fr;                                                                      \
        qrow_ = qrow_ < L ? qrow_ : L - 1;                                                               \
        const unsigned short* qp_ = base_ + (size_t)qrow_ * rs + fg * 8;                                 \
        q0n = *reinterpret_cast<const bf16x8*>(qp_);                                                     \
        q1n = *reinterpret_cast<const bf16x8*>(qp_ + 32);                                                \
        int r0_ = (wave * 2) * 8 + srow, r1_ = (wave * 2 + 1) * 8 + srow;   /* K rows 0..63, V rows 0..55 */ \
        r0_ = r0_ < L ? r0_ : L - 1;                                        /* rows >= L: finite filler */ \
        r1_ = r1_ < L ? r1_ : L - 1;                                                                     \
        kdn0 = *reinterpret_cast<const uint4*>(base_ + (size_t)r0_ * rs + W + sch * 8);                  \
        vdn0 = *reinterpret_cast<const uint4*>(base_ + (size_t)r0_ * rs + 2 * W + sch * 8);              \
        kdn1 = *reinterpret_cast<const uint4*>(base_ + (size_t)r1_ * rs + W + sch * 8);                  \
        vdn1 = *reinterpret_cast<const uint4*>(base_ + (size_t)r1_ * rs + 2 * W + sch * 8);              \
    } while (0)
    int item = blockIdx.x;
    if (item >= items) return;
    ATT52_FETCH(item);
    for (;;) {
        const int b = item / heads, h = item - b * heads;
        const bf16x8 q0 = q0n, q1 = q1n;
        {
            const int row0 = (wave * 2) * 8 + srow, row1 = row0 + 8;
            *reinterpret_cast<uint4*>(kt_ + row0 * 128 + ((sch ^ (row0 & 7)) << 4)) = kdn0;
            *reinterpret_cast<uint4*>(kt_ + row1 * 128 + ((sch ^ (row1 & 7)) << 4)) = kdn1;
            if (row0 < ROWS) *reinterpret_cast<uint4*>(vt + row0 * 128 + sch * 16) = vdn0;
            if (row1 < ROWS) *reinterpret_cast<uint4*>(vt + row1 * 128 + sch * 16) = vdn1;
        }
        const int nxt = item + gridDim.x;
        const bool has_next = nxt < items;
        if (has_next) ATT52_FETCH(nxt);
        __syncthreads();

        // K fragments of all four key tiles out of LDS: row t*16 + fr, logical chunks fg and 4 + fg
        bf16x8 kf[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int row = t * 16 + fr;
            kf[t][0] = *reinterpret_cast<const bf16x8*>(kt_ + row * 128 + (((0 + fg) ^ (row & 7)) << 4));
            kf[t][1] = *reinterpret_cast<const bf16x8*>(kt_ + row * 128 + (((4 + fg) ^ (row & 7)) << 4));
        }
        const int k00 = 4 * fg + (fr >> 2);
        const int krow[4] = {k00, k00 + 16, k00 + 32, (k00 + 48 < ROWS ? k00 + 48 : ROWS - 1)};
        const char* vcol = vt + (4 * (fr & 3)) * 2;
        f32x4 o[4];
        attn52_tile(kf, q0, q1, krow, vcol, L, fg, o);      // this wave's iteration of attention52_kernel's query-tile loop

        // Output row qi, columns 16 dt + 4 fg .. + 3 per accumulator tile: as they stand that is four 8-byte stores per lane,
        // 32 contiguous bytes per row and instruction (store-issue-bound tail: the one-wave and the four-wave form took the
        // same 90 us from cold caches). Lanes fg and fg ^ 1 (lane ^ 16) swap halves - the even one gives away tiles 1, 3 and
        // receives the partner's 0, 2 - so that every lane owns 8 consecutive columns of two tiles: two 16-byte stores, 64
        // contiguous bytes per row and instruction.
        const int qi = wave * 16 + fr;
        uint2 pk[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) pk[dt] = make_uint2(pack_bf16x2(o[dt].x, o[dt].y), pack_bf16x2(o[dt].z, o[dt].w));
        const bool odd = fg & 1;
        uint2 mine[2], theirs[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint2 give = odd ? pk[2 * j] : pk[2 * j + 1];
            mine[j] = odd ? pk[2 * j + 1] : pk[2 * j];
            theirs[j] = make_uint2(__shfl_xor(give.x, 16), __shfl_xor(give.y, 16));
        }
        if (OUT8) {
            // FP8 towers: the rows leave as e4m3 with MX block scales (the A operand of out_proj, gemm256f8.hpp BSA) - the bytes
            // quantize_rows_fp8mx_kernel makes of the bf16 rows. A head's 64 columns are two 32-blocks; block j of row qi is
            // the 8 columns of tile 2 j (even fg) or 2 j + 1 (odd fg) in the four lanes fr, fr + 16, fr + 32, fr + 48.
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int dt = 2 * j + (odd ? 1 : 0);
                const uint4 v = odd ? make_uint4(theirs[j].x, theirs[j].y, mine[j].x, mine[j].y)
                                    : make_uint4(mine[j].x, mine[j].y, theirs[j].x, theirs[j].y);
                const unsigned w_[4] = {v.x, v.y, v.z, v.w};
                float f[8];
                float mxa = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    f[2 * i] = __uint_as_float(w_[i] << 16);
                    f[2 * i + 1] = __uint_as_float(w_[i] & 0xffff0000u);
                    mxa = fmaxf(mxa, fmaxf(fabsf(f[2 * i]), fabsf(f[2 * i + 1])));
                }
                mxa = fmaxf(mxa, __shfl_xor(mxa, 16));
                mxa = fmaxf(mxa, __shfl_xor(mxa, 32));
                const unsigned sb_ = fp8mx_scale_byte(mxa);
                const float inv_ = fp8mx_inv(sb_);
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] *= inv_;
                if (qi < L) {
                    const size_t row_ = (size_t)b * L + qi;
                    *reinterpret_cast<uint2*>(out8 + row_ * W + h * 64 + 4 * (fg & ~1) + dt * 16) = fp8_pack8(f);
                    if (fg == 0) out_bs[row_ * (W >> 5) + h * 2 + j] = (unsigned char)sb_;
                }
            }
        } else if (qi < L) {
            // even fg: tiles 0, 2 at columns 16 dt + 4 fg .. + 7 (own 4, then the partner's); odd fg: tiles 1, 3 at 16 dt + 4 (fg - 1)
            unsigned short* dst = out + ((size_t)b * L + qi) * W + h * 64 + 4 * (fg & ~1);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int dt = 2 * j + (odd ? 1 : 0);
                const uint4 v = odd ? make_uint4(theirs[j].x, theirs[j].y, mine[j].x, mine[j].y)
                                    : make_uint4(mine[j].x, mine[j].y, theirs[j].x, theirs[j].y);
                *reinterpret_cast<uint4*>(dst + dt * 16) = v;
            }
        }
        if (!has_next) break;
        item = nxt;
        __syncthreads();                    // every wave is done with this item's K / V tiles
    }
#undef ATT52_FETCH
}

// ---------------------------------------------------------------------------------------------
// Flash-style attention for long sequences (L > 80: ViT-B/16 L = 197, ViT-L/14 L = 257,
// ViT-L/14@336 L = 577), head dim 64, no mask. A workgroup of WPB waves owns one (sequence, head) and
// WPB consecutive 64-query blocks (one per wave); keys/values stream through in 64-key blocks that the
// workgroup stages ONCE into double-buffered LDS by LDS-DMA (issued before the block's math, one
// barrier per block), so K and V are read from L2 once per workgroup
// instead of once per query block. Online softmax in f32 with exp2 (scale and log2 e folded into one
// FMA). Same operand orientation as attention_kernel: S^T = K Q^T puts the key on the accumulator rows,
// so a block's P^T registers are the B operand of O^T += V^T P^T as they stand, and the per-query
// rescale 2^(m_old - m_new) multiplies whole accumulator tiles of this lane's column.
// K tile rows are 128 B with 16-byte chunks XOR-swizzled by row & 7 (conflict-free ds_read_b128 fragments);
// the V tile is row-major for ds_read_b64_tr_b16.
// ---------------------------------------------------------------------------------------------
// QT = 16-query tiles per wave: 2 (32 queries; 128 VGPRs, four waves per SIMD: with K/V staged once per workgroup either
// way, the smaller wave tile buys twice the resident waves of round 1's QT = 4 to overlap one wave's softmax with
// another's MFMAs). The block loop is VALU-bound (34 v_exp_f32 per 32 MFMAs per wave), so everything else was taken out
// of it: per-element masking selects (the last block is a separate instantiation), the staging addresses' integer
// multiplies (one per-lane base + uniform offsets), and the dependent MFMA pairs of S^T: 731 -> 437 instructions per block.
template <int WPB, int QT>
__global__ void __launch_bounds__(WPB * 64, QT == 2 ? 4 : 2) attention_flash_kernel(const unsigned short* __restrict__ qkv,
                                                                    unsigned short* __restrict__ out, int B, int L,
                                                                    int heads, int qgroups) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // 2 x [K 8 KiB | V 8 KiB]
    constexpr int NT = 4;          // key tiles of 16 per 64-key block
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int W = heads * 64;
    const int qgi = blockIdx.x % qgroups;
    const int bh = blockIdx.x / qgroups;
    const int b = bh / heads, h = bh - b * heads;
    const unsigned short* base = qkv + (size_t)b * L * 3 * W + h * 64;
    const size_t rs = (size_t)3 * W;
    const int q0 = (qgi * WPB + wave) * (16 * QT);
    const bool wave_active = q0 < L;                  // idle waves still stage tiles and hit barriers

    bf16x8 qf[QT][2];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        int row = q0 + t * 16 + fr;
        row = row < L ? row : L - 1;
        const unsigned short* pr = base + (size_t)row * rs + fg * 8;
        qf[t][0] = *reinterpret_cast<const bf16x8*>(pr);
        qf[t][1] = *reinterpret_cast<const bf16x8*>(pr + 32);
    }
    f32x4 o[4][QT];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) o[dt][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -INFINITY; l_run[qt] = 0.f; }

    // staging by LDS-DMA (no VGPRs): a K/V block is 16 pieces of 1 KiB (8 rows x 128 B); pieces 0..7 are
    // K (16-byte chunks XOR-swizzled with row & 7 — applied on the SOURCE address, the DMA destination is
    // lane-linear), pieces 8..15 are V (plain rows). Wave w issues pieces [w*PPW, (w+1)*PPW).
    // Source addresses: each lane keeps the address of its 16 bytes of every piece for key block 0 and adds the block's
    // offset (one 64-bit add per piece); only a block that reaches past row L - 1 recomputes clamped rows. (Recomputing
    // row * row_stride per piece and block cost 20 quarter-rate integer multiplies per block: with the masking selects
    // below, ~900 of the ~2900 VALU cycles of a block against 512 MFMA cycles.)
    constexpr int PPW = 16 / WPB;
    static_assert(PPW <= 8, "a wave's pieces are all K or all V");
    // this lane's 16 bytes of the wave's FIRST piece for key block 0; piece i is 8 rows further (row & 7 and with it the
    // swizzle stay the same), block k0 is k0 rows further
    const int pc0 = wave * PPW, isv0 = pc0 >> 3;
    const int row0 = (pc0 & 7) * 8 + (lane >> 3);
    const unsigned short* const src0 = base + (size_t)row0 * rs + (1 + isv0) * W + (isv0 ? (lane & 7) : ((lane & 7) ^ (row0 & 7))) * 8;
    auto issue_tiles = [&](int k0, int buf) {
        if (k0 + 64 <= L) {                                   // wave-uniform: every row of the block exists
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                const size_t uoff = (size_t)((unsigned)(k0 + 8 * i) * (unsigned)rs);      // uniform: scalar unit
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src0 + uoff),
                                                 (__attribute__((address_space(3))) void*)(smem + buf * 16384 + (pc0 + i) * 1024), 16, 0, 0);
            }
        } else {
            asm volatile("" ::: "memory");                    // keep the clamped form out of the common path
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                int row = k0 + row0 + 8 * i;
                row = row < L ? row : L - 1;                  // rows past the last one read the last one (masked below)
                const unsigned short* src = src0 + (size_t)((unsigned)(row - row0) * (unsigned)rs);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(smem + buf * 16384 + (pc0 + i) * 1024), 16, 0, 0);
            }
        }
    };
    issue_tiles(0, 0);

    const float c = 0.125f * 1.4426950408889634f;     // 1/sqrt(64) * log2(e)
    const int nb = (L + 63) >> 6;
    // one 64-key block; MASK (compile time) = the block reaches past key L - 1: only the last block can, so the loop over
    // the others carries no per-element selects (if-converted, they were 67 VALU instructions per block)
    auto block = [&](auto mask_tag, int j) {
        constexpr bool MASK = decltype(mask_tag)::value;
        const int k0 = j << 6;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of block j have landed
        __syncthreads();                                      // ... everyone's have; block j-1 is fully consumed
        if (j + 1 < nb) issue_tiles(k0 + 64, (j + 1) & 1);   // in flight under this block's math
        const char* kb = smem + (j & 1) * 16384;
        const char* vt = kb + 8192;
        if (wave_active) {
            // S^T tiles: the first halves (head dims 0..31) of all NT x QT accumulators, then the second halves, so that
            // no MFMA waits for the one before it (the two halves of one accumulator back to back did)
            f32x4 s[NT][QT];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int kt = 0; kt < NT; ++kt) {
                    const int row = kt * 16 + fr;
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(kb + row * 128 + (((4 * hf + fg) ^ (row & 7)) << 4));
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt)
                        s[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][hf], hf ? s[kt][qt] : f32x4{0.f, 0.f, 0.f, 0.f},
                                                                            0, 0, 0);
                }
            if constexpr (MASK) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (k0 + kt * 16 + 4 * fg + r >= L) s[kt][qt][r] = -INFINITY;
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][qt][r]);
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                mx *= c;                                            // running max kept in the exp2 domain
                const float m_new = fmaxf(m_run[qt], mx);           // finite: every block holds >= 1 valid key
                const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_new);   // 0 on the first block
                float sum = 0.f;
#pragma unroll
                for (int kt = 0; kt < NT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __builtin_amdgcn_exp2f(fmaf(s[kt][qt][r], c, -m_new));
                        s[kt][qt][r] = e;
                        sum += e;
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                l_run[qt] = l_run[qt] * alpha + sum;
                m_run[qt] = m_new;
                // the running maximum of most rows stops moving after the first few key blocks: alpha is then exactly 1 and
                // the 16 multiplies per query tile are skipped wave-wide (x * 1 is exact: the same bits, 64 VALU cycles less
                // in a loop that is bound by its VALU issue, not by its 32 MFMAs)
                if (__ballot(alpha != 1.0f)) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) o[dt][qt] *= alpha;
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 pf[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) pf[qt] = attn_p_frag(s[2 * ks][qt], s[2 * ks + 1][qt]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const int kk = 32 * ks + 4 * fg + (fr >> 2);
                    const char* ad = vt + kk * 128 + (dt * 16 + 4 * (fr & 3)) * 2;
                    const bf16x8 vf = attn_v_frag(ad, ad + 16 * 128);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt)
                        o[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt], o[dt][qt], 0, 0, 0);
                }
            }
        }
    };
    for (int j = 0; j + 1 < nb; ++j) block(std::false_type{}, j);
    if ((nb << 6) > L) block(std::true_type{}, nb - 1);
    else block(std::false_type{}, nb - 1);

    if (!wave_active) return;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int qi = q0 + qt * 16 + fr;
        if (qi >= L) continue;
        const float inv = 1.0f / l_run[qt];
        unsigned short* dst = out + ((size_t)b * L + qi) * W + h * 64 + 4 * fg;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {       // attn_store_row with the 1 / l factor, kept in place: see attn_store_row
            const f32x4 v = o[dt][qt] * inv;
            *reinterpret_cast<uint2*>(dst + dt * 16) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
        }
    }
}

}  // namespace clipmi
