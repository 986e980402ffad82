// gemm256.hpp — the large-shape NT GEMM: 256x256 block tile, 128 BYTES of K per row and K-tile (64 bf16 or 128 e4m3),
// 8 waves, LDS-DMA prefetch kept in flight ACROSS barriers (counted s_waitcnt vmcnt, raw s_barrier), four phases per
// K-tile and two wave groups running half a phase apart so that one group's MFMA cluster covers the other group's
// LDS reads and DMA issue (the "8-phase" structure of cdna_hip_programming.md §5, re-derived here).
//
// The schedule and the epilogue exist once, in g256_tile below; the bf16 kernel at the end of this file and the FP8
// kernel of gemm256f8.hpp expand it with an operand policy (G256Bf16 here, G256F8<MX, BSA> there).
//
// Same contract and epilogues as gemm.hpp (C[m][n] = sum_k A[m][k] W[n][k]); requires N % 256 == 0 and K a multiple
// of one K-tile, at least two of them (bf16: K % 64 == 0, K >= 128).
//
// LDS (128 KiB, one array): 2 K-tile buffers x [A-lo | A-hi | B-lo | B-hi], each half-tile = 128 rows x
// 128 B (16-B chunks XOR-swizzled with row & 7: on the DMA SOURCE address and on the read address; the DMA
// destination is lane-linear).
//
// Wave (wm, wn), wm in {0,1}, wn in {0..3}, owns output rows {wm*64..+63} of BOTH A halves and columns
// {wn*32..+31} of BOTH B halves, so the four phases of a K-tile touch the half-tiles in the order
//   P0: A-lo x B-lo   P1: A-lo x B-hi   P2: A-hi x B-hi   P3: A-hi x B-lo
// and each phase needs at most ONE half-tile that was not needed before. Phase p of K-tile t issues
// the DMA of half-tile [A-lo, B-lo, B-hi, A-hi][p] of K-tile t+1 into the other buffer: every half-tile
// has >= 3 phases between its issue and its first read (3 half-tiles = 6 DMA instructions per wave in
// flight).
//
// Ordering argument (slots = intervals between consecutive workgroup barriers; group 1 = waves with
// wm == 1 runs ONE slot behind group 0):
//   RAW  a half-tile is read only after (i) every wave has executed the counted vmcnt that retires ITS
//        two DMA instructions of that half-tile, placed at the end of the load slot of the phase
//        BEFORE the first read, and (ii) a barrier that follows the later group's wait. The reader's
//        load slot begins after exactly that barrier.
//   WAR  a buffer is re-filled for K-tile t+1 from slot 8t on; its last reads (K-tile t-1) complete by
//        slot 8t-2 (lgkmcnt(0) at the head of every MFMA slot).
// A policy's block-scale DMA (FP8 with block-scaled A) is issued BEFORE the prologue's: vmcnt retires in issue order,
// so the prologue's first counted wait covers it and no count below changes.
#pragma once
#include "gemm.hpp"

namespace clipmi {

constexpr int G256_HALF = 128 * 128;            // bytes per half-tile (128 rows x 128 B)
constexpr int G256_BUF = 4 * G256_HALF;         // 64 KiB per K-tile buffer
constexpr int G256_LDS = 2 * G256_BUF;          // 128 KiB

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// Operand policy of g256_tile, bf16 form. A policy names
//   F8, BSA        FP8 operands (accumulator scaling and the FP8-only store forms exist) / block-scaled A
//   ES             bytes per operand element: a K-tile is 128 / ES values of k
//   frag           the 16 bytes of a row that a lane reads from LDS
//   a_pitch        elements between rows of A (rows of W are K apart). K-tiles and LDS offsets are in bytes; a source
//                  address is formed in elements and scaled by ES once, as pointer arithmetic on the element type would:
//                  with the pitch itself in bytes the row product became a full 64-bit multiply (22 instructions per lane)
//   KSTEPS, mma    the MFMA slot body: step ks of an accumulator's K-tile from the two fragments of its W rows (b0, b1) and
//                  of its A rows (a0, a1); D = Wfrag x Afrag (C^T tile, see gemm.hpp). By VALUE: handing the fragment arrays
//                  to a function by reference cost 12 VGPRs in every instantiation and spills in the MX ones
//   scale_dma      (BSA) the block-scale slab's DMA behind the buffers; its read rides on the A-fragment read, sb -> mma
//   w_scale / a_scale / scaled   what the epilogue multiplies an accumulator with before the bias
//   store_row_mx / store_row_ln8   (F8) the two store forms that only the FP8 towers have
struct G256Bf16 {
    static constexpr bool F8 = false, BSA = false;
    static constexpr int ES = 2;
    typedef bf16x8 frag;
    static __device__ __forceinline__ size_t a_pitch(const GemmArgs& g) { return gemm_lda(g); }
    static constexpr int KSTEPS = 2;
    static __device__ __forceinline__ f32x4 mma(int ks, frag b0, frag b1, frag a0, frag a1, f32x4 c, int) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ks ? b1 : b0, ks ? a1 : a0, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 w_scale(const GemmArgs&, int) { return f32x4{1.f, 1.f, 1.f, 1.f}; }
    static __device__ __forceinline__ float a_scale(const GemmArgs&, int) { return 1.f; }
    static __device__ __forceinline__ f32x4 scaled(f32x4 c, f32x4, float) { return c; }
};

// One 256x256 output tile: K-loop and LDS-staged epilogue. P = operand policy (above; gemm256f8.hpp).
template <int EPI, class P>
__device__ __forceinline__ void g256_tile(const GemmArgs& g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef typename P::frag frag;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int fr = lane & 15, fg = lane >> 4;

    const int ntn = g.N >> 8;
    int bm, bn;
    gemm_tile_coords(blockIdx.x, gridDim.x, (g.M + 255) >> 8, ntn, 8, 4, bm, bn);
    const int m0 = bm << 8, n0 = bn << 8;
    const int K = g.K;

    // ---- DMA source pointers: half-tile rows [16*wave, 16*wave+16), two 8-row pieces per wave
    const int srow = lane >> 3, spos = lane & 7;
    const char* const Ab = reinterpret_cast<const char*>(g.A);
    const char* const Wb = reinterpret_cast<const char*>(g.W);
    const size_t pa = P::a_pitch(g);
    const char* src[4][2];                      // [A-lo, A-hi, B-lo, B-hi][piece]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wave * 16 + i * 8 + srow;
        const int chunk = (spos ^ (row & 7)) * (16 / P::ES);          // elements
        int ma = m0 + row, mb = m0 + 128 + row;
        ma = ma < g.M ? ma : g.M - 1;
        mb = mb < g.M ? mb : g.M - 1;
        src[0][i] = Ab + ((size_t)ma * pa + chunk) * P::ES;
        src[1][i] = Ab + ((size_t)mb * pa + chunk) * P::ES;
        src[2][i] = Wb + ((size_t)(n0 + row) * K + chunk) * P::ES;
        src[3][i] = Wb + ((size_t)(n0 + 128 + row) * K + chunk) * P::ES;
    }
    const int dma_off = wave * 16 * 128;
    // issue half-tile H (0..3 as in `src`) of K-tile kt into buffer `buf`
#define G256_ISSUE(H, kt, buf)                                                                                        \
    do {                                                                                                              \
        char* d_ = smem + (buf) * G256_BUF + (H) * G256_HALF + dma_off;                                               \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[H][0] + (kt) * 128),     \
                                         (__attribute__((address_space(3))) void*)(d_), 16, 0, 0);                    \
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[H][1] + (kt) * 128),     \
                                         (__attribute__((address_space(3))) void*)(d_ + 1024), 16, 0, 0);             \
    } while (0)

    // ---- fragment read offsets
    const int sw = fr & 7;
    const int c0 = ((0 + fg) ^ sw) * 16, c1 = ((4 + fg) ^ sw) * 16;
    const int offA = (wm * 64 + fr) * 128;                       // + half*16384 + mt*2048
    const int offB = 2 * G256_HALF + (wn * 32 + fr) * 128;       // + half*16384 + nt*2048

    f32x4 acc[2][4][2][2];     // [A half][mt][B half][nt]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[a][i][b][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // block-scaled A: the tile's scale bytes [256][K / 32] behind the K-tile buffers (rows past M: the array is padded to 256 rows)
    const int KB32 = K >> 5;
    const unsigned char* slab = reinterpret_cast<const unsigned char*>(smem) + G256_LDS;
    if constexpr (P::BSA) P::scale_dma(g, smem, m0, wave, lane);
    int sb[4] = {0x7f, 0x7f, 0x7f, 0x7f};      // e8m0 scale of this lane's (row, k-block) per mt of the current A half
    int kt_cur = 0;
    const int sb_off = (wm * 64 + fr) * KB32 + fg;

    frag af[4][2];             // current A half: [mt][16-byte fragment]
    frag bl[2][2], bh[2][2];   // B-lo / B-hi: [nt][16-byte fragment]

#define G256_READ_A(base, half)                                                                      \
    _Pragma("unroll") for (int t_ = 0; t_ < 4; ++t_) {                                               \
        af[t_][0] = *reinterpret_cast<const frag*>((base) + (half) * G256_HALF + offA + t_ * 2048 + c0); \
        af[t_][1] = *reinterpret_cast<const frag*>((base) + (half) * G256_HALF + offA + t_ * 2048 + c1); \
        if (P::BSA) sb[t_] = slab[sb_off + ((half) * 128 + t_ * 16) * KB32 + kt_cur * 4];           \
    }
#define G256_READ_B(dst, base, half)                                                                 \
    _Pragma("unroll") for (int t_ = 0; t_ < 2; ++t_) {                                               \
        dst[t_][0] = *reinterpret_cast<const frag*>((base) + (half) * G256_HALF + offB + t_ * 2048 + c0); \
        dst[t_][1] = *reinterpret_cast<const frag*>((base) + (half) * G256_HALF + offB + t_ * 2048 + c1); \
    }
    // MFMA slot of quadrant (A half a, B half b): the policy's MFMAs between the LDS wait and the slot's barrier (loop
    // order: k-step, A row tile, W row tile)
#define G256_MFMA(a, bfr, b)                                                                         \
    do {                                                                                             \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                           \
        __builtin_amdgcn_sched_barrier(0);                                                           \
        __builtin_amdgcn_s_setprio(1);                                                               \
        _Pragma("unroll") for (int ks_ = 0; ks_ < P::KSTEPS; ++ks_)                                  \
            _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                         \
                _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                     \
                    acc[a][i_][b][j_] = P::mma(ks_, bfr[j_][0], bfr[j_][1], af[i_][0], af[i_][1], acc[a][i_][b][j_], sb[i_]); \
        __builtin_amdgcn_s_setprio(0);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                           \
        __builtin_amdgcn_s_barrier();                                                                \
    } while (0)

    const int nk = (K * P::ES) >> 7;
    // ---- prologue: K-tile 0 into buffer 0, in the order of first use
    G256_ISSUE(0, 0, 0);
    G256_ISSUE(2, 0, 0);
    G256_ISSUE(3, 0, 0);
    G256_ISSUE(1, 0, 0);
    wait_vmcnt<4>();                         // A-lo(0), B-lo(0) landed (this wave's pieces)
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();     // group 1 runs one slot behind

    for (int t = 0; t < nk - 1; ++t) {
        const char* cur = smem + (t & 1) * G256_BUF;
        const int nb = (t + 1) & 1;
        kt_cur = t;
        // P0: A-lo x B-lo
        G256_READ_B(bl, cur, 0);
        __builtin_amdgcn_sched_barrier(0);
        G256_READ_A(cur, 0);
        G256_ISSUE(0, t + 1, nb);
        wait_vmcnt<4>();                     // retires B-hi(t)
        __builtin_amdgcn_s_barrier();
        G256_MFMA(0, bl, 0);
        // P1: A-lo x B-hi
        G256_READ_B(bh, cur, 1);
        G256_ISSUE(2, t + 1, nb);
        wait_vmcnt<4>();                     // retires A-hi(t)
        __builtin_amdgcn_s_barrier();
        G256_MFMA(0, bh, 1);
        // P2: A-hi x B-hi
        G256_READ_A(cur, 1);
        G256_ISSUE(3, t + 1, nb);
        __builtin_amdgcn_s_barrier();
        G256_MFMA(1, bh, 1);
        // P3: A-hi x B-lo (B-lo fragments still in registers)
        G256_ISSUE(1, t + 1, nb);
        wait_vmcnt<4>();                     // retires A-lo(t+1), B-lo(t+1)
        __builtin_amdgcn_s_barrier();
        G256_MFMA(1, bl, 0);
    }
    {   // last K-tile: nothing left to prefetch, the counts shrink
        const char* cur = smem + ((nk - 1) & 1) * G256_BUF;
        kt_cur = nk - 1;
        G256_READ_B(bl, cur, 0);
        __builtin_amdgcn_sched_barrier(0);
        G256_READ_A(cur, 0);
        wait_vmcnt<2>();                     // retires B-hi(last)
        __builtin_amdgcn_s_barrier();
        G256_MFMA(0, bl, 0);
        G256_READ_B(bh, cur, 1);
        wait_vmcnt<0>();                     // retires A-hi(last)
        __builtin_amdgcn_s_barrier();
        G256_MFMA(0, bh, 1);
        G256_READ_A(cur, 1);
        __builtin_amdgcn_s_barrier();
        G256_MFMA(1, bh, 1);
        __builtin_amdgcn_s_barrier();
        G256_MFMA(1, bl, 0);
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();     // balance the stagger: every wave has the same barrier count
#undef G256_ISSUE
#undef G256_READ_A
#undef G256_READ_B
#undef G256_MFMA

    // ---- epilogue, staged through LDS (the K-loop's buffers are dead after the last barrier above).
    // Fragment-shaped stores (16 rows x 32 B per wave-instruction, 32 instructions per lane) made the
    // tail store-ISSUE-bound: ~12 us per round of tiles, 29 us for the f32 read-modify-write (r01,
    // tools/gemm_overhead.py). Instead every lane drops its values (scales / bias / QuickGELU applied) into a
    // row-major LDS image of the tile — 16-byte chunks XOR-swizzled with row & 15 so that the 16 rows
    // of a fragment column do not share banks — and the tile leaves as whole rows, 16 B per lane,
    // 512 B..1 KiB contiguous per wave-instruction; the residual / positional add happens on that pass.
    f32x4 bz[2][2], ws[2][2], cs[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int n = n0 + b * 128 + wn * 32 + nt * 16 + 4 * fg;
            bz[b][nt] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            ws[b][nt] = P::w_scale(g, n);
            if (epi_is_ln(EPI)) cs[b][nt] = *reinterpret_cast<const f32x4*>(g.colsum + n);
        }
    float as[2][4];            // activation row scales of this lane's accumulator rows: [A half][mt]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            int m = m0 + a * 128 + wm * 64 + mt * 16 + fr;
            m = m < g.M ? m : g.M - 1;
            as[a][mt] = P::a_scale(g, m);
        }
#define G256_ACC(a, mt, b, nt) P::scaled(acc[a][mt][b][nt], ws[b][nt], as[a][mt])
    __syncthreads();
    if (epi_is_bf16_out(EPI)) {
        // image: 256 rows x 512 B
#pragma unroll
        for (int idx = 0; idx < 8; ++idx) {
            const int row = (idx >> 2) * 128 + wm * 64 + (idx & 3) * 16 + fr;
            // LN-folded consumer (gemm.hpp; FP8: A = e4m3(x) with MX block scales, W = e4m3(W diag(gamma)), the epilogue is
            // rstd (acc w_scale - mean colsum) + cb with colsum of the ROUNDED e4m3 weights, weights.py ln_fold_terms_fp8)
            f32x2 st = {0.f, 1.f};
            if (epi_is_ln(EPI)) {
                const int m = m0 + row;
                const int nseg = g.K >> 8;
                st = ln_row_stats(g.ln_part_in + (size_t)(m < g.M ? m : g.M - 1) * 2 * nseg, nseg, g.K);
            }
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    f32x4 v;
                    if (epi_is_ln(EPI)) v = ln_apply(G256_ACC(idx >> 2, idx & 3, b, nt), st.x, st.y, cs[b][nt], bz[b][nt]);
                    else v = G256_ACC(idx >> 2, idx & 3, b, nt) + bz[b][nt];
                    if (epi_is_qgelu(EPI)) {
                        v = quick_gelu4(v);
                    }
                    const int colbyte = (b * 128 + wn * 32 + nt * 16 + 4 * fg) * 2;
                    const int off = row * 512 + ((((colbyte >> 4) ^ (row & 15)) << 4) | (colbyte & 8));
                    *reinterpret_cast<uint2*>(smem + off) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
                }
        }
        __syncthreads();
        unsigned short* outp = static_cast<unsigned short*>(g.out);
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int row = wave * 32 + i * 2 + (lane >> 5);
            const int chunk = lane & 31;
            const uint4 v = *reinterpret_cast<const uint4*>(smem + row * 512 + ((chunk ^ (row & 15)) << 4));
            const int m = m0 + row;
            bool left = false;             // FP8 QuickGELU forms: the policy stores the row when g.out_bscale asks for e4m3
            if constexpr (P::F8 && epi_is_qgelu(EPI)) left = P::store_row_mx(g, v, m, n0 + chunk * 8, lane);
            if (!left && m < g.M) *reinterpret_cast<uint4*>(outp + (size_t)m * g.N + n0 + chunk * 8) = v;
        }
    } else {
        // two passes of 128 rows x 1 KiB (f32)
        float* outp = static_cast<float*>(g.out);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (a) __syncthreads();
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = wm * 64 + mt * 16 + fr;
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const f32x4 v = G256_ACC(a, mt, b, nt) + bz[b][nt];
                        const int chunk = (b * 128 + wn * 32 + nt * 16 + 4 * fg) >> 2;
                        *reinterpret_cast<f32x4*>(smem + row * 1024 + ((chunk ^ (row & 15)) << 4)) = v;
                    }
            }
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const int row = wave * 16 + i;
                f32x4 v = *reinterpret_cast<const f32x4*>(smem + row * 1024 + ((lane ^ (row & 15)) << 4));
                const int m = m0 + a * 128 + row;
                if (m < g.M) {
                    size_t orow = (size_t)m;
                    if (EPI == EPI_PATCH_F32) {
                        const int b_ = m / g.np, p_ = m - b_ * g.np;
                        orow = (size_t)b_ * g.L + 1 + p_;
                        v += *reinterpret_cast<const f32x4*>(g.pos + (size_t)(1 + p_) * g.N + n0 + lane * 4);
                    }
                    float* dst = outp + orow * g.N + n0 + lane * 4;
                    if (EPI == EPI_BIAS_RESID_F32 || EPI == EPI_BIAS_RESID_LN8) v += *reinterpret_cast<const f32x4*>(dst);
                    *reinterpret_cast<f32x4*>(dst) = v;
                }
                if constexpr (P::F8 && EPI == EPI_BIAS_RESID_LN8) P::store_row_ln8(g, v, m, n0, lane);
            }
        }
    }
#undef G256_ACC
}

template <int EPI>
__global__ void __launch_bounds__(512, 2) gemm256_bf16_nt_kernel(GemmArgs g) {
    g256_tile<EPI, G256Bf16>(g);
}

}  // namespace clipmi
