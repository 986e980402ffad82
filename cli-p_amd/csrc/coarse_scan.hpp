// coarse_scan.hpp — the coarse half of the coarse-then-exact search (gfx950): the superset argument, coarse_prep_kernel and
// the three scans of a coarse copy - scan_coarse_kernel (<= 64 queries), scan_coarse_wide_kernel, scan_coarse_wide2_kernel
// (int8 copy, up to 1 024 queries) - with the pieces they share: pair_slot, pairs_flush, pairs_publish, i8_pretest_dmin, max16,
// wide_tile_map, i8_block_rsrc. Included by topk.hip only, behind its f32x4, wave_lds_sync and CLIPMI_NT_MASK.
#pragma once
#include "i8_layout.hpp"

namespace clipmi {
namespace {

// =================================================================================================
// Coarse-then-exact path (SURVEY.md §7 option (b)): a bf16 copy of the matrix is scanned with bf16
// MFMA (half the HBM bytes, 64 queries per pass) keeping a PROVABLE SUPERSET of the exact top-K; the
// survivors are re-scored in exact f32 with the same fmaf order as the exact kernel and selected by the
// same radix select, so results stay bit-exact against the oracle.
//
// Superset argument. Let s(r) be the exact (fmaf-chain) score of row r and c(r) the bf16-MFMA score of
// the bf16-rounded operands. bf16 keeps 8 significant bits, so RNE has relative error u8 = 2^-8 per operand and the
// exact products differ by at most (2 u8 + u8^2)|a_k b_k| = 0.0078278 |a_k b_k| (reached: both mantissas just under a
// rounding tie, 1 + (1 - d) 2^-8, in every component); both accumulations (f32, E terms, any order) add at most
// ~2 * E * 2^-24 * sum|a_k b_k|. With sum|a_k b_k| <= ||row|| ||q||, at E = 512:
//        |c(r) - s(r)| <= 0.0078888 * ||row|| * ||q||  <=  margin_q := 0.0080 * R_max * ||q||
// (R_max = largest row norm, kept with the bf16 copy). E = 768: 0.0079193 and 0.0080305, bf16_margin_coef<E> below;
// tests/coarse_tight.py family B presses this bound. tau0_q = exact K-th best of the first S rows is
// a lower bound of the final K-th best score; every row of the true top-K has s >= tau0_q, hence
// c >= tau0_q - margin_q =: the coarse threshold. If a candidate list overflows its capacity a device
// flag makes the (otherwise early-exiting) exact-scan fallback launches run and overwrite the result.
// =================================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- int8 coarse copy (clipmi_quantize_rows_i8 / clipmi_topk_ip_coarse_i8) -------------------------------
// Row r: s_r = (max |x| over r's 32-row block) / 127, q_rk = rint(x_rk / s_r) in [-127, 127], a_r = 1.001 * ||x_r - s_r q_r||_2.
// Query: t_q, p_qk the same way, f_q = y - t_q p_q. The int8 MFMA gives the EXACT integer D = q_r . p_q
// (|D| <= E * 127^2 < 2^24 for E <= 768), and
//      x.y = s_r t_q D + e_r.y + (s_r q_r).f_q      =>      |x.y - s_r t_q D| <= a_r ||y|| + (R_max + A_max) ||f_q||
// (Cauchy-Schwarz twice; ||s_r q_r|| <= ||x_r|| + a_r). A row can be in the exact top-K only if its exact score is
// >= tau_q (the exact K-th best of a sample), so the scan keeps row r for query q when
//      s_r t_q D + a_r * 1.001 ||y|| >= tau_q - 1.001 (R_max + A_max) ||f_q|| - c(E) R_max ||y||,   c(512) = 1e-4
// (the last term covers f32 rounding of both sides and of the exact kernel's fmaf chain: < E * 2^-23 relative;
//  c(E) = 1e-4 E / 512, derived at i8_round_slack<E> below).
// Divided by t_q > 0 so that the kernel's test is one convert + one multiply + one fma + one compare per pair.
// (A second int8 digit of the query - y = t p + u p' + f', a second MFMA chain per row tile - removes the query half of
//  the margin and was measured: 45 % fewer rows reach the exact re-scoring pass (-30 us per 64 queries at 10 M rows), but
//  with 128 MFMAs per 32-row step the one wave per SIMD is MFMA/VALU-bound in the early segments: scans +75 us. Rejected.)
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Per-query constants of a coarse search, once per group of <= qs queries (one wave per query), qmeta [4][qs]
// (qs = 64 for the 64-query passes, the padded query count of a wide pass):
//   [0]    1 / t_q (int8; t_q = max|y| / 127)            or 1 (bf16)
//   [qs]   1.001 ||y|| / t_q (int8)                       or 0
//   [2 qs] the value the scan compares against, (tau - margin) * [0] - written by select_topk_kernel each time a new exact
//          K-th best tau is known (-inf until then)
//   [3 qs] margin: 1.001 (R_max + A_max) ||f_q|| + 1e-4 R_max ||y|| (int8, f_q = y - t_q p_q) or 1.001 * bf16_margin_coef<E> R_max ||q||
//         (bf16); +inf when it is not a number (the threshold then stays -inf: everything survives, the result stays exact)
// and the query image the scan kernels copy into LDS (entry [(qg*KS + s)*64 + lane] = 16 bytes of query 16 qg + (lane & 15):
// bf16 k = 32 s + 8 g .. + 7, or int8 k = 64 s + 16 g .. + 15, g = lane >> 4; zero for queries >= QA). Block 0 also clears
// the call's control words (candidate counters, overflow flag): no memset node.
// Rounding slack of the two superset bounds as a function of the row width (derivations: DESIGN.md 4.1l, summary here).
// int8: the test compares f32 evaluations of both sides of
//      s_r t_q D + a_r 1.001 ||y||  >=  tau_q - 1.001 (R_max + A_max) ||f_q||,
// and tau_q and the row's own exact score come from fmaf chains of E terms. What rounding can move, relative to R_max ||y||:
//   * the row's exact score against its real inner product: gamma_E = E u / (1 - E u), u = 2^-24 (one rounding per fmaf);
//     tau_q itself is COMPARED as computed, not trusted as real, but the budget of round 2 charges a second chain for it;
//   * the integer D is exact (|D| <= E 127^2 <= 12 387 072 < 2^24 for E <= 768), so the left side has three roundings
//     (convert - exact -, multiply inside the fma, the product a_r * yt, the fma) and the right side three (subtract,
//     multiply by 1/t_q, the margin's own sum), each of a quantity <= 1.35 R_max ||y|| / t_q (A_max <= 0.11 R_max and
//     ||f_q|| <= 0.11 ||y|| at E <= 768: half a step times sqrt(E) against a largest component of 127 steps): < 16 u in all;
//   * the norms ||y||, ||f_q||, a_r are upper bounds by themselves (f64 sums of squares, roots rounded up: norm_up); their
//     1.001 factors stay (they were sized for f32 sums: 1e-3 against < 2.3e-5) and the budget does not lean on them.
//   All of this is relative. Where a rounding is absolute - the subnormal grid - or a side can overflow, coarse_prep_kernel
//   sets the margin to +inf instead (I8_TINY .. COARSE_HUGE_RY in i8_layout.hpp).
// Needed: (2 E + 16) u = 6.2e-5 at E = 512, 9.3e-5 at E = 768. The constant is 1e-4 * E / 512: 1e-4 at 512 (unchanged, bit for
// bit), 1.5e-4 at 768 - the same 1.6 x head room at both widths instead of 1.08 x; it is < 1 % of the query half of the margin
// (1.001 (R + A) ||f_q|| ~ 7.6e-3 R ||y|| on unit data), so the survivor count does not notice.
// bf16: |c - s| <= (2 u8 + u8^2 + 2 E u) ||x|| ||y||, u8 = 2^-8 (8 significant bits: half an ulp of a mantissa in [1, 2) is
// 2^-8): 0.0078888 at 512, 0.0079193 at 768. The constant is 0.0080 + 2 (E - 512) u: 0.0080 at 512, 0.0080305 at 768 - the same
// 1.1e-4 of head room at both widths (the kernel multiplies by 1.001 once more for the f32 norms).
template <int E>
constexpr float i8_round_slack() { return 1e-4f * ((float)E / 512.0f); }
template <int E>
constexpr float bf16_margin_coef() { return 0.0080f + 2.0f * (float)(E - 512) * 5.9604644775390625e-8f; }
static_assert(i8_round_slack<512>() == 1e-4f && bf16_margin_coef<512>() == 0.0080f, "the constants at E = 512: 1e-4 (int8 slack), 0.0080 (bf16 margin)");
template <int E>
constexpr bool bf16_coef_covers() { return (double)bf16_margin_coef<E>() > 2.0 / 256 + 1.0 / 65536 + 2.0 * E / 16777216; }
static_assert(bf16_coef_covers<512>() && bf16_coef_covers<768>(), "the bf16 margin must cover 2 u8 + u8^2 + 2 E 2^-24, u8 = 2^-8");
static_assert(768 * 127 * 127 < (1 << 24), "the int8 dot product must stay exact in f32");

template <bool I8, int ET = 512>
__global__ void __launch_bounds__(256) coarse_prep_kernel(const float* __restrict__ q, int E, float rmax, float amax, int QA,
                                                          float* qmeta, uint4* qimage, unsigned* ctl, int nctl, int qs,
                                                          int wide = 0) {
    constexpr int KS = ET / (I8 ? 64 : 32);         // k-steps of the 64-query image; E == ET
    constexpr int KSW = ET / 32;                    // k-steps of the wide image: 16 at 512, 24 at 768 (2 KSW <= 64 lanes write it)
    const int lane = threadIdx.x & 63;
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < nctl; i += 256) ctl[i] = 0u;
    const int qg = qi >> 4, col = qi & 15;
    // wide pass (int8): the B operand of v_mfma_i32_32x32x32_i8 - 32-query groups, KSW k-steps of 32 bytes, entry
    // [(G*KSW + s)*64 + h*32 + n] = bytes 32 s + 16 h .. + 15 of query 32 G + n (lanes 0 .. 2 KSW - 1 hold (s, h) = (lane >> 1, lane & 1))
    const int widx = ((qi >> 5) * KSW + (lane >> 1)) * 64 + (lane & 1) * 32 + (qi & 31);
    if (qi >= QA) {                                            // padding query of a used query group: zero image
        if (wide) { if (lane < 2 * KSW) qimage[widx] = make_uint4(0u, 0u, 0u, 0u); }
        else
            // KS * 4 entries per query: 32 (int8) or 64 (bf16) at E = 512 - one round of the wave -, 48 or 96 at E = 768
            for (int e = lane; e < KS * 4; e += 64) qimage[(qg * KS + (e >> 2)) * 64 + (e & 3) * 16 + col] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    const float* y = q + (size_t)qi * E;
    // ||y|| and ||f_q||: f64 sums of squares, roots rounded up (norm_up) - upper bounds at any magnitude of the query
    float mx = 0.f;
    double ss = 0.0;
    for (int k = lane; k < E; k += 64) { const float v = y[k]; mx = fmaxf(mx, fabsf(v)); ss = fma((double)v, (double)v, ss); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); ss += __shfl_xor(ss, o); }
    const float t = mx > 0.f ? mx / 127.0f : 1.0f;
    const float inv = I8 ? 1.0f / t : 1.0f;
    // the int8 digit of component v; the query images below use the same expression
    auto digit = [&](float v) -> float { return fminf(fmaxf(rintf(v * inv), -127.f), 127.f); };
    double ff = 0.0;
    if (I8) {
        for (int k = lane; k < E; k += 64) {
            const double f = fma(-(double)t, (double)digit(y[k]), (double)y[k]);       // what the digit leaves: f_q (exact in f64)
            ff = fma(f, f, ff);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ff += __shfl_xor(ff, o);
    }
    if (lane == 0) {
        const float Y = norm_up(ss), F = norm_up(ff) * 1.001f;
        float margin = I8 ? 1.001f * (rmax + amax) * F + i8_round_slack<ET>() * rmax * Y : bf16_margin_coef<ET>() * rmax * Y * 1.001f;
        // A query with a NaN or infinite component has no usable coarse bound: its margin is +inf, which the selects turn into a
        // threshold of -inf whatever the K-th best is (inf - inf would be a NaN that passes nothing) - every row then passes, the
        // lists overflow and the exact fallback answers the call, as the contract promises for any data. The other two
        // constants stay finite so that the scans' left-hand sides do (round 5: an infinite component used to give inv = 0 and
        // Y inv = NaN, and such a query came back empty - test_non_finite_queries_through_the_permuted_int8_copy).
        // The same holds where the f32 arithmetic of the bound is not proved (i8_layout.hpp, I8_TINY ..): a query or a database
        // so small that 1 / t_q overflows or that roundings on the subnormal grid (absolute, E half-steps of 2^-149 in a score)
        // outgrow the relative slack, or so large that a score or a scaled side can overflow. R_max ||y|| bounds every score
        // and every partial sum of its fmaf chain.
        constexpr float TINY = I8 ? I8_TINY : BF16_TINY;
        const float RY = rmax * Y;
        const bool in_range = mx >= TINY && mx <= COARSE_HUGE && rmax >= TINY && rmax <= COARSE_HUGE && RY >= TINY && RY <= COARSE_HUGE_RY;
        const bool finite_q = in_range && fabsf(Y) < INFINITY && fabsf(mx) < INFINITY && fabsf(margin) < INFINITY;      // false for NaN too
        if (!finite_q) margin = INFINITY;
        qmeta[qi] = finite_q ? inv : 1.0f;
        qmeta[qs + qi] = I8 && finite_q ? 1.001f * Y * inv : 0.f;
        qmeta[2 * qs + qi] = -INFINITY;
        qmeta[3 * qs + qi] = margin;
    }
    if (I8 && wide) {
        if (lane < 2 * KSW) {
            const float* p = y + 32 * (lane >> 1) + 16 * (lane & 1);
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned pk = 0;
#pragma unroll
                for (int b_ = 0; b_ < 4; ++b_) {
                    pk |= ((unsigned)(int)digit(p[4 * j + b_]) & 0xffu) << (8 * b_);
                }
                w[j] = pk;
            }
            qimage[widx] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        return;
    }
    for (int e = lane; e < KS * 4; e += 64) {          // one round at E = 512; 96 bf16 entries per query at E = 768 take two
        const int s_ = e >> 2, g_ = e & 3;
        uint4 v;
        if (I8) {
            const float* p = y + 64 * s_ + 16 * g_;
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned pk = 0;
#pragma unroll
                for (int b_ = 0; b_ < 4; ++b_) pk |= ((unsigned)(int)digit(p[4 * j + b_]) & 0xffu) << (8 * b_);
                w[j] = pk;
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            const float* p = y + 32 * s_ + 8 * g_;
            v = make_uint4(pack2_bf16(p[0], p[1]), pack2_bf16(p[2], p[3]), pack2_bf16(p[4], p[5]), pack2_bf16(p[6], p[7]));
        }
        qimage[(qg * KS + s_) * 64 + g_ * 16 + col] = v;
    }
}

// A coarse scan appends (CAND_SLOT, slot of the copy); the re-scoring pass turns such an entry into (exact score bits, row id).
// No score has these bits (a NaN score is stored as -inf), so an entry that was re-scored before - the K best a select keeps at
// the head of the list - is recognised and keeps its row id.
// INVARIANT: every writer of cand[].x - sample_scores_kernel, rescore_pairs_kernel, rescore_pairs16_kernel and the
// heads select_topk_kernel keeps (it copies .x unchanged) - stores either CAND_SLOT with a slot, or the RAW bits of a score that is
// not a NaN (NaN -> -inf before the store). Never an order-preserving key of one, never raw bits of an unchecked score: 0xffffffff is a NaN
// pattern and would be read as "slot". tests/test_topk_gpu.py::test_non_finite_queries_through_the_permuted_int8_copy holds it.
constexpr unsigned CAND_SLOT = 0xffffffffu;

// ---- the per-wave pending (query, row) list: what the three scans share ------------------------------------------------------
// Entries (query relative to the workgroup's first, slot of the copy), `npend` of them pending (wave-uniform, no LDS atomics):
// the lanes of a ballot append side by side. Past a kernel's flush mark the wave publishes them itself (pairs_flush), the rest
// goes out per workgroup at the end (pairs_publish); both bound-check the global lists, and a miss arms the exact fallback.
// this lane's position for ballot m of appending lanes behind npend pending entries; the caller then adds popcount(m)
__device__ __forceinline__ int pair_slot(unsigned long long m, int npend) {
    return npend + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// publish a wave's n pending pairs: one global atomic per pair (rare path: ~1 pair in 10^4 passes the threshold)
__device__ __noinline__ void pairs_flush(const uint2* list, int n, int qbase, unsigned* gcnt, uint2* cand, long long cap,
                                         unsigned* overflow) {
    const int lane = threadIdx.x & 63;
    wave_lds_sync();
    for (int e = lane; e < n; e += 64) {
        const uint2 c = list[e];
        const unsigned q = (unsigned)qbase + c.x;
        const unsigned pos = atomicAdd(&gcnt[q], 1u);
        if ((long long)pos < cap) cand[(size_t)q * cap + pos] = make_uint2(CAND_SLOT, c.y);
        else *overflow = 1u;
    }
    wave_lds_sync();
}

// Final publication, aggregated per WORKGROUP: an LDS histogram of the waves' pending pairs over the workgroup's QMAX queries,
// one returning global atomic per (workgroup, query) issued by all lanes at once, then the entries scatter to base + an
// LDS-counted offset. (Per-entry global atomics here meant ~166 k same-address atomics at the end of every scan: ~250 us
// fixed, as much as streaming 1.25 M rows.) smem: 3 QMAX words at the head of the LDS, dead by now (image or ring). Workgroup
// barriers inside: every one of the workgroup's THREADS threads calls this, with its own wave's list and npend.
template <int QMAX, int THREADS>
__device__ __forceinline__ void pairs_publish(char* smem, const uint2* list, int npend, int qbase, unsigned* gcnt, uint2* cand,
                                              long long cap, unsigned* overflow) {
    const int tid = threadIdx.x, lane = tid & 63;
    __syncthreads();
    unsigned* hist = reinterpret_cast<unsigned*>(smem);              // [QMAX] counts
    unsigned* gbase = hist + QMAX;                                   // global base per query
    unsigned* hoff = hist + 2 * QMAX;                                // running offsets
    for (int i = tid; i < QMAX; i += THREADS) { hist[i] = 0; hoff[i] = 0; }
    __syncthreads();
    for (int e = lane; e < npend; e += 64) atomicAdd(&hist[list[e].x], 1u);
    __syncthreads();
    for (int i = tid; i < QMAX; i += THREADS) gbase[i] = hist[i] ? atomicAdd(&gcnt[qbase + i], hist[i]) : 0u;
    __syncthreads();
    for (int e = lane; e < npend; e += 64) {
        const uint2 c = list[e];
        const unsigned pos = gbase[c.x] + atomicAdd(&hoff[c.x], 1u);
        if ((long long)pos < cap) cand[(size_t)(qbase + c.x) * cap + pos] = make_uint2(CAND_SLOT, c.y);
        else *overflow = 1u;
    }
}

struct CoarseArgs {
    const void* dbc;             // coarse copy of the matrix: bf16 [nrows][E] or int8 [nrows][E]
    const float2* rmeta;         // int8 only: per row (scale s_r, error norm a_r >= ||x_r - s_r q_r||), padded to 32 rows
    const float* qmeta;          // [4][64], see coarse_prep_kernel: 1/t_q | 1.001 ||y|| / t_q | scaled threshold | margin
    const uint4* qimage;         // the query image in the scan's LDS layout (coarse_prep_kernel)
    long long row0;              // this launch scans rows [row0, row0 + nrows) of the copy; row0 % 32 == 0 (ids stay global)
    long long nrows;
    const float* q;              // f32 [QA][E]
    int QA;                      // 1..16*QG
    const float* tauc;           // [QA]
    uint2* cand;                 // [QA][cap]: .y = row id (.x filled by the re-scoring pass)
    unsigned* gcnt;              // [128]
    long long cap;
    unsigned* overflow;          // set to 1 when a list would exceed cap
    int abl;                     // development ablation (CLIPMI_COARSE_ABL=1): never append - timing only, results wrong
};

// Per-wave (query, row) list in LDS. One (row tile, query group) block of a step appends at most 4 rows x 64 lanes =
// 256 pairs and the flush test runs after every such block, so the list holds COARSE_FLUSH + 256 entries: it cannot
// overrun by construction (and the append is bound-checked all the same: a miss arms the exact fallback). 6 KiB per
// wave keeps a 64-query int8 scan workgroup at 56 KiB of LDS, so the small kernels of ANOTHER batch in flight (exact
// re-scoring 72 KiB, selects, the sample scan 64 KiB) fit on the same CU instead of waiting for the scan to drain.
constexpr int COARSE_QS = 64;           // qmeta stride of the 64-query passes
constexpr int COARSE_FLUSH = 512;       // flush when more than this many are pending
constexpr int COARSE_LIST = COARSE_FLUSH + 256;
constexpr size_t COARSE_WAVE_BYTES = (size_t)COARSE_LIST * 8 + 16;

// 16 bytes of the streamed coarse copy (CLIPMI_NT_MASK bit 0: non-temporal)
__device__ __forceinline__ uint4 ld_stream(const char* p) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    if constexpr (CLIPMI_NT_MASK & 1) {
        const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
        return make_uint4(v[0], v[1], v[2], v[3]);
    } else
        return *reinterpret_cast<const uint4*>(p);
}

// PREPASS only changes the kernel's NAME (the level-2 pre-pass over S2 rows must not dilute the profiler's
// per-name average of the main scan).
template <int E, int QG, bool PREPASS, bool I8>
__global__ void __launch_bounds__(256) scan_coarse_kernel(CoarseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = E / (I8 ? 64 : 32);   // MFMA k-steps per 16-row tile (16 bytes per lane and step either way)
    constexpr int ROWB = I8 ? E : 2 * E;     // bytes per row of the coarse copy
    constexpr int SLOTS = 2 * KS;       // one step = two row tiles (32 rows): SLOTS 16-byte fragments per lane
    constexpr int NIMG = QG * KS * 64;                  // 16-byte entries of the query image
    constexpr int IMG_BYTES = NIMG * 16;
    static_assert(COARSE_LIST >= COARSE_FLUSH + 4 * 64, "a block's appends must fit behind a pending flush");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = blockDim.x >> 6;
    const int col = lane & 15, g = lane >> 4;

    // query image: built once per search by coarse_prep_kernel (each of 256 workgroups x 3 launches used to read the 128 KiB
    // of f32 queries and quantise them again); here it is a 16-byte-per-lane copy, 8 loads in flight (written out here and in
    // scan_coarse_wide_kernel: as a shared function it moved this kernel's SGPR spills into the per-step path)
    uint4* qimg = reinterpret_cast<uint4*>(smem);
    {
        static_assert(NIMG % 256 == 0, "image copy loop: whole 256-entry rows, every one bounded by NIMG below");
        for (int base = tid; base < NIMG; base += 8 * 256) {
            uint4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = base + j * 256 < NIMG ? a.qimage[base + j * 256] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (base + j * 256 < NIMG) qimg[base + j * 256] = v[j];
        }
    }
    uint2* list = reinterpret_cast<uint2*>(smem + IMG_BYTES + (size_t)wave * COARSE_WAVE_BYTES);
    int npend = 0;                                     // wave-uniform: pairs pending in `list` (positions by ballot prefix)
    __syncthreads();

    bool active[QG];
    float tau[QG], yt[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        active[qg] = qg * 16 + col < a.QA;
        tau[qg] = active[qg] ? a.qmeta[2 * COARSE_QS + qg * 16 + col] : INFINITY;
        yt[qg] = (I8 && active[qg]) ? a.qmeta[COARSE_QS + qg * 16 + col] : 0.f;
    }

    // steps are counted from row 0 of the copy (row0 % 32 == 0), so row = 32 step + ... is the global row id
    const long long step0 = a.row0 >> 5;
    const long long nsteps = step0 + ((a.nrows + 31) >> 5);
    const long long wg = (long long)blockIdx.x * nwaves + wave;
    const long long tw = (long long)gridDim.x * nwaves;
    const long long last_row = a.row0 + a.nrows - 1;

    long long step = step0 + wg;
    if (step < nsteps) {
        uint4 T[SLOTS];
        // bf16 copy: row-major, 64 bytes per row and k-step; int8 copy: 32-row blocks of [16 k-steps of 32 B][64 lanes][16 B]
        // (quantize_rows_i8_kernel), padded to whole blocks: this lane's 16 bytes of MFMA k-step s are bytes 64 s + 16 g
        // of row 16 rt + col = 32-byte k-step 2 s + (g >> 1), half g & 1
        constexpr int KSTRIDE = I8 ? 2048 : 64;
        auto frag_ptr = [&](long long st, int rt) {
            if (I8)
                return static_cast<const char*>(a.dbc) + st * (32 * ROWB) + (g >> 1) * 1024 + ((g & 1) * 32 + rt * 16 + col) * 16;
            long long r = st * 32 + rt * 16 + col;
            r = r > last_row ? last_row : r;
            return static_cast<const char*>(a.dbc) + r * ROWB + 16 * g;
        };
        // int8: (s_r, a_r) of this lane's accumulator rows 4g .. 4g+3 of both row tiles (rmeta is padded to 32 rows)
        uint4 M[4] = {};
        auto load_meta = [&](long long st, uint4* m) {
            if (I8) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    const uint4* mp = reinterpret_cast<const uint4*>(a.rmeta + st * 32 + rt * 16 + 4 * g);
                    m[2 * rt] = mp[0];
                    m[2 * rt + 1] = mp[1];
                }
            }
        };
        {
            const char* p0 = frag_ptr(step, 0);
            const char* p1 = frag_ptr(step, 1);
#pragma unroll
            for (int s_ = 0; s_ < KS; ++s_) {
                T[s_] = ld_stream(p0 + KSTRIDE * s_);
                T[KS + s_] = ld_stream(p1 + KSTRIDE * s_);
            }
            load_meta(step, M);
        }
        using AccT = typename std::conditional<I8, i32x4, f32x4>::type;
        while (true) {
            const long long nxt = step + tw;
            const bool has_next = nxt < nsteps;
            const char* pn[2] = {frag_ptr(has_next ? nxt : step, 0), frag_ptr(has_next ? nxt : step, 1)};
            uint4 MN[4] = {};
            load_meta(has_next ? nxt : step, MN);

            AccT acc[2][QG];                            // [rt][qg]
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) acc[rt][qg] = AccT{0, 0, 0, 0};
            // One slot at a time: the LDS reads of the NEXT slot's query fragments, this slot's MFMAs, then the refill of
            // this slot's register with the next step's fragment. A load can only be issued once the MFMAs reading its
            // register have been, and its data is needed one step later, so a step lasts (HBM latency + the MFMA time
            // between two refills): refilling after every slot instead of every 8 (the first version) keeps that second
            // term at QG MFMAs - main scan 629-648 -> 619 us at 10 M rows. The sched_group_barriers state the order; no
            // fake dependency on the accumulators is needed.
            uint4 B[2][QG];
            auto load_b = [&](int s_, uint4* b) {
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) b[qg] = qimg[(qg * KS + s_) * 64 + lane];
            };
            __builtin_amdgcn_sched_barrier(0);
            load_b(0, B[0]);
#pragma unroll
            for (int slot = 0; slot < SLOTS; ++slot) {
                const int rt = slot / KS;
                // the second row tile re-reads the fragments from LDS (left to itself the compiler keeps all of the first
                // tile's in registers: up to 128 more VGPRs, and no other kernel's wave fits on the SIMD any more)
                if (slot + 1 == KS) asm volatile("" ::: "memory");
                if (slot + 1 < SLOTS) load_b((slot + 1) % KS, B[(slot + 1) & 1]);
                const uint4* b = B[slot & 1];
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) {
                    if constexpr (I8)
                        acc[rt][qg] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, T[slot]),
                                                                            __builtin_bit_cast(i32x4, b[qg]), acc[rt][qg], 0, 0, 0);
                    else
                        acc[rt][qg] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, T[slot]),
                                                                              __builtin_bit_cast(bf16x8, b[qg]), acc[rt][qg], 0, 0, 0);
                }
                T[slot] = ld_stream(pn[rt] + KSTRIDE * (slot % KS));
            }
            __builtin_amdgcn_sched_group_barrier(0x100, QG, 0);                // slot 0's fragments
#pragma unroll
            for (int slot = 0; slot < SLOTS; ++slot) {
                if (slot + 1 < SLOTS) __builtin_amdgcn_sched_group_barrier(0x100, QG, 0);    // DS reads: next slot's fragments
                __builtin_amdgcn_sched_group_barrier(0x008, QG, 0);                          // MFMAs of this slot
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                           // VMEM read: the refill
            }
            __builtin_amdgcn_sched_barrier(0);

            // value compared with tau[qg]: the bf16 score itself, or (int8) D * s_r + a_r * 1.001 ||y|| / t_q
            float val[2][QG][4];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const float sr[4] = {__uint_as_float(M[2 * rt].x), __uint_as_float(M[2 * rt].z), __uint_as_float(M[2 * rt + 1].x),
                                     __uint_as_float(M[2 * rt + 1].z)};
                const float ar[4] = {__uint_as_float(M[2 * rt].y), __uint_as_float(M[2 * rt].w), __uint_as_float(M[2 * rt + 1].y),
                                     __uint_as_float(M[2 * rt + 1].w)};
#pragma unroll
                for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float d = (float)acc[rt][qg][r];
                        val[rt][qg][r] = I8 ? fmaf(d, sr[r], ar[r] * yt[qg]) : d;
                    }
            }
            bool any = false;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        any |= active[qg] && (step * 32 + rt * 16 + 4 * g + r <= last_row) && (val[rt][qg][r] >= tau[qg]);
            // Appends (round 4): positions by ballot prefix into a wave-uniform count, as the wide passes do. The first form took one
            // returning LDS atomic per pair and, per (row tile, query group) block, a wave-level LDS sync + a read of the counter for
            // the flush test - eight of each on ~60 % of the steps at 64 queries. With all appends compiled out (CLIPMI_COARSE_ABL=1)
            // the scan is 10-45 us of 0.8 ms faster: that is what any append path can still gain. Blocks without a hit cost one ballot.
            if (__ballot(any) && !a.abl) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) {
                        bool p[4], anyb = false;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            p[r] = active[qg] && (step * 32 + rt * 16 + 4 * g + r <= last_row) && (val[rt][qg][r] >= tau[qg]);
                            anyb |= p[r];
                        }
                        if (!__ballot(anyb)) continue;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const unsigned long long m = __ballot(p[r]);
                            if (m) {
                                const int pos = pair_slot(m, npend);
                                // <= 256 appends per block behind at most COARSE_FLUSH pending: inside the list (static_assert above)
                                if (p[r]) list[pos] = make_uint2((unsigned)(qg * 16 + col), (unsigned)(step * 32 + rt * 16 + 4 * g + r));
                                npend += __builtin_popcountll(m);
                            }
                        }
                        if (npend > COARSE_FLUSH) {
                            pairs_flush(list, npend, 0, a.gcnt, a.cand, a.cap, a.overflow);
                            npend = 0;
                        }
                    }
            }
            if (!has_next) break;
            step = nxt;
#pragma unroll
            for (int i = 0; i < 4; ++i) M[i] = MN[i];
        }
    }
    pairs_publish<16 * QG, 256>(smem, list, npend, 0, a.gcnt, a.cand, a.cap, a.overflow);      // the query image is dead now
}

// =================================================================================================
// Wide coarse pass (int8 copy only): ONE stream of the copy for up to WIDE_MAX_Q = 1024 queries of one search call
// (reference: query-index.py:111 is one index.search call; SURVEY.md §8d "DB streamed once per batch").
//
// The 64-query pass above is HBM-bound with the matrix cores 17 % busy; a search of Q >> 64 queries as Q / 64 such
// passes streams the copy Q / 64 times. Here the queries are cut into tiles of <= 256 (a 128-KiB int8 image in LDS)
// and every workgroup keeps ONE tile resident for the whole launch. Workgroups with the same `row lane` and different
// tiles walk the same rows of the copy in the same order; they sit on one XCD (blockIdx % 8 labels the XCD's share of
// the grid - speed only), so the copy crosses HBM about once per launch and the other tiles' reads are L2 / Infinity
// Cache hits. Per 32-row step a wave holds the rows' fragments in registers (16 KiB) and walks the tile's 64-query sets:
// per set and k-step 4 query fragments from LDS feed 8 MFMAs (both 16-row tiles: half an LDS read per MFMA, so the LDS
// pipe is at 50 % when the matrix pipe is full); the fragments' registers are refilled with the next step's rows during
// the LAST set. Two waves per SIMD (512 threads): one wave's compare epilogue and its wait for the next rows run under
// the other's MFMAs. The pass is matrix-bound: 2 N Q 512 int8 operations per launch.
// Survivors go to the same per-query lists as the 64-query pass's (entries appended by ballot prefix, no LDS atomics).
// =================================================================================================
constexpr int WIDE_MAX_Q = 1024;                 // queries of one wide launch (4 tiles of 256)
// E = 768 (scan_coarse_wide_kernel<4, 0, 24>, opt-in: clipmi_topk_ip_wide_i8): 1024 as well = 8 tiles of 128, eight workgroups of
// an XCD on every block. The pass is matrix-bound, so the eight readers cost L2 hits the MFMAs hide, while 512 per launch would
// stream the copy from HBM twice per 1024 queries and double the sample / re-score / select launches per query.
constexpr int WIDE768_MAX_Q = 1024;
constexpr int WIDE_TILE_SETS = 4;                // 64-query sets per tile: 4 x 32 KiB of image (E = 512)
constexpr int WIDE768_TILE_SETS = 2;             // E = 768: 2 x 48 KiB
inline int wide_max_q(int E) { return E == 768 ? WIDE768_MAX_Q : WIDE_MAX_Q; }
constexpr int WIDE_FLUSH = 128;                  // pending pairs per wave that trigger a flush
constexpr int WIDE_LIST = WIDE_FLUSH + 256;      // a (row tile, query group) block appends <= 256 behind a pending flush
constexpr size_t WIDE_WAVE_BYTES = (size_t)WIDE_LIST * 8;
constexpr long long WIDE_CAP = 1ll << 15;        // candidate slots per query of a wide pass (overflow arms the exact fallback)

struct WideArgs {
    const signed char* dbc;      // int8 copy, 32-row blocks of [E / 32][64][16 B] (quantize_rows_i8_kernel)
    const float2* rmeta;         // per row (block scale, error norm), padded to 32 rows
    const float2* bmeta;         // per 32-row block (scale, largest error norm)
    const float* qmeta;          // [4][qs]
    const uint4* qimage;         // all queries' image, 64-query sets of 32 KiB (48 KiB at E = 768; coarse_prep_kernel, wide form)
    long long row0, nrows;       // rows [row0, row0 + nrows), row0 % 32 == 0
    int Q, qs;
    int nqt, spt;                // query tiles, 64-query sets per tile (<= WIDE_TILE_SETS; WIDE768_TILE_SETS at E = 768)
    uint2* cand;                 // [Q][cap]
    unsigned* gcnt;              // [qs]
    long long cap;
    unsigned* overflow;
    int map_mode, pf_mode;       // development knobs (CLIPMI_WIDE_MAP / CLIPMI_WIDE_PF)
};

typedef int i32x16 __attribute__((ext_vector_type(16)));

// ---- what the two wide scans share ----------------------------------------------------------------------------------------
// The exact test of a (row, query) pair is  D s + a_r Y_q >= T_q  (T_q = (tau - margin) / t_q, Y_q = 1.001 ||y|| / t_q;
// s the block's scale). Integer pre-test, one per lane (= query): no row of the block can pass unless
// D >= (T_q - amax_block Y_q) / s, rounded down with slack for the f32 roundings on both sides (|D| <= 32 KS 127^2
// < 2^24 is exact in f32: 8.3e6 at 512, 1.24e7 at 768 - static_assert in the kernels) - so the lane's largest D decides, and
// the per-row test runs only where it can succeed.
// The slack, for |x| up to 1.3e7 (u = 2^-24): a row passes when fl(D s + fl(a Y)) >= T, i.e. D >= x* - u (|T| + a Y) / s
// with x* = (T - a Y) / s in real numbers. a / s <= 1.001 sqrt(E) / 2 (half a step per component) and Y <= 1.001 * 127
// sqrt(E), so a Y / s <= 4.9e4 at E = 768 and |T| / s <= |x*| + 4.9e4: D >= x* - u |x*| - 0.006. The computed
// xq = fl(fl(T - a Y) fl(1 / s)) has three roundings: |xq - x*| <= 3.0001 u |x*| (inv_s = 1 / s, or the hardware's
// reciprocal: 1 ulp more, far inside what is taken). The two subtractions below round to
// half a unit each while |xq| < 2^24 (to u |xq| beyond). Needed: 1.006 + 4.1 u |x| = 1.006 + 2.5e-7 |x| (4.2 at
// |x| = 1.3e7); taken: 2 + 2e-6 |x| (28 there) - the constants of the 512 form, which needed 1.004 + 2.5e-7 |x|, hold
// at 768 unchanged. Past 2^24 no D exists: x* > 1.3e7 passes nothing and x* < -1.3e7 everything, and the relative
// slack (2e-6 against 6 u) keeps dmin on the right side of every possible D.
// An all-zero block (s = 0: inv_s = inf) clamps to +-1e9 by its sign; a threshold of -inf (none yet) and NaN give "always";
// +inf (a padding query) would give inf - inf = NaN = "always" and is the CALLER's to exclude.
// bm = the block's (scale, largest error norm); returns the smallest D that can pass.
__device__ __forceinline__ int i8_pretest_dmin(float tq, float yq, float2 bm, float inv_s) {
    float xq = fmaf(-bm.y, yq, tq) * inv_s;
    xq = fminf(fmaxf(xq, -1.0e9f), 1.0e9f);                   // before the slack: no inf - inf; fmaxf(NaN, c) = c: NaN -> always
    xq = xq - 2.0f - fabsf(xq) * 2e-6f;
    return (int)floorf(xq);
}

// the largest of a lane's 16 sums (32 rows x 1 query: its half of the rows): three levels of max3, not a chain of eight
__device__ __forceinline__ int max16(const i32x16& acc) {
    auto max3 = [](int a_, int b_, int c_) { const int m_ = a_ > b_ ? a_ : b_; return m_ > c_ ? m_ : c_; };
    const int m0 = max3(acc[0], acc[1], acc[2]), m1 = max3(acc[3], acc[4], acc[5]), m2 = max3(acc[6], acc[7], acc[8]);
    const int m3 = max3(acc[9], acc[10], acc[11]), m4 = max3(acc[12], acc[13], acc[14]);
    const int ma = max3(m0, m1, m2), mb = max3(m3, m4, acc[15]);
    return ma > mb ? ma : mb;
}

// workgroup -> (query tile, row lane) of `ntiles` query tiles: blocks b, b + 8, ... share an XCD (observed dispatch; speed only),
// the tiles of a row lane are such neighbours. nrl = row lanes of the launch; false: a workgroup beyond the last whole one.
__device__ __forceinline__ bool wide_tile_map(int ntiles, int map_mode, int& qt, int& rl, int& nrl) {
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3, jb = gridDim.x >> 3;
    const int rlx = jb / ntiles;                              // row lanes per XCD label
    if (j >= rlx * ntiles) return false;
    qt = j % ntiles, nrl = rlx * 8;
    rl = map_mode == 1 ? x * rlx + (j / ntiles) : (j / ntiles) * 8 + x;
    return true;
}

// buffer resource of 32-row block `block` of the int8 copy (`bytes` each): rebased per block, so 32-bit offsets suffice for any
// copy size - a load is scalar resource + ONE lane-offset register + a scalar k-step offset
__device__ __forceinline__ __amdgpu_buffer_rsrc_t i8_block_rsrc(const signed char* dbc, int block, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<signed char*>(dbc) + (size_t)block * bytes, 0, bytes, 0x00020000);
}

// KS = E / 32 k-steps: 16 (E = 512, 8 waves: this block's rows and the next one's, 2 x 64 registers, at two waves per SIMD) or
// 24 (E = 768). At 768 the two row sets are 2 x 96 registers; with two accumulators (32) and the fragment ring (16) that is past
// the 256 of a wave at two per SIMD, so the 768 form is the FOUR-wave workgroup: one wave per SIMD owns the SIMD's whole
// register file (512: 256 VGPRs + 256 AGPRs), the allocator keeps what does not fit in VGPRs in AGPRs (MFMA reads its A operand
// from either file) and nothing goes to scratch. The compare of group G - 1 already runs between group G's MFMAs inside one
// wave; what the second wave per SIMD hid at 512 - the append path and the wait for the next block - is exposed here
// (speed not measured).
template <int WAVES, int ABL = 0, int KS = 16>      // ABL: development ablations (1 no compare, 2 few LDS reads, 3 no row loads)
__global__ void __launch_bounds__(WAVES * 64) scan_coarse_wide_kernel(WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(KS == 16 || (KS == 24 && WAVES == 4), "E = 512 (any WAVES) or E = 768 as the four-wave form");
    static_assert(KS * 32 * 127 * 127 < (1 << 24), "the integer sums must be exact in f32 (pretest, append)");
    constexpr int BLOCK_BYTES = 32 * 32 * KS;                 // one 32-row block of the copy
    constexpr int SET_ENTRIES = 2 * KS * 64;                  // 16-byte entries of one 64-query set's image (32 KiB)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;                   // accumulator column (query of a 32-group), row half

    int qt, rl, nrl;
    if (!wide_tile_map(a.nqt, a.map_mode, qt, rl, nrl)) return;
    const int set0 = qt * a.spt;
    int nsets = ((a.Q + 63) >> 6) - set0;
    nsets = nsets > a.spt ? a.spt : nsets;
    if (nsets < 1) return;
    const int qbase = set0 * 64;

    uint4* qimg = reinterpret_cast<uint4*>(smem);
    {
        const uint4* src = a.qimage + (size_t)set0 * SET_ENTRIES;
        const int ne = nsets * SET_ENTRIES;                   // multiple of 2048
        for (int base = tid; base < ne; base += 8 * WAVES * 64) {
            uint4 v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = base + i * WAVES * 64 < ne ? src[base + i * WAVES * 64] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (base + i * WAVES * 64 < ne) qimg[base + i * WAVES * 64] = v[i];
        }
    }
    float* ltau = reinterpret_cast<float*>(smem + (size_t)a.spt * SET_ENTRIES * 16);       // [256] scaled thresholds (128 used at E = 768)
    float* lyt = ltau + 64 * WIDE_TILE_SETS;                                               // [256] 1.001 ||y|| / t_q
    for (int i = tid; i < 64 * WIDE_TILE_SETS; i += WAVES * 64) {
        const bool act = i < nsets * 64 && qbase + i < a.Q;
        ltau[i] = act ? a.qmeta[2 * a.qs + qbase + i] : INFINITY;
        lyt[i] = act ? a.qmeta[a.qs + qbase + i] : 0.f;
    }
    uint2* list = reinterpret_cast<uint2*>(reinterpret_cast<char*>(lyt + 64 * WIDE_TILE_SETS) + (size_t)wave * WIDE_WAVE_BYTES);
    __syncthreads();

    // block indices fit 32 bits (N < 2^32 rows) and are wave-uniform: kept in scalar registers, so the block meta is a
    // scalar load (a vector load here put a vmcnt(0) at the head of the group loop - behind the 16 KB prefetch) and the row
    // loads are scalar base + one lane offset
    const int blk0 = (int)(a.row0 >> 5);
    const int nblk = blk0 + (int)((a.nrows + 31) >> 5);
    const int tw = nrl * WAVES;
    const unsigned last_row32 = (unsigned)(a.row0 + a.nrows - 1);
    int npend = 0;                                            // wave-uniform: pairs pending in `list`

    int blk = __builtin_amdgcn_readfirstlane(blk0 + rl * WAVES + wave);
    if (blk < nblk) {
        uint4 Ta[KS], Tb[KS];                                 // this block's rows / the next block's (in flight for a whole step)
        // rows are loaded as buffer loads (i8_block_rsrc) - 64-bit per-lane addresses cost 26 registers here
        const unsigned lane16 = (unsigned)lane * 16u;
        auto load_block = [&](int b_, uint4 (&dst)[KS]) {
            const __amdgpu_buffer_rsrc_t rs = i8_block_rsrc(a.dbc, b_, BLOCK_BYTES);
#pragma unroll
            for (int s_ = 0; s_ < KS; ++s_)
                dst[s_] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, lane16, s_ * 1024, (CLIPMI_NT_MASK & 2) ? 2 : 0));
        };
        load_block(blk, Ta);
        // the block's (scale, largest error norm): fetched with the rows, one block ahead (a load at the head of a block
        // would be waited for behind that block's own 16 KB prefetch: vmcnt counts in order)
        float2 bm = a.bmeta[blk], bmn = bm;
        // One 32-row block against the tile's 32-query groups. The next block's 16 KB are requested during group `pf_g`
        // and land under the remaining MFMAs: group 0 in the tile-0 workgroup of a row lane, halfway through the step in
        // the other tiles' workgroups of the same row lane (same rows, same order, same XCD; a measured wash - 41 % of the
        // L2 requests hit either way - kept because it spreads the four workgroups' HBM bursts).
        // The compare of group G - 1 is issued between the MFMAs of group G (two accumulators): alone it left the matrix
        // pipe idle for the accumulator drain, a dependent VALU chain and a branch per group (19 % of the launch, by ablation).
        // Returns false after the wave's last block.
        const int ng = 2 * nsets;
        const int pf_g = (qt == 0 || a.pf_mode == 1) ? 0 : a.pf_mode == 2 ? ng - 2 : a.pf_mode == 3 ? qt * ng / a.nqt : ng / 2;
#ifndef CLIPMI_WIDE_BR
#define CLIPMI_WIDE_BR 4
#endif
        constexpr int BR = CLIPMI_WIDE_BR;                     // ring of query fragments: LDS reads run BR MFMAs ahead
        auto run_block = [&](uint4 (&T)[KS], uint4 (&TN)[KS]) -> bool {
            const int nxt = __builtin_amdgcn_readfirstlane(blk + tw);
            const bool has_next = nxt < nblk;
            const float inv_s = 1.0f / bm.x;
            uint4 B[BR];                                       // ring of query fragments, continuous over the groups
            {
                const uint4* img0 = qimg + lane;
#pragma unroll
                for (int p_ = 0; p_ < BR; ++p_) B[p_] = img0[p_ * 64];
            }
            // The integer pre-test (i8_pretest_dmin), one per lane (= query). +inf thresholds (padding queries: any Q that is not
            // a multiple of 32) are "never" by an explicit test - inf - inf would be NaN = "always", and every block would then
            // run the 16-ballot append path for its padding lanes.
            auto pretest = [&](const i32x16& acc, float tq, float yq) -> bool {
                if (tq == INFINITY) return false;
                return max16(acc) >= i8_pretest_dmin(tq, yq, bm, inv_s);
            };
            // per-row test with the block's largest error norm in place of the row's own (a few per cent looser, a superset
            // all the same): no per-row meta loads here - they would queue behind the next block's 16 KB
            auto append = [&](const i32x16& acc, int G, float tq, float yq) {
                const unsigned rbase = (unsigned)blk * 32u + 4u * (unsigned)h;      // rows fit 32 bits (N < 2^32 - 1)
                const float ay = bm.y * yq;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned row = rbase + (unsigned)((i & 3) + 8 * (i >> 2));
                    const float val = fmaf((float)acc[i], bm.x, ay);
                    const bool pass = (val >= tq) && (row <= last_row32);
                    const unsigned long long m = __ballot(pass);
                    if (m) {
                        const int pos = pair_slot(m, npend);
                        if (pass) list[pos] = make_uint2((unsigned)(G * 32 + n), row);
                        npend += __builtin_popcountll(m);
                    }
                    if ((i & 3) == 3 && npend > WIDE_FLUSH) {              // <= 256 appends between two tests
                        pairs_flush(list, npend, qbase, a.gcnt, a.cand, a.cap, a.overflow);
                        npend = 0;
                    }
                }
            };
            // group G's 16 MFMAs into `acc`; group G - 1's pre-test (accumulator `accp`) between them
            auto run_group = [&](int G, i32x16& acc, const i32x16& accp, float& tq, float& yq, float tqp, float yqp) {
                if (G == pf_g) {
                    if (ABL == 3) {
#pragma unroll
                        for (int s_ = 0; s_ < KS; ++s_) TN[s_] = T[s_];
                    } else {
                        load_block(has_next ? nxt : blk, TN);
                    }
                    bmn = a.bmeta[has_next ? nxt : blk];
                }
                const uint4* img = qimg + (size_t)G * (KS * 64) + lane;
                const uint4* imgn = qimg + (size_t)(G + 1 < ng ? G + 1 : G) * (KS * 64) + lane;   // the next group's head
                tq = ltau[G * 32 + n];                                     // read ahead of the fragments: no wait of their own
                yq = lyt[G * 32 + n];
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = 0;
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int s_ = 0; s_ < KS; ++s_) {
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(i32x4, T[s_]),
                                                                __builtin_bit_cast(i32x4, B[s_ % BR]), acc, 0, 0, 0);
                    if (ABL != 2) B[s_ % BR] = s_ + BR < KS ? img[(s_ + BR) * 64] : imgn[(s_ + BR - KS) * 64];
                }
                bool hitp = false;
                if (ABL != 1) hitp = pretest(accp, tqp, yqp);
#pragma unroll
                for (int s_ = 0; s_ < KS; ++s_) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      // MFMA of k-step s
                    if (ABL != 2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);        // DS read: the fragment BR k-steps on
                    if (ABL != 1) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);        // VALU: two of the pre-test's ~30
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ABL == 1) asm volatile("" :: "v"(accp), "v"(tqp), "v"(yqp));
                if (G > 0 && __ballot(hitp)) append(accp, G - 1, tqp, yqp);
            };
            i32x16 accA, accB;
            float tqA = 0.f, yqA = 0.f, tqB = INFINITY, yqB = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) accB[i] = 0;
            for (int G = 0; G < ng; G += 2) {
                run_group(G, accA, accB, tqA, yqA, tqB, yqB);
                run_group(G + 1, accB, accA, tqB, yqB, tqA, yqA);
            }
            if (ABL != 1 && __ballot(pretest(accB, tqB, yqB))) append(accB, ng - 1, tqB, yqB);
            blk = nxt;
            bm = bmn;
            return has_next;
        };
        while (run_block(Ta, Tb) && run_block(Tb, Ta)) {}
    }
    pairs_publish<64 * WIDE_TILE_SETS, WAVES * 64>(smem, list, npend, qbase, a.gcnt, a.cand, a.cap, a.overflow);      // the image is dead now
}

// =================================================================================================
// Wide pass, second form (more than 256 queries): QUERIES IN REGISTERS, ROWS THROUGH AN LDS RING.
//
// scan_coarse_wide_kernel keeps a 256-query tile's image in LDS and the rows in registers: one KiB of LDS per MFMA, the rows'
// fragments twice over (this block + the next) in 128 registers, 256 registers with spills - no room for a deeper fragment ring,
// and four workgroups fetch every block. Here a wave owns NG (two, or one) 32-query groups for the whole launch (their B
// fragments: 64 NG registers), a workgroup's 8 waves = a tile of 256 NG queries, and the 32-row blocks arrive by LDS-DMA in a
// ring of NB slots (the copy's block layout IS the MFMA register image, so the DMA deposits fragments as they are read): with
// two groups every row fragment read from LDS feeds two MFMAs (half a KiB per MFMA) and two workgroups fetch a block instead of
// four. All 8 waves walk the same blocks; ONE barrier per block publishes the slot that landed and frees the one that was
// read, waves 4-7 take it half a block later than waves 0-3, and the fragment ring in registers never drains.
// The compare is scan_coarse_wide_kernel's integer pre-test per lane; lanes that pass queue their sums and the per-row test
// runs on 64 queued hits at a time (see the kernel). One call of 1 024 queries at 10 M rows: 6.26 -> 5.46 ms.
// =================================================================================================
constexpr int W2_MIN_Q = 192;                     // query counts below this take scan_coarse_wide_kernel (rows in registers, queries in
                                                  // LDS: 1.17 ms against 1.23 at 128 queries, 1.65 against 1.59 at 200 - 10 M rows,
                                                  // profiles/r05_wide_balanced_tiles.txt)
constexpr int W2_SLOT = 16384 + 256;              // a ring slot: 16 KiB of fragments + the block's meta

template <int N_>
__device__ __forceinline__ void w2_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }

template <int NB, int NG>      // ring slots; 32-query groups per wave (2: tiles of 512 queries, 1: tiles of 256)
__global__ void __launch_bounds__(512) scan_coarse_wide2_kernel(WideArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = 16;
    constexpr int TILE_Q = 8 * NG * 32;                       // queries of a workgroup
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    // workgroup -> (query tile, row lane): blocks b, b + 8, ... share an XCD; the tiles of a row lane are such neighbours.
    // Round 5 - BALANCED tiles (640 queries used to be a full tile + a quarter-full one at the full tile's
    // price): the call's 32-query groups are dealt evenly over the tiles, and inside a tile evenly over the waves - a wave owns
    // cnt = 0, 1 or .. NG consecutive groups (waves 0 .. rem-1 one more than the rest; SIMD partners are waves w, w + 4, so a
    // tile of 10 groups loads its SIMDs 3 / 3 / 2 / 2 instead of 4 / 4 / 2 / 0) and SKIPS the MFMAs of the groups it does not have.
    const int ngroups = (a.Q + 31) >> 5;
    const int ntile = (ngroups + 8 * NG - 1) / (8 * NG);
    int qt, rl, nrl;
    if (!wide_tile_map(ntile, 0, qt, rl, nrl)) return;
    nrl = __builtin_amdgcn_readfirstlane(nrl);
    const int gpt = (ngroups + ntile - 1) / ntile;                                   // groups per tile (the last may hold fewer)
    const int tg0 = qt * gpt, tgn = (ngroups - tg0) < gpt ? (ngroups - tg0) : gpt;   // this tile's groups [tg0, tg0 + tgn)
    const int gbase_ = tgn >> 3, grem_ = tgn & 7;
    const int cntw = __builtin_amdgcn_readfirstlane(gbase_ + (wave < grem_ ? 1 : 0));              // this wave's groups
    const int wg0 = __builtin_amdgcn_readfirstlane(wave * gbase_ + (wave < grem_ ? wave : grem_)); // its first group, tile-local
    const int qbase = tg0 * 32;
    char* ring = smem;                                            // NB slots of 16 KiB of fragments + 256 B of block meta
    uint2* list = reinterpret_cast<uint2*>(smem + (size_t)NB * W2_SLOT + (size_t)wave * WIDE_WAVE_BYTES);

    // this wave's NG query groups: fragments (the wide image of coarse_prep_kernel: entry [(G 16 + s) 64 + lane]) and per-lane
    // thresholds - constant over the launch
    uint4 Bq[NG][KS];
    float tq[NG], yq[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int G = tg0 + wg0 + g;
        const bool has_img = g < cntw && G * 32 < a.qs;             // the image covers qs (a multiple of 64) queries
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_)
            Bq[g][s_] = has_img ? a.qimage[((size_t)G * KS + s_) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
        const int qi = G * 32 + n;
        const bool act = g < cntw && qi < a.Q;
        tq[g] = act ? a.qmeta[2 * a.qs + qi] : INFINITY;
        yq[g] = act ? a.qmeta[a.qs + qi] : 0.f;
    }

    const int blk0 = (int)(a.row0 >> 5);
    const int nblk = blk0 + (int)((a.nrows + 31) >> 5);
    const unsigned last_row32 = (unsigned)(a.row0 + a.nrows - 1);
    const int first = __builtin_amdgcn_readfirstlane(blk0 + rl);
    const int nk = first < nblk ? (nblk - first + nrl - 1) / nrl : 0;       // blocks of this row lane (the same for all 8 waves)
    int npend = 0;
    if (nk > 0) {
        // block k of the row lane -> ring slot k % NB; this wave moves k-steps 2 wave, 2 wave + 1 of it (2 x 1 KiB). Past the
        // last block the last one is fetched again (into a slot nobody reads): the counted waits below stay valid to the end.
        // (buffer loads: scalar resource rebased per block, ONE long-lived lane-offset register - per-lane 64-bit addresses were
        //  recycled as fragment registers and the compiler then waited vmcnt(0) for the DMA before the first LDS read)
        const unsigned lane16 = (unsigned)lane * 16u, lane4 = (unsigned)lane * 4u;
        auto issue = [&](int k) {
            const int b_ = __builtin_amdgcn_readfirstlane(first + (k < nk ? k : nk - 1) * nrl);
            const __amdgpu_buffer_rsrc_t rs = i8_block_rsrc(a.dbc, b_, 32 * 512);
            char* dst = ring + (size_t)(k & (NB - 1)) * W2_SLOT + (size_t)(2 * wave) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) char*)dst, 16, lane16, (2 * wave) * 1024, 0,
                                                     (CLIPMI_NT_MASK & 16) ? 2 : 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) char*)(dst + 1024), 16, lane16,
                                                     (2 * wave + 1) * 1024, 0, (CLIPMI_NT_MASK & 16) ? 2 : 0);
            // the block's (scale, largest error norm) travels with it: 8 bytes through a buffer of 8 (lanes 2.. read past it: zeros),
            // every wave writes the same words - a third DMA per block and wave keeps the counted waits uniform. (A scalar load
            // returns out of order on lgkmcnt, a vector load shares vmcnt with the DMA and the compiler waits vmcnt(0) for it.)
            const __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float2*>(a.bmeta) + b_, 0, 8, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rm, (__attribute__((address_space(3))) char*)(ring + (size_t)(k & (NB - 1)) * W2_SLOT + 16384),
                                                     4, lane4, 0, 0, 0);
        };
#pragma unroll
        for (int k = 0; k < NB - 1; ++k) issue(k);
        const unsigned ring_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)ring + lane16;
        const unsigned list_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)reinterpret_cast<char*>(list);
        // The compare of scan_coarse_wide_kernel (see there): an integer pre-test per lane (= query), the per-row test and the
        // ballot appends only behind it. It follows the block's MFMAs; waves 4-7 run HALF A BLOCK behind waves 0-3 (their barrier
        // sits at the end of a block instead of its middle), so on every SIMD one wave's compare runs under its partner's MFMAs.
        auto pretest = [&](const i32x16& acc, float tq_, float yq_, float2 bm_) -> bool {
            const int dmin = i8_pretest_dmin(tq_, yq_, bm_, __builtin_amdgcn_rcpf(bm_.x));      // 1 ulp: far inside the slack
            return (max16(acc) >= dmin) & (tq_ != INFINITY);      // +inf (padding query): never; no branch in the MFMA stream
        };
        // A lane whose pre-test passes ("hit": one (query, block) pair with possibly a passing row) does NOT run the per-row test
        // there: that is 16 values x (convert, fma, compare, ballot, branch) for the whole wave per hit, the wave is coupled to the
        // other seven by the ring's barrier, and in the last segment one of the 16 (wave, group) pairs of a workgroup hits in four
        // blocks out of five. The hit lanes drop their 16 sums + (query, first row, scale, a_max Y_q, T_q) into the wave's queue in
        // LDS (96 bytes each, by ballot prefix); when 64 are queued every lane takes ONE entry and the 16 ballot rounds serve 64
        // hits at once. Same per-row test, same survivors (their order in the lists differs; the lists are unordered).
        // (All LDS traffic here is inline asm: a compiler-visible access waits vmcnt(0) for the DMA in flight.)
        int hcount = 0;                                            // wave-uniform: entries queued
        const unsigned hq_a = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(smem + (size_t)NB * W2_SLOT + 8 * WIDE_WAVE_BYTES) +
                              (unsigned)wave * (64u * 96u);
        auto drain = [&]() {
            const bool mine = lane < hcount;
            const unsigned ea = hq_a + (unsigned)(mine ? lane : 0) * 96u;
            i32x4 mt0, mt1;
            asm volatile("s_waitcnt lgkmcnt(0)\n\tds_read_b128 %0, %2 offset:64\n\tds_read_b128 %1, %2 offset:80\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(mt0), "=&v"(mt1) : "v"(ea) : "memory");
            const unsigned qidx = (unsigned)mt0[0], rbase = (unsigned)mt0[1];
            const float s_ = __int_as_float(mt0[2]), ay = __int_as_float(mt0[3]), tq_ = __int_as_float(mt1[0]);
#pragma unroll
            for (int i4 = 0; i4 < 4; ++i4) {
                i32x4 v;
                asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(ea + (unsigned)i4 * 16u) : "memory");
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const unsigned row = rbase + (unsigned)(c + 8 * i4);
                    const float val = fmaf((float)v[c], s_, ay);
                    const bool pass = mine && (val >= tq_) && (row <= last_row32);
                    const unsigned long long m = __ballot(pass);
                    if (m) {
                        // (pair_slot written out: through it hipcc swaps two instructions at each of this kernel's 56 appends)
                        const int pos = npend + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                        if (pass) {
                            const uint2 ent = make_uint2(qidx, row);
                            asm volatile("ds_write_b64 %0, %1" ::"v"(list_a + (unsigned)pos * 8u), "v"(ent) : "memory");
                        }
                        npend += __builtin_popcountll(m);
                    }
                }
                if (npend > WIDE_FLUSH) {                          // <= 256 appends between two tests
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    pairs_flush(list, npend, qbase, a.gcnt, a.cand, a.cap, a.overflow);
                    npend = 0;
                }
            }
            hcount = 0;
        };
        auto enqueue = [&](const i32x16& acc, int g, bool hit, int blk_, float2 bm_) {
            const unsigned long long m = __ballot(hit);
            if (!m) return;
            const int nh = __builtin_popcountll(m);
            if (hcount + nh > 64) drain();
            if (hit) {
                const unsigned ea = hq_a + (unsigned)pair_slot(m, hcount) * 96u;
                const i32x4 v0 = {acc[0], acc[1], acc[2], acc[3]}, v1 = {acc[4], acc[5], acc[6], acc[7]};
                const i32x4 v2 = {acc[8], acc[9], acc[10], acc[11]}, v3 = {acc[12], acc[13], acc[14], acc[15]};
                const i32x4 m0 = {(wg0 + g) * 32 + n, (int)((unsigned)blk_ * 32u + 4u * (unsigned)h), __float_as_int(bm_.x),
                                  __float_as_int(bm_.y * yq[g])};
                const i32x4 m1 = {__float_as_int(tq[g]), 0, 0, 0};
                asm volatile("ds_write_b128 %0, %1\n\tds_write_b128 %0, %2 offset:16\n\tds_write_b128 %0, %3 offset:32\n\t"
                             "ds_write_b128 %0, %4 offset:48\n\tds_write_b128 %0, %5 offset:64\n\tds_write_b128 %0, %6 offset:80"
                             ::"v"(ea), "v"(v0), "v"(v1), "v"(v2), "v"(v3), "v"(m0), "v"(m1) : "memory");
            }
            hcount += nh;
        };
        // The fragment ring never drains: the reads behind k-steps 12-15 of block k fetch k-steps 0-3 of block k + 1. Barrier b
        // publishes block b + 1 (everyone's pieces have landed) and frees block b - 1's slot for block b + NB - 1; waves 0-3 reach
        // it in the MIDDLE of block b, waves 4-7 at the END of block b - 1 (before block 0 for b = 0): same count, half a block apart.
        // lgkmcnt by hand: LDS operations complete in order, 4 fragment reads are in flight before every k-step, so lgkmcnt(3)
        // retires the oldest; anything younger in between (the meta read, an append's list writes) only makes a wait retire more.
        const bool late = wave >= 4;
        i32x4 A[4];
        auto frag = [&](int k, int s_) -> unsigned { return ring_a + (unsigned)(k & (NB - 1)) * (unsigned)W2_SLOT + (unsigned)s_ * 1024u; };
        auto ring_barrier = [&](int b_) {
            // my pieces of block b + 1 have landed (NB - 3 younger blocks may be in flight)
            w2_wait_vmcnt<3 * (NB - 3)>();
            __builtin_amdgcn_s_barrier();
            issue(b_ + NB - 1);
        };
        // block 0: my pieces landed (NB - 2 younger blocks may be in flight), then everyone's
        w2_wait_vmcnt<3 * (NB - 2)>();
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int p_ = 0; p_ < 4; ++p_) asm volatile("ds_read_b128 %0, %1" : "=v"(A[p_]) : "v"(frag(0, p_)));
        if (late) ring_barrier(0);
        // The block loop exists once per number of groups the wave really has (NGA = 0 .. NG; wave-uniform, chosen ONCE): a
        // wave-uniform `if` around the MFMAs inside one loop was tried first and tripled the launch's time - any control flow
        // inside the hand-counted stream costs the schedule. All copies take the same barriers at the same places.
        // (acc has a fixed bound: with `acc[NG]` the operands of the refill's asm are type-dependent and hipcc drops the
        //  kernel's HOST stub without a diagnostic - the library then fails to load with an undefined __device_stub__ symbol)
#define W2_BLOCKS(NGA)                                                                                                 \
        for (int k = 0; k < nk; ++k) {                                                                                 \
            const int blk = __builtin_amdgcn_readfirstlane(first + k * nrl);                                           \
            i32x16 acc[2];                                                                                             \
            _Pragma("unroll") for (int g = 0; g < 2; ++g)                                                              \
                _Pragma("unroll") for (int i = 0; i < 16; ++i) acc[g][i] = 0;                                          \
            uint2 pm = make_uint2(0u, 0u);                    /* the block's meta, read from its slot behind k-step 0 */ \
            _Pragma("unroll") for (int s_ = 0; s_ < KS; ++s_) {                                                        \
                /* (k-step 4's wait also retires the meta read: it is older than the fragment of k-step 5) */          \
                if (s_ == 4) asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(A[s_ & 3]), "+v"(pm));                         \
                else asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(A[s_ & 3]));                                           \
                _Pragma("unroll") for (int g = 0; g < (NGA); ++g)                                                      \
                    acc[g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s_ & 3], __builtin_bit_cast(i32x4, Bq[g][s_]), acc[g], 0, 0, 0); \
                if (s_ == KS / 2 - 1 && !late) ring_barrier(k);                                                        \
                if (s_ == KS - 1 && late && k + 1 < nk) ring_barrier(k + 1);                                           \
                /* the refill may not overtake the MFMAs that read the register: tie it to their results */            \
                const unsigned fa = s_ + 4 < KS ? frag(k, s_ + 4) : frag(k + 1, s_ + 4 - KS);                          \
                asm volatile("ds_read_b128 %0, %1" : "=v"(A[s_ & 3]) : "v"(fa), "v"(acc[0]), "v"(acc[(NGA) > 1 ? (NGA) - 1 : 0])); \
                if (s_ == 0)                                                                                           \
                    asm volatile("ds_read_b64 %0, %1" : "=v"(pm) : "v"(ring_a - lane16 + (unsigned)(k & (NB - 1)) * (unsigned)W2_SLOT + 16384u)); \
            }                                                                                                          \
            const float2 bm = make_float2(__uint_as_float(pm.x), __uint_as_float(pm.y));                               \
            _Pragma("unroll") for (int g = 0; g < (NGA); ++g) enqueue(acc[g], g, pretest(acc[g], tq[g], yq[g], bm), blk, bm); \
        }
        if (cntw >= NG) { W2_BLOCKS(NG) }
        else if (NG > 1 && cntw == 1) { W2_BLOCKS(1) }
        else { W2_BLOCKS(0) }
#undef W2_BLOCKS
        if (hcount) drain();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        w2_wait_vmcnt<0>();                                   // the re-fetched tail blocks: nothing may land after the ring is reused
    }
    pairs_publish<TILE_Q, 512>(smem, list, npend, qbase, a.gcnt, a.cand, a.cap, a.overflow);      // the ring is dead now
}

}  // namespace
}  // namespace clipmi
