// topk.hip — exact flat inner-product top-K over a packed [N][E] f32 matrix (gfx950).
//
// Replaces `index.search(features, k + offset + 1)` (reference query-index.py:111) with an exact
// streaming pass. HBM-bound: the matrix is read once per batch of <= 16
// queries; scores are produced by v_mfma_f32_16x16x4_f32 (exact f32, one fmaf chain per
// (row, query) in a FIXED order, restated in oracle/topk_oracle.c) and selected per wavefront
// with a threshold filter + bounded candidate buffer in LDS.
//
// Score order ("score order" in DESIGN.md): for row r, query q, E = 16*NT:
//     acc = 0; for t in [0,NT) for c in [0,4) for g in [0,4): k = 16t + 4g + c;
//         acc = fmaf(db[r][k], q[k], acc)
// (t,c) is one MFMA instruction; g is the MFMA's internal k index (lane >> 4).
//
// Ordering rule everywhere (wave select, block merge, cross-rank merge, oracle):
//     a beats b  <=>  a.score > b.score || (a.score == b.score && a.id < b.id); NaN never selected.
#include "common.hpp"
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <type_traits>
#include <hip/hip_ext.h>

namespace clipmi {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Cache policy of the once-read streams (CLIPMI_NT_MASK, compile time): bit 0 the coarse copies of the 64-query
// passes, bit 1 the first wide form's rows (65-256 queries), bit 4 the second form's, bit 2 the re-scored f32 rows, bit 3 the exact
// f32 scan. A set bit = the non-temporal hint
// (`nt`): the 64-query int8 scan streams 5.2 GB per call and reads 6.15 -> 6.62 TB/s with it; the first wide form (one workgroup
// per block) gains 1-5 %; the others lose or do not move (bits 2, 3, 4 stay clear).
#ifndef CLIPMI_NT_MASK
#define CLIPMI_NT_MASK 3
#endif
template <int BIT>
__device__ __forceinline__ f32x4 ld16_f(const float* p) {
    if constexpr ((CLIPMI_NT_MASK >> BIT) & 1) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    else return *reinterpret_cast<const f32x4*>(p);
}

constexpr int SAMPLE_MIN_N = 65536;     // below this the pre-pass is not worth its launches
constexpr int LDS_LIMIT = 160 * 1024 - 512;

__device__ __forceinline__ bool beats(float sa, unsigned ia, float sb, unsigned ib) {
    return sa > sb || (sa == sb && ia < ib);
}

// LDS traffic of ONE wave is processed in issue order; this only has to stop the compiler from
// moving LDS accesses across the point and to drain the wave's outstanding LDS operations.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Keep the best min(n, K) of the n candidates in buf[0..n) (n = *cnt_p, wave-uniform), sorted by
// the ordering rule, using rank counting: rank(e) = #{j : cand_j beats cand_e}. Ids are unique,
// so ranks are a permutation. All 64 lanes of the wave must call this together.
__device__ void wave_compact(uint2* buf, uint2* scratch, int* cnt_p, float* thr_p, int K, int lane) {
    const int n = *cnt_p;
    for (int e = lane; e < n; e += 64) {
        const uint2 me = buf[e];
        const float ms = __uint_as_float(me.x);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const uint2 o = buf[j];
            rank += beats(__uint_as_float(o.x), o.y, ms, me.y) ? 1 : 0;
        }
        if (rank < K) scratch[rank] = me;
    }
    wave_lds_sync();
    const int m = n < K ? n : K;
    for (int e = lane; e < m; e += 64) buf[e] = scratch[e];
    if (lane == 0) {
        *cnt_p = m;
        *thr_p = (n >= K) ? __uint_as_float(scratch[K - 1].x) : -INFINITY;
    }
    wave_lds_sync();
}

struct ScanArgs {
    const float* db;        // [nrows][E]
    long long nrows;        // >= 1
    const float* q;         // first query of this group, [QA][E]
    int QA;                 // active queries in this pass, 1..16*QG
    int K;
    int C;                  // candidate capacity per (wave, query): multiple of 16, >= K + 16
    int wave_bytes;         // LDS bytes per wave
    const float* thr_in;    // [QA] initial thresholds (valid lower bounds) or nullptr
    uint2* cand;            // [QA][cap] dense candidate lists (unsorted); entries per query <= rows of the launch <= cap
                            // (every (query, row) pair is published at most once: make_plan's cap = min(NL * C, rows))
    unsigned* gcnt;         // [32] entries used per query; zeroed on the stream before the launch
    long long cap;
    const unsigned* run_if; // optional device flag: the kernel exits at once when *run_if == 0
    int q_total;            // gridDim.y > 1 only: queries over all groups; group y takes queries [y*QA, y*QA + QA) and
                            // the matching slices of q, thr_in, cand, gcnt
};

// PREPASS only changes the kernel's NAME (profilers average per name; the threshold pre-pass over
// a few thousand rows must not dilute the main scan's average duration).
// QG = 16-query column groups per pass (1 or 2): every DB fragment feeds QG independent MFMA
// accumulator chains. The pass stays HBM-bound up to QG = 2 (f32 MFMA: 2 x 128 instructions of 32
// cycles per 32 KiB tile per SIMD = 16 B/clk/CU against ~10 B/clk/CU of HBM), and two chains hide
// the 40-cycle dependent-accumulator latency of a single one.
template <int E, bool PREPASS, int QG>
__global__ void __launch_bounds__(256) scan_topk_f32_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = E / 16;      // float4 per lane per 16-row tile
    constexpr int NCH = NT / 8;     // chunks of 8 float4
    if (a.run_if && *a.run_if == 0) return;       // fallback launch that is not needed (uniform)
    if (gridDim.y > 1) {                          // the coarse path's fallback: all query groups in one launch
        const int y = blockIdx.y, left = a.q_total - y * a.QA;
        a.q += (size_t)y * a.QA * E;
        a.cand += (size_t)y * a.QA * a.cap;
        a.gcnt += y * a.QA;
        if (a.thr_in) a.thr_in += y * a.QA;
        a.QA = left < a.QA ? left : a.QA;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nwaves = blockDim.x >> 6;
    const int col = lane & 15;      // query column of this lane inside a group (B operand / accumulator column)
    const int g = lane >> 4;        // MFMA k index supplied by this lane; accumulator row group

    // query image, one 1-KiB lane-linear piece per (group, t): entry [(qg*NT + t)*64 + lane] =
    // q[16*qg + col][16t+4g .. +3]
    f32x4* qimg = reinterpret_cast<f32x4*>(smem);
    for (int idx = tid; idx < QG * NT * 64; idx += blockDim.x) {
        const int l = idx & 63, t = (idx >> 6) % NT, qg = (idx >> 6) / NT;
        const int c_ = qg * 16 + (l & 15), g_ = l >> 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c_ < a.QA) v = *reinterpret_cast<const f32x4*>(a.q + (size_t)c_ * E + 16 * t + 4 * g_);
        qimg[idx] = v;
    }
    char* wbase = smem + QG * NT * 1024 + (size_t)wave * a.wave_bytes;
    uint2* buf = reinterpret_cast<uint2*>(wbase);            // [QA][C]
    uint2* scratch = buf + (size_t)a.QA * a.C;                // [C]
    int* cnt = reinterpret_cast<int*>(scratch + a.C);         // [32]
    float* thr = reinterpret_cast<float*>(cnt + 32);          // [32]
    if (lane < 32) {
        cnt[lane] = 0;
        thr[lane] = (lane < a.QA) ? (a.thr_in ? a.thr_in[lane] : -INFINITY) : INFINITY;
    }
    __syncthreads();

    bool active[QG];
    float tau[QG];
#pragma unroll
    for (int qg = 0; qg < QG; ++qg) {
        active[qg] = qg * 16 + col < a.QA;
        tau[qg] = thr[qg * 16 + col];
    }
    const int C = a.C, K = a.K;

    const long long ntiles = (a.nrows + 15) >> 4;
    const long long wg = (long long)blockIdx.x * nwaves + wave;
    const long long tw = (long long)gridDim.x * nwaves;
    const long long last_row = a.nrows - 1;

    long long tile = wg;
    if (tile < ntiles) {
        f32x4 T[NT];
        {
            long long r = tile * 16 + col;
            r = r > last_row ? last_row : r;
            const float* p = a.db + r * E + 4 * g;
#pragma unroll
            for (int t = 0; t < NT; ++t) T[t] = ld16_f<3>(p + 16 * t);
        }
        while (true) {
            const long long nxt = tile + tw;
            const bool has_next = nxt < ntiles;
            long long rn = (has_next ? nxt : tile) * 16 + col;
            rn = rn > last_row ? last_row : rn;
            const float* pn = a.db + rn * E + 4 * g;

            f32x4 acc[QG];
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) acc[qg] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int t = 8 * c + j;
                    f32x4 bq[QG];
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) bq[qg] = qimg[(qg * NT + t) * 64 + lane];
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].x, bq[qg].x, acc[qg], 0, 0, 0);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].y, bq[qg].y, acc[qg], 0, 0, 0);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].z, bq[qg].z, acc[qg], 0, 0, 0);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].w, bq[qg].w, acc[qg], 0, 0, 0);
                }
                // this chunk's registers are free: refill them with the next tile (stays in
                // flight across the candidate step below and the first chunks of the next pass).
                // The sched_barriers pin the refill HERE: left alone, hipcc sinks all refills
                // behind the tile's last MFMA and the wave then waits out the full HBM latency.
                // The empty asm consumes the chunk's last MFMA results and clobbers memory, so no
                // refill load can be hoisted above an MFMA that still reads the old registers
                // (which would cost a register copy behind a vmcnt(0) at the loop head).
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) asm volatile("" : "+a"(acc[qg]) : : "memory");
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int t = 8 * c + j;
                    T[t] = ld16_f<3>(pn + 16 * t);
                }
                __builtin_amdgcn_sched_barrier(0);
            }

            // accumulator qg: column = query 16*qg + col, rows = tile*16 + 4g + r
            const long long row0 = tile * 16 + 4 * g;
            bool any = false;
            bool pp[QG][4];
#pragma unroll
            for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pp[qg][r] = active[qg] && (row0 + r <= last_row) && (acc[qg][r] >= tau[qg]);
                    any |= pp[qg][r];
                }
            if (__ballot(any)) {
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) {
                    const int qi = qg * 16 + col;
                    uint2* qb = buf + (size_t)qi * C;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (pp[qg][r]) {
                            const int pos = atomicAdd(&cnt[qi], 1);
                            qb[pos] = make_uint2(__float_as_uint(acc[qg][r]), (unsigned)(row0 + r));
                        }
                }
                wave_lds_sync();
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) {
                    const bool need = active[qg] && (g == 0) && (cnt[qg * 16 + col] > C - 16);
                    unsigned long long mask = __ballot(need);
                    if (mask) {
                        while (mask) {
                            const int qq = qg * 16 + __builtin_ctzll(mask);
                            mask &= mask - 1;
                            wave_compact(buf + (size_t)qq * C, scratch, &cnt[qq], &thr[qq], K, lane);
                        }
                        tau[qg] = thr[qg * 16 + col];
                    }
                }
            }
            if (!has_next) break;
            tile = nxt;
        }
    }

    // publish the block's surviving candidates (unsorted, possibly more than K per wave): ONE
    // returning atomic per (block, query), issued by up to 32 lanes at once — per-wave serial atomics
    // here cost ~200 us of same-address contention at the end of a 1M-row scan
    __syncthreads();
    unsigned* gbase = reinterpret_cast<unsigned*>(smem);            // query image is dead now
    auto wave_cnt = [&](int w) {
        return reinterpret_cast<int*>(smem + QG * NT * 1024 + (size_t)w * a.wave_bytes + (size_t)(a.QA + 1) * a.C * 8);
    };
    if (wave == 0 && lane < a.QA) {
        unsigned total = 0;
        for (int w = 0; w < nwaves; ++w) total += (unsigned)wave_cnt(w)[lane];
        gbase[lane] = total ? atomicAdd(&a.gcnt[lane], total) : 0u;
    }
    __syncthreads();
    for (int qq = 0; qq < a.QA; ++qq) {
        const int n = cnt[qq];
        if (n == 0) continue;
        unsigned base = gbase[qq];
        for (int w = 0; w < wave; ++w) base += (unsigned)wave_cnt(w)[qq];
        uint2* dst = a.cand + (size_t)qq * a.cap + base;
        for (int e = lane; e < n; e += 64) dst[e] = buf[(size_t)qq * C + e];
    }
}

// Level 1 of the coarse path's pre-pass: exact scores of the first `nrows` rows (a few thousand) for up to 64 queries
// in ONE launch, written out unfiltered as candidate entries cand[q][row] = (score bits, row) for the radix select to
// take the K-th best of. Same MFMA sequence per (row, query) as scan_topk_f32_kernel (score order of this file's
// header). blockIdx.y picks 16 of the queries (a 32-KiB f32 image): the 25 MB of sample rows are read up to four times
// (from L2 after the first), and in exchange a workgroup fits on a CU - LDS and registers - beside a coarse scan
// workgroup of another batch in flight; with the 128-KiB image of all 64 queries this launch waited for that whole scan
// to drain, and its row tile + 16 accumulators spilled 252 B. A NaN score is stored as -inf.
// QG = 2 (the wide pass: up to 1024 queries): 32 queries per workgroup. With 16, every (row tile, query group) unit loaded its
// 32 KiB of rows for 128 MFMAs - 8 B per cycle and SIMD, the CU's whole L2 -> register rate - and the launch took 287 us for
// 83 us of f32 MFMA work at Q = 1024; 32 queries per row tile halve the loads per MFMA and give each
// wave two independent accumulator chains.
template <int E, int QG = 1>
__global__ void __launch_bounds__(256) sample_scores_kernel(const float* __restrict__ db, long long nrows,
                                                            const float* __restrict__ q, int QA, uint2* __restrict__ cand,
                                                            long long cap, unsigned* __restrict__ gcnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = E / 16;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, g = lane >> 4;
    const int qbase = blockIdx.y * 16 * QG;
    f32x4* qimg = reinterpret_cast<f32x4*>(smem);
    // QG*NT*64 = 2048 entries (E = 512; 3072 at E = 768) over 256 threads, 8 loads in flight per thread (one at a time cost
    // ~10 us per block). RAGGED: the image is not a whole number of 2048-entry rounds (E = 768), so the last round is bounded.
    constexpr int NIMG = QG * NT * 64;
    constexpr bool RAGGED = NIMG % (8 * 256) != 0;
    for (int base = tid; base < NIMG; base += 8 * 256) {
        f32x4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int idx = base + j * 256;
            const int l = idx & 63, t = (idx >> 6) % NT, qg = (idx >> 6) / NT;
            const int c_ = qbase + qg * 16 + (l & 15), g_ = l >> 4;
            v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (c_ < QA && (!RAGGED || idx < NIMG)) v[j] = *reinterpret_cast<const f32x4*>(q + (size_t)c_ * E + 16 * t + 4 * g_);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (!RAGGED || base + j * 256 < NIMG) qimg[base + j * 256] = v[j];
    }
    if (blockIdx.x == 0 && tid < 16 * QG && qbase + tid < QA) gcnt[qbase + tid] = (unsigned)nrows;
    __syncthreads();
    const long long ntiles = (nrows + 15) >> 4;
    const long long last_row = nrows - 1;
    for (long long tile = (long long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long long)gridDim.x * 4) {
        long long r = tile * 16 + col;
        r = r > last_row ? last_row : r;
        const float* p = db + r * E + 4 * g;
        f32x4 T[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) T[t] = *reinterpret_cast<const f32x4*>(p + 16 * t);
        // all 32 loads of the row tile are in flight before the first MFMA: left to itself the scheduler sank them into the
        // MFMA chain two at a time (vmcnt(1) after every load: 32 dependent L2 round trips per tile, ~16 us per tile against
        // 1.7 us of MFMA - round 4, hipcc -S)
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[QG];
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) acc[qg] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            f32x4 bq[QG];
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) bq[qg] = qimg[(qg * NT + t) * 64 + lane];
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].x, bq[qg].x, acc[qg], 0, 0, 0);
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].y, bq[qg].y, acc[qg], 0, 0, 0);
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].z, bq[qg].z, acc[qg], 0, 0, 0);
#pragma unroll
            for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(T[t].w, bq[qg].w, acc[qg], 0, 0, 0);
        }
        // accumulator qg: column = query 16*qg + col, rows = tile*16 + 4g + r_: a lane's four rows of one query are
        // 32 contiguous bytes of that query's list (two 16-byte stores; the four lane groups complete the 128-byte line)
#pragma unroll
        for (int qg = 0; qg < QG; ++qg) {
            const int qi = qbase + qg * 16 + col;
            const long long row = tile * 16 + 4 * g;
            unsigned sb[4];
#pragma unroll
            for (int r_ = 0; r_ < 4; ++r_) {
                const float sc = acc[qg][r_];
                sb[r_] = __float_as_uint(sc == sc ? sc : -INFINITY);
            }
            if (qi < QA) {
                uint2* dst = cand + (size_t)qi * cap + row;          // cap and row are multiples of 4: 32-byte aligned
                if (row + 3 <= last_row) {
                    *reinterpret_cast<uint4*>(dst) = make_uint4(sb[0], (unsigned)row, sb[1], (unsigned)row + 1);
                    *reinterpret_cast<uint4*>(dst + 2) = make_uint4(sb[2], (unsigned)row + 2, sb[3], (unsigned)row + 3);
                } else {
#pragma unroll
                    for (int r_ = 0; r_ < 4; ++r_)
                        if (row + r_ <= last_row) dst[r_] = make_uint2(sb[r_], (unsigned)(row + r_));
                }
            }
        }
    }
}

// Composite 64-bit key: larger = better under the ordering rule. High word = order-preserving
// image of the f32 score (-0 folded into +0), low word = ~id (smaller id wins ties). Keys of
// distinct rows are distinct, so "the K largest keys" is exactly the rule's top-K.
__device__ __forceinline__ unsigned long long ckey(uint2 c) {
    const float s = __uint_as_float(c.x) + 0.0f;
    unsigned u = __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(~c.y);
}

constexpr int SEL_THREADS = 512;
constexpr int SEL_STAGE = 12288;      // candidate entries a select block keeps in LDS (96 KiB); longer lists stream from L2
constexpr int SEL_FIXED = 32 * 8 + (256 + 8 + 8) * 4;
// large K leaves less room beside the K-entry result buffer; host (LDS size) and device (staging test) share this
__host__ __device__ constexpr int sel_stage_entries(int K, int limit = LDS_LIMIT) {
    return (limit - SEL_FIXED - K * 8) / 8 < SEL_STAGE ? ((limit - SEL_FIXED - K * 8) / 8 < 0 ? 0 : (limit - SEL_FIXED - K * 8) / 8)
                                                       : SEL_STAGE;
}

// One block per query: exact top-K of a dense, unsorted candidate list by MSB-first radix
// select on the composite key (8-bit digits, starting at the highest bit in which the list's
// keys differ), then a rank-count sort of the K survivors. All passes stream the list from
// global memory (it is L2-resident: a few thousand 8-byte entries) - unless it fits SEL_STAGE entries, in which case
// the block copies it into LDS once (loads batched four deep) and every pass runs out of LDS: the per-pass loop
// (load, LDS atomic, next load) otherwise pays one L2 round trip per 512 entries, ~17 us for a 7 k-entry list
// against ~5 us staged (seven selects per 64-query search).
struct SelectArgs {
    const uint2* cand;                  // [queries][cap] candidate lists, unsorted (keep: the K best go back to their heads)
    unsigned* gcnt;                     // entries used per query; left at 0 (keep & 1: at min(M, K)) for the call's next scan
    long long cap;
    int K;
    long long id_base = 0;              // added to the row ids written to out_i
    float* out_s = nullptr;             // [queries][K] scores and ids in rank order, padded with (-FLT_MAX, -1); null: no result
    long long* out_i = nullptr;
    float* thr_out = nullptr;           // [queries] the exact K-th best score (-inf with fewer than K entries), or null
    const unsigned* run_if = nullptr;   // optional device flag: the kernel exits at once when *run_if == 0
    unsigned* m_out = nullptr;          // [queries] list lengths, for the measurement hooks (keep & 2: added to what is there)
    int keep = 0;                       // bit 0: the K selected entries stay at the head of the list for the next segment
    int stage_cap = -1;                 // entries of LDS the launch reserved behind the K-entry result (-1: the most K leaves)
    float* qmeta = nullptr;             // coarse search ([4][qs], coarse_prep_kernel): the next scan's threshold goes to [2 qs]
    int qs = 64;                        // qmeta's stride
    int dense = 0;                      // the list is a sample's: entry e IS row e, only the 4 score bytes are staged
    unsigned* arm_fallback = nullptr;   // set to 1 when a query's margin in qmeta is +inf (no usable coarse bound)
};

__global__ void __launch_bounds__(SEL_THREADS) select_topk_kernel(SelectArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (a.run_if && *a.run_if == 0) return;
    // the sample's select of a coarse search: a query without a usable coarse bound (NaN / infinite component: its margin is +inf,
    // coarse_prep_kernel) arms the exact fallback for the call - the coarse lists canonicalise NaN scores to -inf, which only the
    // exact scan tells from a true -inf (the oracle never returns a NaN-scoring row). (Set here, not by coarse_prep_kernel: that
    // launch also CLEARS the flag.)
    if (a.arm_fallback && a.qmeta && threadIdx.x == 0 && a.qmeta[3 * a.qs + blockIdx.x] == INFINITY) *a.arm_fallback = 1u;
    unsigned long long* red = reinterpret_cast<unsigned long long*>(smem);   // [16] min, [16] max
    unsigned* hist = reinterpret_cast<unsigned*>(red + 32);                  // [256]
    unsigned* wsum = hist + 256;                                             // [8]
    unsigned* ctl = wsum + 8;                                                // [8] b, above, nsel
    const int K = a.K;
    uint2* sel = reinterpret_cast<uint2*>(ctl + 8);                          // [K]
    uint2* lent = sel + K;                                                   // [SEL_STAGE] staged copy of the list

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    long long M = a.gcnt[q];
    if (M > a.cap) M = a.cap;
    const uint2* src = a.cand + (size_t)q * a.cap;
    const int need = (int)(M < K ? M : K);
    // stage_cap: entries of LDS the launch reserved behind the K-entry result buffer (-1: the most K leaves room for)
    const bool staged = M <= (a.stage_cap < 0 ? sel_stage_entries(K) : a.stage_cap);
    // dense (the wide pass's sample lists: entry e IS row e - sample_scores_kernel writes cand[q][row] = (score, row)): only the
    // 4 score bytes of an entry are staged, the id is the index - 48 KiB instead of 96 for 12 288 rows, so three select blocks
    // fit on a CU instead of one (1024 of them per call of 1024 queries: 121 -> ~50 us)
    unsigned* const l32 = reinterpret_cast<unsigned*>(lent);
    if (staged && a.dense) {
        for (long long e0 = tid; e0 < M; e0 += 4 * SEL_THREADS) {
            unsigned v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = e0 + (long long)j * SEL_THREADS;
                v[j] = src[e < M ? e : M - 1].x;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = e0 + (long long)j * SEL_THREADS;
                if (e < M) l32[e] = v[j];
            }
        }
        __syncthreads();
    } else if (staged) {
        for (long long e0 = tid; e0 < M; e0 += 4 * SEL_THREADS) {
            uint2 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = e0 + (long long)j * SEL_THREADS;
                v[j] = src[e < M ? e : M - 1];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long e = e0 + (long long)j * SEL_THREADS;
                if (e < M) lent[e] = v[j];
            }
        }
        __syncthreads();
    }
    // the passes below exist twice, once per address space of the list (a pointer select would make every access a
    // flat load, each waiting on both counters in a loop that also holds LDS atomics: 54 us per select, measured)
    auto passes = [&](auto ent) {

        unsigned long long T = 0;     // select keys >= T
        if (M > K) {
            unsigned long long kmin = ~0ull, kmax = 0ull;
            for (long long e = tid; e < M; e += SEL_THREADS) {
                const unsigned long long k = ckey(ent(e));
                kmin = k < kmin ? k : kmin;
                kmax = k > kmax ? k : kmax;
            }
    #pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long lo = __shfl_xor(kmin, o), hi = __shfl_xor(kmax, o);
                kmin = lo < kmin ? lo : kmin;
                kmax = hi > kmax ? hi : kmax;
            }
            if (lane == 0) { red[wave] = kmin; red[16 + wave] = kmax; }
            __syncthreads();
            for (int w = 0; w < SEL_THREADS / 64; ++w) {
                kmin = red[w] < kmin ? red[w] : kmin;
                kmax = red[16 + w] > kmax ? red[16 + w] : kmax;
            }
            const unsigned long long diff = kmin ^ kmax;          // != 0: M >= 2 distinct keys
            int hi_shift = 64 - __builtin_clzll(diff);              // low bits not fixed yet, 1..64
            unsigned long long prefix = hi_shift >= 64 ? 0ull : ((kmax >> hi_shift) << hi_shift);
            unsigned r = (unsigned)K;                               // wanted: the r largest keys matching prefix
            while (hi_shift > 0) {
                const int w = hi_shift < 8 ? hi_shift : 8;
                const int shift = hi_shift - w;
                const unsigned dmask = (1u << w) - 1u;
                if (tid < 256) hist[tid] = 0;
                __syncthreads();
                for (long long e = tid; e < M; e += SEL_THREADS) {
                    const unsigned long long k = ckey(ent(e));
                    const bool match = hi_shift >= 64 || (k >> hi_shift) == (prefix >> hi_shift);
                    if (match) atomicAdd(&hist[(unsigned)(k >> shift) & dmask], 1u);
                }
                __syncthreads();
                // inclusive suffix sums S[t] = sum_{u >= t} hist[u] over 256 bins (waves 0..3)
                unsigned h = 0, S = 0;
                if (tid < 256) {
                    h = hist[tid];
                    S = h;
    #pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const unsigned v = __shfl_down(S, o);
                        if (lane + o < 64) S += v;
                    }
                    if (lane == 0) wsum[wave] = S;
                }
                __syncthreads();
                if (tid < 256) {
                    for (int w2 = wave + 1; w2 < 4; ++w2) S += wsum[w2];
                    const unsigned above = S - h;                    // count in bins > tid
                    if (S >= r && above < r) { ctl[0] = (unsigned)tid; ctl[1] = above; ctl[2] = h; }
                }
                __syncthreads();
                const unsigned b = ctl[0], above = ctl[1], cb = ctl[2];
                prefix |= (unsigned long long)b << shift;
                hi_shift = shift;
                r -= above;
                __syncthreads();
                if (cb == r) break;                                  // the whole bin is selected
            }
            T = prefix;
        }

        if (tid == 0) ctl[4] = 0;
        __syncthreads();
        for (long long e = tid; e < M; e += SEL_THREADS) {
            const uint2 c = ent(e);
            if (ckey(c) >= T) {
                const unsigned pos = atomicAdd(&ctl[4], 1u);
                if (pos < (unsigned)need) sel[pos] = c;
            }
        }
        __syncthreads();
        uint2* dst_keep = a.keep ? const_cast<uint2*>(src) : nullptr;     // every read of src is behind the barrier above
        for (int e = tid; e < need; e += SEL_THREADS) {
            const uint2 me = sel[e];
            const unsigned long long mk = ckey(me);
            int rank = 0;
            for (int j = 0; j < need; ++j) rank += ckey(sel[j]) > mk ? 1 : 0;
            if (dst_keep) dst_keep[rank] = me;
            if (a.out_s) {
                a.out_s[(size_t)q * K + rank] = __uint_as_float(me.x);
                a.out_i[(size_t)q * K + rank] = a.id_base + (long long)me.y;
            }
            if (a.thr_out && rank == K - 1) a.thr_out[q] = __uint_as_float(me.x);
            // coarse search: the next segment's scan threshold, (tau - margin) / t_q (coarse_prep_kernel's qmeta)
            // (an infinite margin - a non-finite query, coarse_prep_kernel - means "no threshold", not inf - inf)
            if (a.qmeta && rank == K - 1)
                a.qmeta[2 * a.qs + q] = a.qmeta[3 * a.qs + q] == INFINITY ? -INFINITY : (__uint_as_float(me.x) - a.qmeta[3 * a.qs + q]) * a.qmeta[q];
        }
        if (a.out_s)
            for (int e = need + tid; e < K; e += SEL_THREADS) {
                a.out_s[(size_t)q * K + e] = -FLT_MAX;
                a.out_i[(size_t)q * K + e] = -1;
            }
        if (a.thr_out && need < K && tid == 0) a.thr_out[q] = -INFINITY;
        if (a.qmeta && need < K && tid == 0) a.qmeta[2 * a.qs + q] = -INFINITY;
    };
    if (staged && a.dense) passes([&](long long e) -> uint2 { return make_uint2(l32[e], (unsigned)e); });
    else if (staged) passes([&](long long e) -> uint2 { return lent[e]; });
    else passes([&](long long e) -> uint2 { return src[e]; });
    // leave the counter zeroed for the next scan of this call (every thread read M at entry; the
    // barriers above order that read before this store) — saves a memset node per scan
    // keep = 1 (segmented coarse scan): the K selected entries stay at the head of the list and the next segment's
    // survivors are appended behind them; keep bit 1: add to the measurement counter instead of overwriting it
    if (tid == 0) {
        a.gcnt[q] = a.keep & 1 ? (unsigned)need : 0u;
        if (a.m_out) a.m_out[q] = (a.keep & 2 ? a.m_out[q] : 0u) + (unsigned)M;       // list length(s), for measurement hooks
    }
}

__global__ void fill_empty_kernel(float* out_s, long long* out_i, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out_s[i] = -FLT_MAX; out_i[i] = -1; }
}

// Cross-rank merge: R lists of K (score f32, id i64; id < 0 = empty) per query, rank counting
// straight from LDS. One block per query.
__global__ void __launch_bounds__(256) merge_lists_i64_kernel(const float* __restrict__ scores, const long long* __restrict__ ids,
                                                              long long rstride_s, long long rstride_i,
                                                              int R, int Q, int K, float* out_s, long long* out_i) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = R * K;
    long long* sid = reinterpret_cast<long long*>(smem);          // [n]
    float* ss = reinterpret_cast<float*>(sid + n);                 // [n]
    int* nvalid = reinterpret_cast<int*>(ss + n);
    if (tid == 0) *nvalid = 0;
    __syncthreads();
    int myvalid = 0;
    for (int e = tid; e < n; e += blockDim.x) {
        const int r = e / K, k = e - r * K;
        const size_t src = (size_t)q * K + k;
        const long long id = ids[(size_t)r * rstride_i + src];
        const float s = scores[(size_t)r * rstride_s + src];
        const bool ok = id >= 0 && s == s;
        sid[e] = ok ? id : -1;
        ss[e] = s;
        myvalid += ok ? 1 : 0;
    }
    atomicAdd(nvalid, myvalid);
    __syncthreads();
    for (int e = tid; e < n; e += blockDim.x) {
        const long long mi = sid[e];
        if (mi < 0) continue;
        const float ms = ss[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const long long oi = sid[j];
            const float os = ss[j];
            rank += (oi >= 0 && (os > ms || (os == ms && oi < mi))) ? 1 : 0;
        }
        if (rank < K) {
            out_s[(size_t)q * K + rank] = ms;
            out_i[(size_t)q * K + rank] = mi;
        }
    }
    const int nv = *nvalid;
    for (int e = (nv < K ? nv : K) + tid; e < K; e += blockDim.x) {
        out_s[(size_t)q * K + e] = -FLT_MAX;
        out_i[(size_t)q * K + e] = -1;
    }
}

// =================================================================================================
// Coarse-then-exact path (SURVEY.md §7 option (b)): a bf16 copy of the matrix is scanned with bf16
// MFMA (half the HBM bytes, 64 queries per pass) keeping a PROVABLE SUPERSET of the exact top-K; the
// survivors are re-scored in exact f32 with the same fmaf order as the exact kernel and selected by the
// same radix select, so results stay bit-exact against the oracle.
//
// Superset argument. Let s(r) be the exact (fmaf-chain) score of row r and c(r) the bf16-MFMA score of
// the bf16-rounded operands. bf16 RNE has relative error u = 2^-9 per operand, so the exact products
// differ by at most (2u + u^2)|a_k b_k|; both accumulations (f32, E terms, any order) add at most
// ~2 * E * 2^-24 * sum|a_k b_k|. With sum|a_k b_k| <= ||row|| ||q||, at E = 512:
//        |c(r) - s(r)| <= 0.004 * ||row|| * ||q||  <=  margin_q := 0.0041 * R_max * ||q||
// (R_max = largest row norm, kept with the bf16 copy). E = 768: 0.0040017 and 0.0041305, bf16_margin_coef<E> below. tau0_q = exact K-th best of the first S rows is
// a lower bound of the final K-th best score; every row of the true top-K has s >= tau0_q, hence
// c >= tau0_q - margin_q =: the coarse threshold. If a candidate list overflows its capacity a device
// flag makes the (otherwise early-exiting) exact-scan fallback launches run and overwrite the result.
// =================================================================================================
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2v __attribute__((ext_vector_type(2)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack2_bf16(float a, float b) {
    f32x2v v = {a, b};
    bf16x2v r = __builtin_convertvector(v, bf16x2v);
    return __builtin_bit_cast(unsigned, r);
}

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
__global__ void __launch_bounds__(256) quantize_rows_i8_kernel(const float* __restrict__ db, long long N, int E,
                                                               const unsigned* __restrict__ perm,
                                                               signed char* __restrict__ out, float2* __restrict__ meta,
                                                               float2* __restrict__ bmeta, unsigned* __restrict__ slot_rows) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long blk = blockIdx.x, r0 = blk * 32;
    float mx = 0.f;
    for (int i = 0; i < 8; ++i) {
        const long long t = r0 + wave * 8 + i;                     // slot
        const long long r = t < N ? (perm ? (long long)perm[t] : t) : N;
        if (r < N)
            for (int k = lane * 4; k < E; k += 256) {
                const float4 v = *reinterpret_cast<const float4*>(db + (size_t)r * E + k);
                mx = fmaxf(fmaxf(mx, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
            }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = mx > 0.f ? mx / 127.0f : 1.0f;
    const float inv = 1.0f / s;
    signed char* oblk = out + (size_t)blk * 32 * E;
    float amax_w = 0.f;
    for (int i = 0; i < 8; ++i) {
        const int rloc = wave * 8 + i;
        const long long t = r0 + rloc;                             // slot
        const long long r = t < N ? (perm ? (long long)perm[t] : t) : N;
        float ee = 0.f;
        for (int k = lane * 4; k < E; k += 256) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < N) v = *reinterpret_cast<const float4*>(db + (size_t)r * E + k);
            float qv[4] = {rintf(v.x * inv), rintf(v.y * inv), rintf(v.z * inv), rintf(v.w * inv)};
            const float xv[4] = {v.x, v.y, v.z, v.w};
            unsigned pk = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                qv[j] = fminf(fmaxf(qv[j], -127.f), 127.f);
                const float e = xv[j] - s * qv[j];
                ee = fmaf(e, e, ee);
                pk |= ((unsigned)(int)qv[j] & 0xffu) << (8 * j);
            }
            const int ks = k >> 5, h = (k >> 4) & 1, b = k & 15;
            *reinterpret_cast<unsigned*>(oblk + (size_t)ks * 1024 + (h * 32 + rloc) * 16 + b) = pk;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ee += __shfl_xor(ee, o);
        const float a_r = r < N ? sqrtf(ee) * 1.001f : 0.f;
        if (lane == 0) {
            meta[t] = make_float2(s, a_r);
            slot_rows[t] = r < N ? (unsigned)r : 0xffffffffu;
        }
        amax_w = fmaxf(amax_w, a_r);
    }
    if (lane == 0) red[4 + wave] = amax_w;
    __syncthreads();
    if (tid == 0) bmeta[blk] = make_float2(s, fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7])));
}

// Per-query constants of a coarse search, once per group of <= qs queries (one wave per query), qmeta [4][qs]
// (qs = 64 for the 64-query passes, the padded query count of a wide pass):
//   [0]    1 / t_q (int8; t_q = max|y| / 127)            or 1 (bf16)
//   [qs]   1.001 ||y|| / t_q (int8)                       or 0
//   [2 qs] the value the scan compares against, (tau - margin) * [0] - written by select_topk_kernel each time a new exact
//          K-th best tau is known (-inf until then)
//   [3 qs] margin: 1.001 (R_max + A_max) ||f_q|| + 1e-4 R_max ||y|| (int8, f_q = y - t_q p_q) or 1.001 * 0.0041 R_max ||q||
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
//   * the norms ||y||, ||f_q||, a_r are sums of E squares in f32 (relative error < (E + 2) u / 2 each after the root):
//     covered by their own 1.001 factors (1e-3 against < 2.3e-5).
// Needed: (2 E + 16) u = 6.2e-5 at E = 512, 9.3e-5 at E = 768. The constant is 1e-4 * E / 512: 1e-4 at 512 (unchanged, bit for
// bit), 1.5e-4 at 768 - the same 1.6 x head room at both widths instead of 1.08 x; it is < 1 % of the query half of the margin
// (1.001 (R + A) ||f_q|| ~ 7.6e-3 R ||y|| on unit data), so the survivor count does not notice.
// bf16: |c - s| <= (2 u9 + u9^2 + 2 E u) ||x|| ||y||, u9 = 2^-9: 0.0039712 at 512, 0.0040017 at 768 (no longer below the
// 0.004 the header's argument rounds to). The constant is 0.0041 + 2 (E - 512) u: 0.0041 at 512 (unchanged), 0.0041305 at 768 -
// the same 1.3e-4 of head room at both widths.
template <int E>
constexpr float i8_round_slack() { return 1e-4f * ((float)E / 512.0f); }
template <int E>
constexpr float bf16_margin_coef() { return 0.0041f + 2.0f * (float)(E - 512) * 5.9604644775390625e-8f; }
static_assert(i8_round_slack<512>() == 1e-4f && bf16_margin_coef<512>() == 0.0041f, "E = 512 keeps its constants bit for bit");
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
    float mx = 0.f, ss = 0.f;
    for (int k = lane; k < E; k += 64) { const float v = y[k]; mx = fmaxf(mx, fabsf(v)); ss = fmaf(v, v, ss); }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); ss += __shfl_xor(ss, o); }
    const float t = mx > 0.f ? mx / 127.0f : 1.0f;
    const float inv = I8 ? 1.0f / t : 1.0f;
    // the int8 digit of component v; the query images below use the same expression
    auto digit = [&](float v) -> float { return fminf(fmaxf(rintf(v * inv), -127.f), 127.f); };
    float ff = 0.f;
    if (I8) {
        for (int k = lane; k < E; k += 64) {
            const float f = fmaf(-t, digit(y[k]), y[k]);       // what the digit leaves: f_q
            ff = fmaf(f, f, ff);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ff += __shfl_xor(ff, o);
    }
    if (lane == 0) {
        const float Y = sqrtf(ss), F = sqrtf(ff) * 1.001f;
        float margin = I8 ? 1.001f * (rmax + amax) * F + i8_round_slack<ET>() * rmax * Y : bf16_margin_coef<ET>() * rmax * Y * 1.001f;
        // A query with a NaN or infinite component has no usable coarse bound: its margin is +inf, which the selects turn into a
        // threshold of -inf whatever the K-th best is (inf - inf would be a NaN that passes nothing) - every row then passes, the
        // lists overflow and the exact fallback answers the call, as the contract promises for any data. The other two
        // constants stay finite so that the scans' left-hand sides do (round 5: an infinite component used to give inv = 0 and
        // Y inv = NaN, and such a query came back empty - test_non_finite_queries_through_the_permuted_int8_copy).
        const bool finite_q = fabsf(Y) < INFINITY && fabsf(mx) < INFINITY && fabsf(margin) < INFINITY;      // false for NaN too
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
constexpr size_t RESCORE16_LDS = 512 * 4 + 4 * 16 * 68 * 4;      // rescore_pairs16_kernel (E = 512 only: the wide passes): the query + four waves' tiles of 16 row chunks

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

// publish a wave's n pending pairs: one global atomic per pair (rare path: ~1 pair in 10^4 passes the threshold)
__device__ __noinline__ void coarse_flush(const uint2* list, int n, unsigned* gcnt, uint2* cand, long long cap, unsigned* overflow) {
    const int lane = threadIdx.x & 63;
    wave_lds_sync();
    for (int e = lane; e < n; e += 64) {
        const uint2 c = list[e];
        const unsigned pos = atomicAdd(&gcnt[c.x], 1u);
        if ((long long)pos < cap) cand[(size_t)c.x * cap + pos] = make_uint2(CAND_SLOT, c.y);
        else *overflow = 1u;
    }
    wave_lds_sync();
}

// PREPASS only changes the kernel's NAME (the level-2 pre-pass over S2 rows must not dilute the profiler's
// per-name average of the main scan).
// 16 bytes of the streamed coarse copy (CLIPMI_NT_MASK bit 0: non-temporal)
__device__ __forceinline__ uint4 ld_stream(const char* p) {
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    if constexpr (CLIPMI_NT_MASK & 1) {
        const u4v v = __builtin_nontemporal_load(reinterpret_cast<const u4v*>(p));
        return make_uint4(v[0], v[1], v[2], v[3]);
    } else
        return *reinterpret_cast<const uint4*>(p);
}

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
    // of f32 queries and quantise them again); here it is a 16-byte-per-lane copy, 8 loads in flight
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
                                const int pos = npend + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                                // <= 256 appends per block behind at most COARSE_FLUSH pending: inside the list (static_assert above)
                                if (p[r]) list[pos] = make_uint2((unsigned)(qg * 16 + col), (unsigned)(step * 32 + rt * 16 + 4 * g + r));
                                npend += __builtin_popcountll(m);
                            }
                        }
                        if (npend > COARSE_FLUSH) {
                            coarse_flush(list, npend, a.gcnt, a.cand, a.cap, a.overflow);
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
    // final publication, aggregated per BLOCK: one returning global atomic per (block, query) issued by
    // 64 lanes at once, then entries scatter to base + an LDS-counted offset. (Per-entry global atomics
    // here meant ~166 k same-address atomics at the end of every scan: ~250 us fixed, as much as
    // streaming 1.25 M rows.)
    __syncthreads();
    constexpr int QMAXC = 16 * QG;                                   // <= blockDim.x for every launch shape
    unsigned* hist = reinterpret_cast<unsigned*>(smem);              // query image is dead now: [QMAXC] counts
    unsigned* gbase = hist + QMAXC;                                  // global base per query
    unsigned* hoff = hist + 2 * QMAXC;                               // running offsets
    if (tid < QMAXC) { hist[tid] = 0; hoff[tid] = 0; }
    __syncthreads();
    const int n_mine = npend;
    for (int e = lane; e < n_mine; e += 64) atomicAdd(&hist[list[e].x], 1u);
    __syncthreads();
    if (tid < QMAXC) gbase[tid] = hist[tid] ? atomicAdd(&a.gcnt[tid], hist[tid]) : 0u;
    __syncthreads();
    for (int e = lane; e < n_mine; e += 64) {
        const uint2 c = list[e];
        const unsigned pos = gbase[c.x] + atomicAdd(&hoff[c.x], 1u);
        if ((long long)pos < a.cap) a.cand[(size_t)c.x * a.cap + pos] = make_uint2(CAND_SLOT, c.y);
        else *a.overflow = 1u;
    }
}

// Exact f32 re-scoring of the coarse survivors: (exact score bits, row id) for every entry of the candidate lists. A lane that
// owns a (query, row) pair runs the SAME fmaf chain as the MFMA scan (t, c, g order) - one serial chain over the row's E
// components, so the score bits equal the exact kernel's and the oracle's; that chain is why a row cannot be split over lanes and
// the rows go through a per-wave LDS tile: fetched COOPERATIVELY (4 rows x 256 B contiguous per wave-instruction), read back by
// the owning lane. (A first version with one thread fetching its own 2-KB row: ~1 ms for 175 k pairs, 4 uncoalesced loads in flight.)
//
// Two forms. rescore_pairs16_kernel (round 4, the wide passes' lists: up to 1 024 queries x ~500 pairs): a wave takes SIXTEEN pairs
// and issues all 32 loads of their whole rows (32 KB in flight per wave) before it touches the first chunk - one HBM round trip
// per batch, 19 KB of LDS per block, three waves per SIMD; the compute runs on lanes 0-15's rows four times over (lanes l and
// l + 16 k read the same LDS words: broadcasts), 4 x the issue slots per pair and still far below the gathers' time. One call of
// 1 024 queries at 10 M rows: 6.26 -> 6.08-6.12 ms (same box). rescore_pairs_kernel (below): 64 pairs per wave in 8 chunks, kept
// for the 64-query passes, where the two gather at the same rate and this one costs the other call in flight less.
template <int E>
__global__ void __launch_bounds__(256) rescore_pairs16_kernel(const float* __restrict__ db, const float* __restrict__ q,
                                                            uint2* cand, const unsigned* __restrict__ gcnt, long long cap,
                                                            const unsigned* __restrict__ slot_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RS = 68;                                  // floats per staged row chunk (64 + 4 pad: conflict-free b128 reads)
    constexpr int NCH = E / 64;                             // 256-byte chunks per row
    float* qs = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* st = qs + E + wave * 16 * RS;
    const int qi = blockIdx.y;
    for (int k = threadIdx.x; k < E; k += 256) qs[k] = q[(size_t)qi * E + k];
    __syncthreads();
    long long M = gcnt[qi];
    if (M > cap) M = cap;
    uint2* lst = cand + (size_t)qi * cap;
    const int r16 = lane & 15, j4 = lane >> 4;
    for (long long base = ((long long)blockIdx.x * 4 + wave) * 16; base < M; base += (long long)gridDim.x * 4 * 16) {
        const long long my = base + r16;
        const uint2 ent = lst[my < M ? my : M - 1];
        // a fresh survivor names a SLOT of the (permuted) int8 copy: its row id comes from slot_rows (one more dependent read,
        // for survivors only); entries kept from earlier segments are row ids already
        const unsigned id_my = (ent.x == CAND_SLOT && slot_rows) ? slot_rows[ent.y] : ent.y;
        f32x4 nx[4][NCH];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned rid = __shfl(id_my, 4 * i + j4);
            const float* rowp = db + (size_t)rid * E + r16 * 4;
#pragma unroll
            for (int c = 0; c < NCH; ++c) nx[i][c] = ld16_f<2>(rowp + c * 64);
        }
        float acc = 0.f;
#pragma unroll
        for (int chunk = 0; chunk < NCH; ++chunk) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(st + (4 * i + j4) * RS + r16 * 4) = nx[i][chunk];
            wave_lds_sync();
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                f32x4 v[4];
#pragma unroll
                for (int g_ = 0; g_ < 4; ++g_) v[g_] = *reinterpret_cast<const f32x4*>(st + r16 * RS + 16 * tt + 4 * g_);
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int g_ = 0; g_ < 4; ++g_)
                        acc = __builtin_fmaf(v[g_][c], qs[64 * chunk + 16 * tt + 4 * g_ + c], acc);
                // pin the chain here: with the chunk loop unrolled the compiler sinks all 512 fmaf below the last chunk (acc
                // is only used at the end) and keeps every chunk's LDS reads alive - 512 registers + 550 spilled to scratch
                asm volatile("" : "+v"(acc) :: "memory");
            }
            wave_lds_sync();
        }
        if (j4 == 0 && my < M) lst[my] = make_uint2(__float_as_uint(acc == acc ? acc : -INFINITY), id_my);      // NaN never ranks
    }
}

// The 64-query passes' form (rounds 2-3): 64 pairs per wave, 8 chunks of 16 loads with one chunk of prefetch. Same-box A/B
// (CLIPMI_RESCORE=16 / 64, development library; profiles/r04_search_rescore_ab.txt): its lists (2 500 / 1 500 / 700 pairs per
// query) are gathered at the same ~5 TB/s by either form - 58.6 / 41.6 / 29.3 us against 58.1 / 47.8 / 27.2 at 10 M rows - and
// with two calls in flight this one disturbs the other call's streaming scan less (0.976 against 1.005 ms per call).
constexpr size_t rescore_lds(int E) { return (size_t)E * 4 + 4 * 64 * 68 * 4; }      // the query + four waves' tiles of 64 row chunks
constexpr size_t RESCORE_LDS = rescore_lds(512);
template <int E>
__global__ void __launch_bounds__(256) rescore_pairs_kernel(const float* __restrict__ db, const float* __restrict__ q,
                                                            uint2* cand, const unsigned* __restrict__ gcnt, long long cap,
                                                            const unsigned* __restrict__ slot_rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RS = 68;                                  // floats per staged row chunk (64 + 4 pad: conflict-free b128 reads)
    float* qs = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* st = qs + E + wave * 64 * RS;
    const int qi = blockIdx.y;
    for (int k = threadIdx.x; k < E; k += 256) qs[k] = q[(size_t)qi * E + k];
    __syncthreads();
    long long M = gcnt[qi];
    if (M > cap) M = cap;
    uint2* lst = cand + (size_t)qi * cap;
    for (long long base = ((long long)blockIdx.x * 4 + wave) * 64; base < M; base += (long long)gridDim.x * 4 * 64) {
        const long long my = base + lane;
        const uint2 ent = lst[my < M ? my : M - 1];
        // a fresh survivor names a SLOT of the (permuted) int8 copy: its row id comes from slot_rows (one more dependent read,
        // for survivors only); entries kept from earlier segments are row ids already
        const unsigned id_my = (ent.x == CAND_SLOT && slot_rows) ? slot_rows[ent.y] : ent.y;
        float acc = 0.f;
        // chunk c+1's 16 loads are issued (to registers) before chunk c is consumed from LDS: one
        // HBM round trip per chunk stays, but it overlaps the previous chunk's LDS reads and fmaf chain
        f32x4 nx[16];
        const float* rowp[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned rid = __shfl(id_my, 4 * i + (lane >> 4));
            rowp[i] = db + (size_t)rid * E + (lane & 15) * 4;
            nx[i] = ld16_f<2>(rowp[i]);
        }
        for (int chunk = 0; chunk < E / 64; ++chunk) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                *reinterpret_cast<f32x4*>(st + (4 * i + (lane >> 4)) * RS + (lane & 15) * 4) = nx[i];
            if (chunk + 1 < E / 64) {
#pragma unroll
                for (int i = 0; i < 16; ++i) nx[i] = ld16_f<2>(rowp[i] + (chunk + 1) * 64);
            }
            wave_lds_sync();
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                f32x4 v[4];
#pragma unroll
                for (int g_ = 0; g_ < 4; ++g_) v[g_] = *reinterpret_cast<const f32x4*>(st + lane * RS + 16 * tt + 4 * g_);
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int g_ = 0; g_ < 4; ++g_)
                        acc = __builtin_fmaf(v[g_][c], qs[64 * chunk + 16 * tt + 4 * g_ + c], acc);
            }
            wave_lds_sync();
        }
        if (my < M) lst[my] = make_uint2(__float_as_uint(acc == acc ? acc : -INFINITY), id_my);      // NaN never ranks
    }
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
// meta of the int8 copy: row entries for N rounded up to 32 rows (+32), then one (scale, largest error norm) pair per block (+1)
inline size_t i8_row_meta_entries(int64_t N) { return (size_t)((N + 31) / 32 * 32 + 32); }
inline size_t i8_block_meta_entries(int64_t N) { return (size_t)((N + 31) / 32 + 1); }
// ... and behind the block meta one u32 per slot: the row it holds (quantize_rows_i8_kernel)
inline const unsigned* i8_slot_rows(const float2* rmeta, int64_t N) {
    return reinterpret_cast<const unsigned*>(rmeta + i8_row_meta_entries(N) + i8_block_meta_entries(N));
}

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

__device__ __noinline__ void wide_flush(const uint2* list, int n, int qbase, unsigned* gcnt, uint2* cand, long long cap,
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

    // workgroup -> (query tile, row lane): blocks b, b + 8, ... share an XCD (observed dispatch; speed only)
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3, jb = gridDim.x >> 3;
    const int rlx = jb / a.nqt;                               // row lanes per XCD label
    if (j >= rlx * a.nqt) return;
    const int qt = j % a.nqt, nrl = rlx * 8;
    const int rl = a.map_mode == 1 ? x * rlx + (j / a.nqt) : (j / a.nqt) * 8 + x;
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
        // rows are loaded as buffer loads: scalar resource (rebased per block, so 32-bit offsets suffice for any copy size),
        // ONE lane-offset register, scalar k-step offsets - 64-bit per-lane addresses cost 26 registers here
        const unsigned lane16 = (unsigned)lane * 16u;
        auto load_block = [&](int b_, uint4 (&dst)[KS]) {
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<signed char*>(a.dbc) + (size_t)b_ * BLOCK_BYTES, 0, BLOCK_BYTES, 0x00020000);
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
            // The exact test of a (row, query) pair is  D s + a_r Y_q >= T_q  (T_q = (tau - margin) / t_q, Y_q = 1.001 ||y|| / t_q;
            // s the block's scale). Integer pre-test, one per lane (= query): no row of the block can pass unless
            // D >= (T_q - amax_block Y_q) / s, rounded down with slack for the f32 roundings on both sides (|D| <= 32 KS 127^2
            // < 2^24 is exact in f32: 8.3e6 at 512, 1.24e7 at 768 - static_assert above) - so the lane's largest D decides, and the
            // per-row test runs only where it can succeed.
            // The slack, for |x| up to 1.3e7 (u = 2^-24): a row passes when fl(D s + fl(a Y)) >= T, i.e. D >= x* - u (|T| + a Y) / s
            // with x* = (T - a Y) / s in real numbers. a / s <= 1.001 sqrt(E) / 2 (half a step per component) and Y <= 1.001 * 127
            // sqrt(E), so a Y / s <= 4.9e4 at E = 768 and |T| / s <= |x*| + 4.9e4: D >= x* - u |x*| - 0.006. The computed
            // xq = fl(fl(T - a Y) fl(1 / s)) has three roundings: |xq - x*| <= 3.0001 u |x*|. The two subtractions below round to
            // half a unit each while |xq| < 2^24 (to u |xq| beyond). Needed: 1.006 + 4.1 u |x| = 1.006 + 2.5e-7 |x| (4.2 at
            // |x| = 1.3e7); taken: 2 + 2e-6 |x| (28 there) - the constants of the 512 form, which needed 1.004 + 2.5e-7 |x|, hold
            // at 768 unchanged. Past 2^24 no D exists: x* > 1.3e7 passes nothing and x* < -1.3e7 everything, and the relative
            // slack (2e-6 against 6 u) keeps dmin on the right side of every possible D.
            // +inf thresholds (padding queries: any Q that is not a multiple of 32) are "never" by
            // an explicit test - inf - inf below would be NaN = "always", and every block would then run the 16-ballot append
            // path for its padding lanes; an all-zero block (s = 0: inv_s = inf) clamps to +-1e9 by its sign;
            // -inf (no threshold yet) and NaN stay "always".
            auto pretest = [&](const i32x16& acc, float tq, float yq) -> bool {
                if (tq == INFINITY) return false;
                float xq = fmaf(-bm.y, yq, tq) * inv_s;
                xq = fminf(fmaxf(xq, -1.0e9f), 1.0e9f);                   // before the slack: no inf - inf; fmaxf(NaN, c) = c: NaN -> always
                xq = xq - 2.0f - fabsf(xq) * 2e-6f;
                const int dmin = (int)floorf(xq);
                auto max3 = [](int a_, int b_, int c_) { const int m_ = a_ > b_ ? a_ : b_; return m_ > c_ ? m_ : c_; };
                const int m0 = max3(acc[0], acc[1], acc[2]), m1 = max3(acc[3], acc[4], acc[5]), m2 = max3(acc[6], acc[7], acc[8]);
                const int m3 = max3(acc[9], acc[10], acc[11]), m4 = max3(acc[12], acc[13], acc[14]);
                const int ma = max3(m0, m1, m2), mb = max3(m3, m4, acc[15]);              // three levels, not a chain of eight
                return (ma > mb ? ma : mb) >= dmin;
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
                        const int pos = npend + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                                          __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                        if (pass) list[pos] = make_uint2((unsigned)(G * 32 + n), row);
                        npend += __builtin_popcountll(m);
                    }
                    if ((i & 3) == 3 && npend > WIDE_FLUSH) {              // <= 256 appends between two tests
                        wide_flush(list, npend, qbase, a.gcnt, a.cand, a.cap, a.overflow);
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
    // final publication, aggregated per block (one returning global atomic per (block, query))
    __syncthreads();
    constexpr int QMAXC = 64 * WIDE_TILE_SETS;
    unsigned* hist = reinterpret_cast<unsigned*>(smem);              // the image is dead now
    unsigned* gbase = hist + QMAXC;
    unsigned* hoff = hist + 2 * QMAXC;
    for (int i = tid; i < QMAXC; i += WAVES * 64) { hist[i] = 0; hoff[i] = 0; }
    __syncthreads();
    for (int e = lane; e < npend; e += 64) atomicAdd(&hist[list[e].x], 1u);
    __syncthreads();
    for (int i = tid; i < QMAXC; i += WAVES * 64) gbase[i] = hist[i] ? atomicAdd(&a.gcnt[qbase + i], hist[i]) : 0u;
    __syncthreads();
    for (int e = lane; e < npend; e += 64) {
        const uint2 c = list[e];
        const unsigned pos = gbase[c.x] + atomicAdd(&hoff[c.x], 1u);
        if ((long long)pos < a.cap) a.cand[(size_t)(qbase + c.x) * a.cap + pos] = make_uint2(CAND_SLOT, c.y);
        else *a.overflow = 1u;
    }
}

struct Plan {
    int C, waves, QA, QG, grid, grid_sample, wave_bytes, stage, E;
    size_t lds_scan, lds_sel;
    long long NL, NL_sample, cap, sample_rows;
    bool sample;
};

// Shared by workspace sizing and launch so both always agree.
// lds_limit: what a workgroup of the exact scan or a select may take (the coarse path asks for COARSE_SIDE_LDS so its
// side kernels fit on a CU beside a coarse scan workgroup of another batch in flight)
bool make_plan(long long N, int E, int Q, int K, Plan& p, int lds_limit = LDS_LIMIT) {
    if (N < 0 || Q < 1 || K < 1 || (E != 512 && E != 768)) return false;
    p.E = E;
    p.C = (int)align_up((size_t)K + 16, 16);
    p.waves = 0;
    // prefer 4 waves per block and as many queries per pass as LDS allows (32, else 16, else fewer)
    for (int w = 4; w >= 1 && p.waves == 0; w >>= 1)
        for (int qg = (Q > 16 ? 2 : 1); qg >= 1; --qg) {
            const int qimg = qg * (E / 16) * 1024;
            const long long per_wave = (lds_limit - qimg) / w - 256;
            const long long fit = per_wave / ((long long)p.C * 8) - 1;     // queries that fit beside scratch
            const int qwant = Q < 16 * qg ? Q : 16 * qg;
            if (fit >= qwant || (qg == 1 && fit >= 1)) {
                p.waves = w; p.QG = qg; p.QA = (int)(fit < qwant ? fit : qwant);
                break;
            }
        }
    if (p.waves == 0) return false;
    if (SEL_FIXED + (long long)K * 8 > lds_limit) return false;
    p.stage = sel_stage_entries(K, lds_limit);
    p.lds_sel = SEL_FIXED + (size_t)K * 8 + (size_t)p.stage * 8;
    if (p.lds_sel > (size_t)lds_limit) return false;
    const int qimg = p.QG * (E / 16) * 1024;
    p.wave_bytes = (p.QA + 1) * p.C * 8 + 256;
    p.lds_scan = (size_t)qimg + (size_t)p.waves * p.wave_bytes;
    const long long ntiles = (N + 15) / 16;
    long long grid = (ntiles + p.waves - 1) / p.waves;
    if (grid > NUM_CU) grid = NUM_CU;            // one block per CU: the ring keeps ~100 KB in flight per CU
    if (grid < 1) grid = 1;
    p.grid = (int)grid;
    p.NL = grid * p.waves;
    // threshold pre-pass over the first S rows: S ~ sqrt(N*K) balances the two select passes
    p.sample = N >= SAMPLE_MIN_N;
    long long S = 4096;
    while (S < 65536 && S * S < N * (long long)K) S *= 2;
    p.sample_rows = S;
    p.grid_sample = (int)((S / 16 + p.waves - 1) / p.waves);
    p.NL_sample = (long long)p.grid_sample * p.waves;
    const long long nl = p.NL > p.NL_sample ? p.NL : p.NL_sample;
    p.cap = nl * p.C;
    // a scan appends every (query, row) pair at most once and compaction only drops entries: the waves of one launch never
    // publish more than `rows` entries per query, and the lists are dense (one running counter per query). Without this bound a
    // large K on a small index sized the lists by the pre-pass's many one-tile waves: 2048 x 8144 entries = 133 MB per query
    // at K = 8128 for 70 k rows, 8.5 GB for the 64 lists of a coarse search's fallback.
    // (the pre-pass only runs with N >= SAMPLE_MIN_N >= S rows, so N bounds both launches)
    const long long rows = (long long)align_up((size_t)(N > 0 ? N : 1), 16);
    if (p.cap > rows) p.cap = rows;
    return true;
}

// the largest K make_plan accepts at row width E (it depends on nothing else: the last plan tried is one wave, one query)
int max_k(int E) {
    Plan p;
    int lo = 0, hi = 1 << 20;                    // make_plan(lo) holds or lo = 0; make_plan(hi) fails
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        (make_plan(1, E, 1, mid, p) ? lo : hi) = mid;
    }
    return lo;
}

int opt_in_lds(const void* fn, size_t bytes) {
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return set_err(CLIPMI_EHIP, "hipFuncSetAttribute(%zu B LDS): %s", bytes, hipGetErrorString(e));
    }
    return 0;
}

// One kernel launch of the search paths: the LDS limit, the opt-in above 64 KiB, an optional event pair around the launch,
// and the launch check under `name`.
template <typename Args>
int launch_kernel(void (*kern)(Args), const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t st, hipEvent_t* ev,
                  const Args& a) {
    if (lds > (size_t)LDS_LIMIT) return set_err(CLIPMI_EUNSUPPORTED, "%s: %zu B of LDS", name, lds);
    if (int rc = opt_in_lds((const void*)kern, lds)) return rc;
    // measurement: plain event records around the launch (for a millisecond-scale kernel they agree
    // with rocprofv3's dispatch time to <1 %; hipExtLaunchKernel's start/stop events read ~7 % long here)
    if (ev) (void)hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(kern, grid, block, lds, st, a);
    if (ev) (void)hipEventRecord(ev[1], st);
    CLIPMI_CHECK_LAUNCH(name);
    return 0;
}

template <bool PREPASS>
int launch_scan(int E, int QG, const ScanArgs& a, int grid, int waves, size_t lds, hipStream_t st, hipEvent_t* ev = nullptr,
                int ny = 1) {
    auto go = [&](void (*kern)(ScanArgs)) {
        return launch_kernel(kern, "scan_topk_f32_kernel", dim3(grid, ny), dim3(waves * 64), lds, st, ev, a);
    };
    if (E == 512) return QG == 2 ? go(scan_topk_f32_kernel<512, PREPASS, 2>) : go(scan_topk_f32_kernel<512, PREPASS, 1>);
    return QG == 2 ? go(scan_topk_f32_kernel<768, PREPASS, 2>) : go(scan_topk_f32_kernel<768, PREPASS, 1>);
}

}  // namespace
}  // namespace clipmi

using namespace clipmi;

extern "C" size_t clipmi_topk_ip_workspace_bytes(int64_t N, int E, int Q, int K) {
    Plan p;
    if (!make_plan(N, E, Q, K, p)) {
        set_err(CLIPMI_EINVAL, "topk_ip: unsupported N=%lld E=%d Q=%d K=%d (E in {512,768}; 1 <= K <= %d at E = 512, <= %d at E = 768)",
                (long long)N, E, Q, K, max_k(512), max_k(768));
        return 0;
    }
    return align_up((size_t)p.QA * p.cap * sizeof(uint2), 256) + 256 /*gcnt*/ + 256 /*thr*/ + 256;
}

static int topk_ip_impl(const void* db_dev, int db_dtype, int64_t N, int E, const float* q_dev, int Q, int K,
                        int64_t id_base, float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                        void* stream, hipEvent_t* scan_ev) {
    if (db_dtype != CLIPMI_F32) return set_err(CLIPMI_EUNSUPPORTED, "topk_ip: db_dtype %d (only CLIPMI_F32)", db_dtype);
    if (!q_dev || !out_score_dev || !out_id_dev) return set_err(CLIPMI_EINVAL, "topk_ip: NULL pointer");
    if (N >= (1ll << 32) - 1) return set_err(CLIPMI_EINVAL, "topk_ip: N=%lld exceeds 2^32-2 rows per shard", (long long)N);
    Plan p;
    if (!make_plan(N, E, Q, K, p))
        return set_err(CLIPMI_EINVAL, "topk_ip: unsupported N=%lld E=%d Q=%d K=%d (E in {512,768}; 1 <= K <= %d at E = 512, <= %d at E = 768)",
                       (long long)N, E, Q, K, max_k(512), max_k(768));
    hipStream_t st = as_stream(stream);
    if (N == 0) {
        const long long n = (long long)Q * K;
        hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_score_dev,
                           (long long*)out_id_dev, n);
        CLIPMI_CHECK_LAUNCH("fill_empty_kernel");
        return 0;
    }
    if (!db_dev || !ws_dev) return set_err(CLIPMI_EINVAL, "topk_ip: NULL db or workspace");
    const size_t need_ws = clipmi_topk_ip_workspace_bytes(N, E, Q, K);
    if (ws_bytes < need_ws) return set_err(CLIPMI_EWORKSPACE, "topk_ip: workspace %zu < %zu", ws_bytes, need_ws);
    Arena ar(ws_dev, ws_bytes);
    uint2* cand = ar.take<uint2>((size_t)p.QA * p.cap);
    unsigned* gcnt = ar.take<unsigned>(32);
    float* thr0 = ar.take<float>(32);

    if (int rc = opt_in_lds((const void*)select_topk_kernel, p.lds_sel)) return rc;

    // candidate counters: zeroed once here; every select_topk_kernel re-zeroes the ones it consumed
    if (hipMemsetAsync(gcnt, 0, 128, st) != hipSuccess) return set_err(CLIPMI_EHIP, "hipMemsetAsync");
    for (int q0 = 0; q0 < Q; q0 += p.QA) {
        const int qa = (Q - q0) < p.QA ? (Q - q0) : p.QA;
        ScanArgs a;
        a.db = static_cast<const float*>(db_dev);
        a.q = q_dev + (size_t)q0 * E;
        a.QA = qa;
        a.K = K;
        a.C = p.C;
        a.wave_bytes = p.wave_bytes;
        a.cand = cand;
        a.gcnt = gcnt;
        a.cap = p.cap;
        a.thr_in = nullptr;
        a.run_if = nullptr;
        a.q_total = 0;
        if (p.sample) {
            // pre-pass: exact K-th best score of the first S rows = a valid lower bound for the
            // K-th best of all rows; the main pass then only buffers scores >= that bound
            a.nrows = p.sample_rows;
            int rc = launch_scan<true>(E, p.QG, a, p.grid_sample, p.waves, p.lds_scan, st);
            if (rc) return rc;
            SelectArgs s;
            s.cand = cand; s.gcnt = gcnt; s.cap = p.cap; s.K = K;
            s.thr_out = thr0;
            hipLaunchKernelGGL(select_topk_kernel, dim3(qa), dim3(SEL_THREADS), p.lds_sel, st, s);
            CLIPMI_CHECK_LAUNCH("select_topk_kernel(sample)");
            a.thr_in = thr0;
        }
        a.nrows = N;
        int rc = launch_scan<false>(E, p.QG, a, p.grid, p.waves, p.lds_scan, st, scan_ev);
        if (rc) return rc;
        SelectArgs s;
        s.cand = cand; s.gcnt = gcnt; s.cap = p.cap; s.K = K;
        s.id_base = id_base; s.out_s = out_score_dev + (size_t)q0 * K; s.out_i = (long long*)out_id_dev + (size_t)q0 * K;
        hipLaunchKernelGGL(select_topk_kernel, dim3(qa), dim3(SEL_THREADS), p.lds_sel, st, s);
        CLIPMI_CHECK_LAUNCH("select_topk_kernel");
    }
    return 0;
}

extern "C" int clipmi_topk_ip(const void* db_dev, int db_dtype, int64_t N, int E, const float* q_dev, int Q, int K,
                              int64_t id_base, float* out_score_dev, int64_t* out_id_dev, void* ws_dev,
                              size_t ws_bytes, void* stream) {
    return topk_ip_impl(db_dev, db_dtype, N, E, q_dev, Q, K, id_base, out_score_dev, out_id_dev, ws_dev, ws_bytes,
                        stream, nullptr);
}

namespace clipmi {
namespace {
constexpr long long COARSE_CAP = 1ll << 18;      // candidate slots per query of the coarse pass
constexpr int COARSE_SIDE_LDS = 100 * 1024;      // LDS of every kernel of the coarse path other than the scans: a 64-query
                                                 // int8 scan workgroup of an early segment takes 56 KiB, so one of these
                                                 // (from another batch in flight) fits beside it
constexpr int COARSE_MAIN_LDS = 104 * 1024;      // LDS the last segment's scan reserves, see launch_coarse
constexpr int COARSE_Q = 64;                     // queries per coarse pass. (128 per pass was tried: its 128-KiB query image
                                                 // leaves LDS for only 2 waves per CU = 2 of 4 SIMDs, and the pass turns
                                                 // MFMA-bound: 5.29 ms per 128 queries vs 2 x 2.21 ms)

// The scan of a 64-query pass for run-time (row width, 16-query groups, pre-pass name, copy): {512, 768} x {1, 2, 4} x {pre} x
// {int8, bf16}
template <int E, bool I8, class Go>
int launch_coarse_ei(int qg, bool pre, const Go& go) {
    switch (qg) {
    case 1: return pre ? go(scan_coarse_kernel<E, 1, true, I8>) : go(scan_coarse_kernel<E, 1, false, I8>);
    case 2: return pre ? go(scan_coarse_kernel<E, 2, true, I8>) : go(scan_coarse_kernel<E, 2, false, I8>);
    case 4: return pre ? go(scan_coarse_kernel<E, 4, true, I8>) : go(scan_coarse_kernel<E, 4, false, I8>);
    }
    return set_err(CLIPMI_EUNSUPPORTED, "scan_coarse: %d query groups", qg);
}

int launch_coarse(int E, int qg, bool pre, bool i8, const CoarseArgs& a, long long nsteps, hipStream_t st, hipEvent_t* ev) {
    if (E != 512 && E != 768) return set_err(CLIPMI_EUNSUPPORTED, "scan_coarse: E = %d", E);
    constexpr int WAVES = 4;
    // the final publication reuses the head of the query image for 3 * 16 QG counters: keep >= 1 KiB
    // (image: 1 KiB per query group and k-step - E = 768: 48 KiB int8, 96 KiB bf16 at 64 queries; + 4 x 6 KiB of lists)
    size_t lds = (size_t)qg * (E / (i8 ? 64 : 32)) * 1024 + WAVES * COARSE_WAVE_BYTES;
    // The LAST segment's scan (3/4 of the rows) reserves COARSE_MAIN_LDS although it uses 56-88 KiB: with two batches in
    // flight on two streams, two such scans then cannot share a CU. Sharing halves each one's bandwidth, both finish
    // together and both batches run their latency-bound side kernels at the same time with HBM idle (1.06-1.08 ms per 64
    // queries at 10 M rows); kept apart the streams settle half a batch out of phase - one scans while the other runs
    // its pre-pass, early segments, re-scoring and selects, which DO fit beside the early segments' unpadded scans - and a
    // batch takes 0.97-1.00 ms. (Padding every scan, i.e. the 114 KiB all of them used to need: 1.02-1.04 ms.)
    // development: CLIPMI_COARSE_WGS=2 - two workgroups (8 waves, 128 KB of rows in flight) per CU, no LDS padding
    static const int wgs = [] { const int v = (int)dev_knob("CLIPMI_COARSE_WGS", 1); return v == 2 ? 2 : 1; }();
    if (!pre && wgs == 1 && lds < (size_t)COARSE_MAIN_LDS) lds = COARSE_MAIN_LDS;
    long long g_ = (nsteps + WAVES - 1) / WAVES;
    const int grid = (int)(g_ < (long long)NUM_CU * wgs ? g_ : (long long)NUM_CU * wgs);
    auto go = [&](void (*kern)(CoarseArgs)) {
        return launch_kernel(kern, "scan_coarse_kernel", dim3(grid), dim3(WAVES * 64), lds, st, ev, a);
    };
    if (E == 768) return i8 ? launch_coarse_ei<768, true>(qg, pre, go) : launch_coarse_ei<768, false>(qg, pre, go);
    return i8 ? launch_coarse_ei<512, true>(qg, pre, go) : launch_coarse_ei<512, false>(qg, pre, go);
}

// coarse_prep_kernel for a run-time (row width, copy); E in {512, 768} (checked by the callers)
void launch_coarse_prep(int E, bool i8, unsigned blocks, hipStream_t st, const float* q, float rmax, float amax, int QA, float* qmeta,
                        uint4* qimage, unsigned* ctl, int nctl, int qs, int wide) {
    const auto kern = E == 768 ? (i8 ? coarse_prep_kernel<true, 768> : coarse_prep_kernel<false, 768>)
                               : (i8 ? coarse_prep_kernel<true, 512> : coarse_prep_kernel<false, 512>);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, st, q, E, rmax, amax, QA, qmeta, qimage, ctl, nctl, qs, wide);
}

// sample_scores_kernel for a run-time (row width, QG): 16 QG queries per workgroup, their f32 image in LDS (32 KiB per 16 queries,
// 48 KiB at E = 768)
int launch_sample_scores(int E, int QG, dim3 grid, hipStream_t st, const float* db, long long nrows, const float* q, int QA,
                         uint2* cand, long long cap, unsigned* gcnt) {
    const size_t lds = (size_t)QG * (E / 16) * 1024;
    const auto kern = E == 768 ? (QG == 2 ? sample_scores_kernel<768, 2> : sample_scores_kernel<768, 1>)
                               : (QG == 2 ? sample_scores_kernel<512, 2> : sample_scores_kernel<512, 1>);
    if (int rc = opt_in_lds((const void*)kern, lds)) return rc;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, db, nrows, q, QA, cand, cap, gcnt);
    return 0;
}

constexpr int COARSE_CTL = 2 * COARSE_Q + 32;     // fallback counters | coarse counters | flag block (word 0: the overflow flag)
inline int wide_qs(int Q) { return (Q + 63) / 64 * 64; }

// The workspace of one chunk of a coarse search and what sizes it: query stride, candidate slots per query, control words,
// uint4 entries of the query image, and whether the (unused) tauc slot of the 64-query passes exists.
struct WsShape { int qs; long long cap; int nctl; size_t image; bool tauc; };
struct CoarseWs {
    uint2* cand_e; uint2* cand_c; unsigned* gcnt_e; unsigned* gcnt_c; unsigned* flag; float* thr0; float* tauc;
    unsigned* last_m; float* qmeta; uint4* qimage;
};

// 64-query passes: the bf16 image of 64 queries, 64 KiB at E = 512, 96 KiB at 768 (int8: half of it)
inline WsShape pass64_shape(int E) { return {COARSE_Q, COARSE_CAP, COARSE_CTL, (size_t)4 * (E / 32) * 64, true}; }
// wide passes of Qc queries: 2 (E / 32) 64 entries per 64-query set: 32 KiB, 48 KiB at E = 768
inline WsShape wide_shape(int E, int Qc) {
    const int qs = wide_qs(Qc);
    return {qs, WIDE_CAP, 2 * qs + 4, qs / 64 * (size_t)(4 * E), false};
}

// the plan of the coarse path's side kernels (sample select, fallback scan + select): within COARSE_SIDE_LDS when K allows
bool coarse_plan(long long N, int E, int Q, int K, Plan& p) {
    const int q = Q > 32 ? 32 : Q;
    return make_plan(N, E, q, K, p, COARSE_SIDE_LDS) || make_plan(N, E, q, K, p);
}

size_t carve(const Plan& p, const WsShape& s, void* base, size_t cap, CoarseWs* w) {
    const size_t qs = (size_t)s.qs;
    Arena ar(base ? base : reinterpret_cast<void*>(256), cap);
    CoarseWs x;
    x.cand_e = ar.take<uint2>(qs * p.cap);             // the exact fallback's lists, all query groups side by side
    x.cand_c = ar.take<uint2>(qs * s.cap);
    x.gcnt_e = ar.take<unsigned>(s.nctl);              // one control block, cleared by coarse_prep_kernel
    x.gcnt_c = x.gcnt_e + qs;
    x.flag = x.gcnt_e + 2 * qs;
    x.thr0 = ar.take<float>(qs);
    x.tauc = s.tauc ? ar.take<float>(qs) : nullptr;
    x.last_m = ar.take<unsigned>(qs);
    x.qmeta = ar.take<float>(4 * qs);
    x.qimage = ar.take<uint4>(s.image);
    if (w) *w = x;
    return ar.off + 256;
}

inline int opt_in_rescore(int E = 512) {
    if (E == 768) return opt_in_lds((const void*)rescore_pairs_kernel<768>, rescore_lds(768));
    if (int rc = opt_in_lds((const void*)rescore_pairs_kernel<512>, RESCORE_LDS)) return rc;
    return opt_in_lds((const void*)rescore_pairs16_kernel<512>, RESCORE16_LDS);
}

// wide: the lists of a wide pass (up to 1 024 queries x ~500 pairs) go to the 16-pair form, the 64-query passes' to the 64-pair one
// E = 768: the 64-pair form only, for the wide pass too (the 16-pair form would hold 4 x 12 row chunks = 192 VGPRs in flight)
inline void launch_rescore(bool wide, dim3 grid, hipStream_t st, const float* db, const float* q, uint2* cand, const unsigned* gcnt,
                           long long cap, const unsigned* slot_rows, int E = 512) {
    if (E == 768) {
        hipLaunchKernelGGL(rescore_pairs_kernel<768>, grid, dim3(256), rescore_lds(768), st, db, q, cand, gcnt, cap, slot_rows);
        return;
    }
#ifdef CLIPMI_DEV
    static const int form = (int)dev_knob("CLIPMI_RESCORE", 0);            // 16 / 64: force one form (A/B)
    if (form == 16) wide = true;
    if (form == 64) wide = false;
#endif
    if (wide) hipLaunchKernelGGL(rescore_pairs16_kernel<512>, grid, dim3(256), RESCORE16_LDS, st, db, q, cand, gcnt, cap, slot_rows);
    else hipLaunchKernelGGL(rescore_pairs_kernel<512>, grid, dim3(256), RESCORE_LDS, st, db, q, cand, gcnt, cap, slot_rows);
}

// ---- wide pass: host side -----------------------------------------------------------------------------------------

bool wide_disabled() {          // CLIPMI_WIDE=0: searches of more than 64 queries as 64-query passes (A/B aid)
    static const bool off = dev_knob("CLIPMI_WIDE", 1) == 0;
    return off;
}

int wide_waves() {
    static const int w = dev_knob("CLIPMI_WIDE_WAVES", 8) == 4 ? 4 : 8;
    return w;
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
    const int x = blockIdx.x & 7, j = blockIdx.x >> 3, jb = gridDim.x >> 3;
    const int rlx = jb / ntile;
    if (j >= rlx * ntile) return;
    const int qt = j % ntile, nrl = __builtin_amdgcn_readfirstlane(rlx * 8);
    const int rl = (j / ntile) * 8 + x;
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
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<signed char*>(a.dbc) + (size_t)b_ * (32 * 512), 0, 32 * 512, 0x00020000);
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
            float xq = fmaf(-bm_.y, yq_, tq_) * __builtin_amdgcn_rcpf(bm_.x);      // 1 ulp: far inside the slack below
            xq = fminf(fmaxf(xq, -1.0e9f), 1.0e9f);
            xq = xq - 2.0f - fabsf(xq) * 2e-6f;
            const int dmin = (int)floorf(xq);
            auto max3 = [](int a_, int b_, int c_) { const int m_ = a_ > b_ ? a_ : b_; return m_ > c_ ? m_ : c_; };
            const int m0 = max3(acc[0], acc[1], acc[2]), m1 = max3(acc[3], acc[4], acc[5]), m2 = max3(acc[6], acc[7], acc[8]);
            const int m3 = max3(acc[9], acc[10], acc[11]), m4 = max3(acc[12], acc[13], acc[14]);
            const int ma = max3(m0, m1, m2), mb = max3(m3, m4, acc[15]);
            return ((ma > mb ? ma : mb) >= dmin) & (tq_ != INFINITY);      // +inf (padding query): never; no branch in the MFMA stream
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
                    wide_flush(list, npend, qbase, a.gcnt, a.cand, a.cap, a.overflow);
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
                const int slot = hcount + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                const unsigned ea = hq_a + (unsigned)slot * 96u;
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
    // final publication, aggregated per workgroup (one returning global atomic per (workgroup, query))
    __syncthreads();
    unsigned* hist = reinterpret_cast<unsigned*>(smem);              // the ring is dead now
    unsigned* gbase = hist + TILE_Q;
    unsigned* hoff = hist + 2 * TILE_Q;
    for (int i = tid; i < TILE_Q; i += 512) { hist[i] = 0; hoff[i] = 0; }
    __syncthreads();
    for (int e = lane; e < npend; e += 64) atomicAdd(&hist[list[e].x], 1u);
    __syncthreads();
    for (int i = tid; i < TILE_Q; i += 512) gbase[i] = hist[i] ? atomicAdd(&a.gcnt[qbase + i], hist[i]) : 0u;
    __syncthreads();
    for (int e = lane; e < npend; e += 64) {
        const uint2 c = list[e];
        const unsigned pos = gbase[c.x] + atomicAdd(&hoff[c.x], 1u);
        if ((long long)pos < a.cap) a.cand[(size_t)(qbase + c.x) * a.cap + pos] = make_uint2(CAND_SLOT, c.y);
        else *a.overflow = 1u;
    }
}

// groups per wave: always the two-group instantiation since round 5 - its tiles are balanced and a wave skips the groups it does
// not have, so a part-filled tile no longer costs a full one (round 4 picked tiles of 256 queries for 513-768 queries)
inline int wide2_groups(int Q) { (void)Q; return 2; }

template <int NB>
int launch_wide2(const WideArgs& a, hipStream_t st, hipEvent_t* ev, int ng) {
    const size_t lds = (size_t)NB * W2_SLOT + 8 * WIDE_WAVE_BYTES + 8 * 64 * 96;        // ring | pair lists | hit queues
    auto go = [&](void (*kern)(WideArgs)) {
        return launch_kernel(kern, "scan_coarse_wide2_kernel", dim3(NUM_CU), dim3(512), lds, st, ev, a);
    };
    return ng == 2 ? go(scan_coarse_wide2_kernel<NB, 2>) : go(scan_coarse_wide2_kernel<NB, 1>);
}

template <int WAVES, int ABL = 0, int KS = 16>
int launch_wide(const WideArgs& a, hipStream_t st, hipEvent_t* ev) {
    // image (2 KiB per k-step and 64-query set) | thresholds | lists: 8 waves 154 KiB at E = 512, 4 waves 110 KiB at E = 768
    if (a.spt > (KS == 24 ? WIDE768_TILE_SETS : WIDE_TILE_SETS)) return set_err(CLIPMI_EINVAL, "scan_coarse_wide: %d sets per tile", a.spt);
    const size_t lds = (size_t)a.spt * (KS * 2048) + 2048 + WAVES * WIDE_WAVE_BYTES;
    return launch_kernel(scan_coarse_wide_kernel<WAVES, ABL, KS>, "scan_coarse_wide_kernel", dim3(NUM_CU), dim3(WAVES * 64), lds, st, ev, a);
}

// segment boundaries of a wide search: rows [0, b[0]), [b[0], b[1]), ... [b[n-2], N); b[n-1] = N. After every segment the
// exact K-th best of all rows seen so far filters the next one, so the boundaries grow geometrically: with ratio r the
// number of exactly re-scored rows per query is about (segments) x (r - 1) x K x e^{0.36 z} - 5 segments of ratio 4 from
// 64 k rows give ~3 k at 10 M rows where the 64-query pass's three (ratio ~10 from N K / 2048) give ~5 k; a wide pass
// re-scores for up to 1024 queries at once (2 KB of f32 row per pair), so its re-scoring bytes rival the scan's
// (measured at 10 M rows, Q = 1024, same box: ratio 4 158 k q/s, 5 150 k, 6 152 k, 8 149 k, 3 146 k).
constexpr int WIDE_MAX_SEGS = 8;
int wide_segments(long long N, int K, long long S1, long long* b) {
    static const long long first = dev_knob("CLIPMI_WIDE_SEG0", 0);
    static const int ratio = [] { const int r = (int)dev_knob("CLIPMI_WIDE_SEG_RATIO", 4); return r >= 2 ? r : 4; }();
    long long s = first > 0 ? first : 65536;
    if (s < S1) s = S1;
    s = (s + 31) & ~31ll;
    int n = 0;
    while (n < WIDE_MAX_SEGS - 1 && s * 2 <= N && s + 65536 <= N) {
        b[n++] = s;
        s = (s * ratio) & ~31ll;
    }
    b[n++] = N;
    (void)K;
    return n;
}

// segment boundaries of a 64-query search, in wide_segments' form: [0, S2) (the pre-pass, its threshold from the sample),
// then [S2, N1) and [N1, N) with N1 ~ N/4, each scanned ONCE. After every segment the exact K-th best of all rows seen so far
// is the next segment's threshold: the last 75 % of the rows are filtered by the K-th best of the first 25 % (about 100
// survivors per query at 10 M rows instead of 6 k with the pre-pass threshold), which is what the exact re-scoring
// pass - a 2-KB row read per survivor - is paid for. One more segment would save ~25 us of re-scoring and cost
// ~55 us of launches.
int coarse_segments(long long N, int K, long long S1, long long* b) {
    // S2 ~ N*K/2048, so that only ~2-3 k rows per query survive the coarse pass; every survivor costs a 2-KB row read in the
    // re-scoring pass. The sample (S1 rows, no threshold) only feeds this segment's filter.
    // (not rounded up to a power of two: at 12.5 M rows that made the first segment 524 k rows instead of 311 k and its
    //  re-scoring, filtered only by the sample's weak bound, the largest of the three)
    // (one unfiltered scan of S2 rows was tried for small shards: its 32 k-entry selects cost more
    //  than the sample scan + select they replace)
    long long S2 = (N * (long long)K / 2048 + 31) & ~31ll;
    if (S2 > ((N / 8) & ~31ll)) S2 = (N / 8) & ~31ll;
    if (S2 < 32768) S2 = 32768;                     // > S1 (<= 12 288) always, and <= N / 2 (N >= 65536 here)
    long long N1 = (N / 4) & ~31ll;
    if (N1 < 4 * S2) N1 = 4 * S2;
    int n = 0;
    b[n++] = S2;
    if (N1 + 65536 <= N) b[n++] = N1;
    b[n++] = N;
    (void)S1;
    return n;
}

// ---- the coarse search: one set of stages, driven for 64-query and for wide passes ------------------------------------------
// The copy a search scans. i8 = false: dbc is the bf16 copy (rmeta, amax unused); i8 = true: dbc is the int8 copy, rmeta its
// per-row (scale, error norm) pairs padded to a multiple of 32 rows, amax >= every error norm
struct CoarseCopy { const void* dbc; const float2* rmeta; bool i8; float rmax, amax; };

// One chunk of a search (<= 64 or <= 1 024 queries): what every stage reads.
struct Chunk {
    int E, K, Q, qs;                 // Q: queries of this chunk; qs: the stride of qmeta and of the workspace's per-query arrays
    bool i8, wide;                   // wide: launch_rescore's form
    long long N, cap;                // cap: candidate slots per query
    const float* db; const float* q; const unsigned* slot_rows;
    Plan p; CoarseWs w;
    long long id_base; float* out_s; long long* out_i;
    hipStream_t st;
};

int coarse_check(const void* db, const CoarseCopy& cp, int64_t N, int E, const float* q, int Q, int K, const float* out_s,
                 const int64_t* out_i, const void* ws, Plan& p) {
    if (!db || !cp.dbc || !q || !out_s || !out_i || !ws || (cp.i8 && !cp.rmeta))
        return set_err(CLIPMI_EINVAL, "topk_ip_coarse: NULL pointer");
    if (cp.i8 && !(cp.amax >= 0.f)) return set_err(CLIPMI_EINVAL, "topk_ip_coarse_i8: amax=%g", cp.amax);
    if ((E != 512 && E != 768) || N < SAMPLE_MIN_N)
        return set_err(CLIPMI_EUNSUPPORTED, "topk_ip_coarse: needs E = 512 or 768 and N >= %d", SAMPLE_MIN_N);
    if (!(cp.rmax > 0.f) || N >= (1ll << 32) - 1)
        return set_err(CLIPMI_EINVAL, "topk_ip_coarse: rmax=%g N=%lld", cp.rmax, (long long)N);
    if (!coarse_plan(N, E, Q, K, p)) return set_err(CLIPMI_EINVAL, "topk_ip_coarse: unsupported Q=%d K=%d (1 <= K <= %d at E = %d)", Q, K, max_k(E), E);
    return 0;
}

// rows of the sample: it only has to thin the first segment's candidates (S2*K/S1 per query): 8 k rows are enough, and its
// select then ranks 8 k entries per query instead of 32 k (12288 = what the select keeps in LDS; N >= 65536 here)
inline long long sample_rows(const Plan& p) {
    const long long S1 = p.stage < 4096 ? 4096 : (p.stage / 16) * 16;
    return S1 > 12288 ? 12288 : S1;
}

// the sample (exact, unfiltered, every query of the chunk in one launch): scores of the first S1 rows -> K-th best per query
// = the first segment's threshold
int sample_threshold(const Chunk& c, long long S1, int QG, dim3 grid) {
    if (int rc = launch_sample_scores(c.E, QG, grid, c.st, c.db, S1, c.q, c.Q, c.w.cand_c, c.cap, c.w.gcnt_c)) return rc;
    CLIPMI_CHECK_LAUNCH("sample_scores_kernel");
    // the sample's lists are dense (entry e IS row e): only the 4 score bytes are staged (48 KiB instead of 96 per block;
    // round 5). S1 <= 12 288 rows always fit; LDS sized for them, not for the generic 8-byte stage
    SelectArgs s;
    s.cand = c.w.cand_c; s.gcnt = c.w.gcnt_c; s.cap = c.cap; s.K = c.K;
    s.thr_out = c.w.thr0; s.qmeta = c.w.qmeta; s.qs = c.qs;
    s.stage_cap = (int)S1; s.dense = 1; s.arm_fallback = c.w.flag;
    hipLaunchKernelGGL(select_topk_kernel, dim3(c.Q), dim3(SEL_THREADS), SEL_FIXED + (size_t)c.K * 8 + (size_t)S1 * 4 + 16, c.st, s);
    CLIPMI_CHECK_LAUNCH("select_topk_kernel(sample)");
    return 0;
}

// segment `seg` of the copy behind its scan: exact re-scoring of the survivors -> select. Every segment but the last leaves
// the exact K-th best of all rows seen so far as the next one's threshold; the last writes the result.
int rescore_select(const Chunk& c, int seg, bool last) {
    // ~1-3 k survivors per query = ~11 blocks of 256 pairs; a larger grid only queues idle blocks
    launch_rescore(c.wide, dim3(12, c.Q), c.st, c.db, c.q, c.w.cand_c, c.w.gcnt_c, c.cap, c.slot_rows, c.E);
    CLIPMI_CHECK_LAUNCH("rescore_pairs_kernel");
    // 4096 staged entries (32 KiB of LDS) cover these lists; a select block then fits on a CU even beside the
    // last segment's scan of ANOTHER batch in flight (104 KiB), which the 96-KiB staging of the sample select does not
    const int scap = c.p.stage < 4096 ? c.p.stage : 4096;
    SelectArgs s;
    s.cand = c.w.cand_c; s.gcnt = c.w.gcnt_c; s.cap = c.cap; s.K = c.K;
    if (last) { s.id_base = c.id_base; s.out_s = c.out_s; s.out_i = c.out_i; }
    else { s.thr_out = c.w.thr0; s.qmeta = c.w.qmeta; s.qs = c.qs; }
    // keep: bit 0 = the K best stay at the head of the list (gcnt = K) and the next segment appends behind them, so no row is
    // scanned twice; bit 1 = add to the survivor count
    s.m_out = c.w.last_m; s.keep = (last ? 0 : 1) | (seg > 0 ? 2 : 0); s.stage_cap = scap;
    hipLaunchKernelGGL(select_topk_kernel, dim3(c.Q), dim3(SEL_THREADS), SEL_FIXED + (size_t)c.K * 8 + (size_t)scap * 8, c.st, s);
    CLIPMI_CHECK_LAUNCH("select_topk_kernel(coarse)");
    return 0;
}

// fallback: exact scan + select, exiting at once unless a coarse list overflowed
// (two launches: the exact scan takes its groups of p.QA queries as blockIdx.y, each with its own lists)
int exact_fallback(const Chunk& c) {
    const Plan& p = c.p;
    ScanArgs a;
    a.db = c.db;
    a.K = c.K; a.C = p.C; a.wave_bytes = p.wave_bytes;
    a.cand = c.w.cand_e; a.gcnt = c.w.gcnt_e; a.cap = p.cap;
    a.q = c.q; a.QA = c.Q < p.QA ? c.Q : p.QA; a.q_total = c.Q; a.nrows = c.N; a.thr_in = c.w.thr0; a.run_if = c.w.flag;
    if (int rc = launch_scan<false>(c.E, p.QG, a, p.grid, p.waves, p.lds_scan, c.st, nullptr, (c.Q + p.QA - 1) / p.QA)) return rc;
    SelectArgs s;
    s.cand = c.w.cand_e; s.gcnt = c.w.gcnt_e; s.cap = p.cap; s.K = c.K;
    s.id_base = c.id_base; s.out_s = c.out_s; s.out_i = c.out_i;
    s.run_if = c.w.flag; s.stage_cap = p.stage;
    hipLaunchKernelGGL(select_topk_kernel, dim3(c.Q), dim3(SEL_THREADS), p.lds_sel, c.st, s);
    CLIPMI_CHECK_LAUNCH("select_topk_kernel(fallback)");
    return 0;
}

struct SampleGeom { int QG; dim3 grid; };

// The 64-query passes of the bf16 or the int8 copy: what they do their own way.
struct Pass64 {
    CoarseCopy copy;
    static constexpr bool wide = false;
    int chunk(int) const { return COARSE_Q; }
    WsShape shape(int E, int) const { return pass64_shape(E); }
    // per-query constants, the query image the scans copy, and the cleared counters + overflow flag (selects re-zero
    // what they consume): one launch per 64-query group
    unsigned prep_blocks(int Q) const { return (unsigned)((Q + 15) / 16 * 4); }
    SampleGeom sample(int Q, long long S1) const {
        long long gs = ((S1 + 15) / 16 + 3) / 4;
        if (gs > NUM_CU) gs = NUM_CU;
        return {1, dim3((unsigned)gs, (unsigned)((Q + 15) / 16))};
    }
    int segments(long long N, int K, long long S1, long long* b) const { return coarse_segments(N, K, S1, b); }
    // `pre` (every segment but the last) only picks the kernel NAME profilers average under
    int scan(const Chunk& c, long long r0, long long r1, bool last, hipEvent_t* ev) const {
        CoarseArgs a;
        a.dbc = copy.dbc; a.rmeta = copy.rmeta; a.qmeta = c.w.qmeta; a.qimage = c.w.qimage; a.q = c.q; a.QA = c.Q; a.tauc = c.w.tauc;
        a.row0 = r0; a.nrows = r1 - r0;
        a.cand = c.w.cand_c; a.gcnt = c.w.gcnt_c; a.cap = c.cap; a.overflow = c.w.flag;
        a.abl = (int)dev_knob("CLIPMI_COARSE_ABL", 0);
        return launch_coarse(c.E, c.Q <= 16 ? 1 : c.Q <= 32 ? 2 : 4, !last, copy.i8, a, (a.nrows + 31) / 32, c.st, ev);
    }
};

// The wide passes of the int8 copy (64 < Q): chunks of <= WIDE_MAX_Q queries, each ONE pass of the copy in segments.
// E = 768 (clipmi_topk_ip_wide_i8 only): the same sequence with the four-wave scan (tiles of 128 queries), the sample and the
// 64-pair re-scoring at 768; chunks of WIDE768_MAX_Q.
struct WidePass {
    CoarseCopy copy;
    static constexpr bool wide = true;
    int chunk(int E) const { return wide_max_q(E); }
    WsShape shape(int E, int Qc) const { return wide_shape(E, Qc); }
    unsigned prep_blocks(int Q) const { return (unsigned)((Q + 63) / 64 * 16); }
    SampleGeom sample(int Q, long long S1) const {
        // grid.y = 16-query groups (up to 64): blocks of the same x read the same rows, and every block first copies a
        // 32-KiB query image - so few, fat blocks per group (each wave 4+ row tiles) once the groups alone fill the chip
        long long gs = ((S1 + 15) / 16 + 3) / 4;
        if (gs > NUM_CU) gs = NUM_CU;
        static const int sdiv = [] { const int d = (int)dev_knob("CLIPMI_WIDE_SAMPLE_DIV", 8); return d > 0 ? d : 8; }();
        static const int sqg = (int)dev_knob("CLIPMI_WIDE_SAMPLE_QG", 2);
        const int ngroups = (Q + 16 * sqg - 1) / (16 * sqg);
        if (ngroups >= 8 / sqg && gs > sdiv) gs = (gs + sdiv - 1) / sdiv;
        // QG = 2 at 768 as well: 48 row registers more than at 512, inside the 512 of a 256-thread workgroup (resource table,
        // no scratch)
        return {sqg == 2 ? 2 : 1, dim3((unsigned)gs, (unsigned)ngroups)};
    }
    int segments(long long N, int K, long long S1, long long* b) const { return wide_segments(N, K, S1, b); }
    int scan(const Chunk& c, long long r0, long long r1, bool, hipEvent_t* ev) const {
        const int qc = c.Q, nsets = (qc + 63) / 64, tile_sets = c.E == 768 ? WIDE768_TILE_SETS : WIDE_TILE_SETS;
        WideArgs a;
        a.dbc = static_cast<const signed char*>(copy.dbc); a.rmeta = copy.rmeta; a.qmeta = c.w.qmeta; a.qimage = c.w.qimage;
        a.bmeta = copy.rmeta + i8_row_meta_entries(c.N);
        a.row0 = r0; a.nrows = r1 - r0;
        a.Q = qc; a.qs = c.qs;
        a.nqt = (nsets + tile_sets - 1) / tile_sets;
        a.spt = (nsets + a.nqt - 1) / a.nqt;
        a.cand = c.w.cand_c; a.gcnt = c.w.gcnt_c; a.cap = c.cap; a.overflow = c.w.flag;
        {
            static const int map_env = (int)dev_knob("CLIPMI_WIDE_MAP", 0), pf_env = (int)dev_knob("CLIPMI_WIDE_PF", 0);
            a.map_mode = map_env; a.pf_mode = pf_env;
        }
        if (c.E == 768) return launch_wide<4, 0, 24>(a, c.st, ev);
#ifdef CLIPMI_DEV
        static const int abl = (int)dev_knob("CLIPMI_WIDE_ABL", 0);        // ablations + the 4-wave form: development build only
        // CLIPMI_WIDE2=0: never the second form (A/B); CLIPMI_WIDE2_MINQ: smallest query count that takes it
        static const int w2 = (int)dev_knob("CLIPMI_WIDE2", 1);
        static const int w2_minq = (int)dev_knob("CLIPMI_WIDE2_MINQ", W2_MIN_Q);
        static const int w2_ng = (int)dev_knob("CLIPMI_WIDE2_NG", 0);              // 1 / 2: force the groups per wave (A/B)
        if (w2 && qc >= w2_minq) return launch_wide2<4>(a, c.st, ev, w2_ng == 1 || w2_ng == 2 ? w2_ng : wide2_groups(qc));
        return abl == 1 ? launch_wide<8, 1>(a, c.st, ev) : abl == 2 ? launch_wide<8, 2>(a, c.st, ev)
             : abl == 3 ? launch_wide<8, 3>(a, c.st, ev)
             : wide_waves() == 4 ? launch_wide<4>(a, c.st, ev) : launch_wide<8>(a, c.st, ev);
#else
        return qc >= W2_MIN_Q ? launch_wide2<4>(a, c.st, ev, wide2_groups(qc)) : launch_wide<8>(a, c.st, ev);
#endif
    }
};

// The coarse-then-exact search, chunk by chunk: prep -> sample threshold -> per segment of the copy (scan -> exact re-scoring
// -> select) -> exact fallback. `events` (measurement hooks): pairs handed out in order to the launches that stream the copy,
// as far as max_events reaches; *used = how many were recorded.
template <class Driver>
int coarse_search(const Driver& d, const void* db_dev, int64_t N, int E, const float* q_dev, int Q, int K, int64_t id_base,
                  float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes, void* stream,
                  hipEvent_t* events = nullptr, int max_events = 0, int* used = nullptr) {
    Chunk c;
    if (int rc = coarse_check(db_dev, d.copy, N, E, q_dev, Q, K, out_score_dev, out_id_dev, ws_dev, c.p)) return rc;
    const int chunk = d.chunk(E);
    const WsShape shape = d.shape(E, Q < chunk ? Q : chunk);
    if (ws_bytes < carve(c.p, shape, nullptr, ~(size_t)0, nullptr))
        return set_err(CLIPMI_EWORKSPACE, "topk_ip_coarse: workspace %zu too small", ws_bytes);
    carve(c.p, shape, ws_dev, ws_bytes, &c.w);
    c.E = E; c.K = K; c.qs = shape.qs; c.i8 = d.copy.i8; c.wide = Driver::wide; c.N = N; c.cap = shape.cap;
    c.db = static_cast<const float*>(db_dev);
    // int8: the rows the copy's slots hold, behind the block meta (quantize_rows_i8_kernel); bf16 copy: rows in order
    c.slot_rows = c.i8 ? i8_slot_rows(d.copy.rmeta, N) : nullptr;
    c.id_base = id_base; c.st = as_stream(stream);
    if (int rc = opt_in_lds((const void*)select_topk_kernel, c.p.lds_sel)) return rc;
    if (int rc = opt_in_rescore(E)) return rc;
    const long long S1 = sample_rows(c.p);
    long long bnd[WIDE_MAX_SEGS];
    const int nseg = d.segments(N, K, S1, bnd);
    int ev_used = 0;
    for (int q0 = 0; q0 < Q; q0 += chunk) {
        c.Q = (Q - q0) < chunk ? (Q - q0) : chunk;
        c.q = q_dev + (size_t)q0 * E;
        c.out_s = out_score_dev + (size_t)q0 * K;
        c.out_i = (long long*)out_id_dev + (size_t)q0 * K;
        launch_coarse_prep(E, c.i8, d.prep_blocks(c.Q), c.st, c.q, d.copy.rmax, d.copy.amax, c.Q, c.w.qmeta, c.w.qimage, c.w.gcnt_e,
                           shape.nctl, c.qs, Driver::wide);
        CLIPMI_CHECK_LAUNCH("coarse_prep_kernel");
        const SampleGeom sg = d.sample(c.Q, S1);
        if (int rc = sample_threshold(c, S1, sg.QG, sg.grid)) return rc;
        long long r0 = 0;
        for (int seg = 0; seg < nseg; r0 = bnd[seg++]) {
            const bool last = seg + 1 == nseg;
            hipEvent_t* ev = (events && ev_used + 2 <= max_events) ? events + ev_used : nullptr;
            if (int rc = d.scan(c, r0, bnd[seg], last, ev)) return rc;
            if (ev) ev_used += 2;
            if (int rc = rescore_select(c, seg, last)) return rc;
        }
        if (int rc = exact_fallback(c)) return rc;
    }
    if (used) *used = ev_used;
    return 0;
}

inline CoarseCopy i8_copy(const void* db_i8_dev, const float* meta_dev, float rmax, float amax) {
    return {db_i8_dev, reinterpret_cast<const float2*>(meta_dev), true, rmax, amax};
}
}  // namespace
}  // namespace clipmi

extern "C" size_t clipmi_topk_ip_coarse_workspace_bytes(int64_t N, int E, int Q, int K) {
    Plan p;
    if ((E != 512 && E != 768) || N < SAMPLE_MIN_N || !coarse_plan(N, E, Q, K, p)) {
        set_err(CLIPMI_EUNSUPPORTED, "topk_ip_coarse: unsupported: needs E = 512 or 768, N >= %d and 1 <= K <= %d at E = 512, <= %d at E = 768",
                SAMPLE_MIN_N, max_k(512), max_k(768));
        return 0;
    }
    size_t need = carve(p, pass64_shape(E), nullptr, ~(size_t)0, nullptr);
    // E = 768 has no wide pass: more than 64 queries run as 64-query passes inside the call, on the one 64-query workspace
    if (Q > COARSE_Q && E == 512) {           // the int8 path takes a search of more than 64 queries as wide passes
        const size_t wide = carve(p, wide_shape(E, Q < WIDE_MAX_Q ? Q : WIDE_MAX_Q), nullptr, ~(size_t)0, nullptr);
        need = wide > need ? wide : need;
    }
    return need;
}

extern "C" int clipmi_topk_ip_coarse(const void* db_dev, const void* db_bf16_dev, int64_t N, int E, float rmax,
                                     const float* q_dev, int Q, int K, int64_t id_base, float* out_score_dev,
                                     int64_t* out_id_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    return coarse_search(Pass64{{db_bf16_dev, nullptr, false, rmax, 0.f}}, db_dev, N, E, q_dev, Q, K, id_base, out_score_dev,
                         out_id_dev, ws_dev, ws_bytes, stream);
}

extern "C" size_t clipmi_i8_copy_bytes(int64_t N, int E) {
    return N < 0 || E < 32 ? 0 : (size_t)((N + 31) / 32 * 32) * (size_t)E;
}

extern "C" size_t clipmi_i8_meta_bytes(int64_t N) {
    return N < 0 ? 0 : (i8_row_meta_entries(N) + i8_block_meta_entries(N)) * sizeof(float2) + (size_t)((N + 31) / 32 * 32 + 32) * sizeof(unsigned);
}

extern "C" int clipmi_quantize_rows_i8(const float* db_dev, int64_t N, int E, const uint32_t* perm_dev, void* out_i8_dev,
                                       size_t out_i8_bytes, float* meta_dev, size_t meta_bytes, void* stream) {
    if (!db_dev || !out_i8_dev || !meta_dev || N < 1 || E < 32 || E % 32 != 0)
        return set_err(CLIPMI_EINVAL, "quantize_rows_i8: bad arguments (N=%lld E=%d; E must be a multiple of 32)", (long long)N, E);
    if (out_i8_bytes < clipmi_i8_copy_bytes(N, E) || meta_bytes < clipmi_i8_meta_bytes(N))
        return set_err(CLIPMI_EINVAL, "quantize_rows_i8: copy %zu B / meta %zu B, need %zu / %zu (clipmi_i8_copy_bytes, clipmi_i8_meta_bytes)",
                       out_i8_bytes, meta_bytes, clipmi_i8_copy_bytes(N, E), clipmi_i8_meta_bytes(N));
    if (N >= (1ll << 32) - 1) return set_err(CLIPMI_EINVAL, "quantize_rows_i8: N=%lld (slots are 32-bit)", (long long)N);
    float2* meta = reinterpret_cast<float2*>(meta_dev);
    hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3((unsigned)((N + 31) / 32)), dim3(256), 0, as_stream(stream), db_dev,
                       (long long)N, E, perm_dev, static_cast<signed char*>(out_i8_dev), meta, meta + i8_row_meta_entries(N),
                       const_cast<unsigned*>(i8_slot_rows(meta, N)));
    CLIPMI_CHECK_LAUNCH("quantize_rows_i8_kernel");
    return 0;
}

// ---- build-side helpers of the coarse copies (index load time, reference build-index.py:75-89 / query-index.py:60-75:
// the vectors are read once and kept): the bounds the coarse passes need and the bf16 copy, computed on the device by
// the library itself (r02 did these with framework tensor ops).
// stats2[0] = largest row norm, accumulated in f64 and rounded UP to f32 (a valid `rmax`); stats2[1] = largest a_r of
// the int8 copy's row meta (0 when meta is null). Non-negative floats order as their bit patterns: atomicMax on uint.
__global__ void __launch_bounds__(256) rows_stats_kernel(const float* __restrict__ db, long long N, int E, const float2* __restrict__ meta,
                                                         unsigned* __restrict__ stats2) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long long)gridDim.x * 4;
    float best = 0.f, abest = 0.f;
    for (long long r = wave0; r < N; r += nw) {
        const float* row = db + (size_t)r * E;
        double acc = 0.0;
        for (int k = lane * 4; k < E; k += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + k);
            acc += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        const double nd = sqrt(acc);
        float nf = (float)nd;
        if ((double)nf < nd) nf = nextafterf(nf, INFINITY);
        // a NaN row (or NaN error norm) must surface as a non-finite maximum: the index then keeps the search on the exact
        // path (index.py: isfinite(rmax)); `nf > best` alone would silently drop it
        best = !(nf == nf) ? INFINITY : (nf > best ? nf : best);
        if (meta && lane == 0) {
            const float a_ = meta[r].y;
            abest = !(a_ == a_) ? INFINITY : (a_ > abest ? a_ : abest);
        }
    }
    if (lane == 0) {
        atomicMax(stats2, __float_as_uint(best));
        if (meta) atomicMax(stats2 + 1, __float_as_uint(abest));
    }
}

__global__ void __launch_bounds__(256) rows_absmax_kernel(const float* __restrict__ db, long long N, int E, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long long)gridDim.x * 4;
    for (long long r = wave0; r < N; r += nw) {
        float mx = 0.f;
        for (int k = lane * 4; k < E; k += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(db + (size_t)r * E + k);
            mx = fmaxf(fmaxf(mx, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0) out[r] = mx;
    }
}

__global__ void __launch_bounds__(256) rows_to_bf16_kernel(const float* __restrict__ db, long long n4, uint2* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4*>(db)[i];
        out[i] = make_uint2(pack2_bf16(v.x, v.y), pack2_bf16(v.z, v.w));
    }
}

extern "C" int clipmi_rows_stats(const float* db_dev, int64_t N, int E, const float* meta_dev, float* stats2_dev, void* stream) {
    if (!db_dev || !stats2_dev || N < 1 || E < 4 || E % 4 != 0)
        return set_err(CLIPMI_EINVAL, "rows_stats: bad arguments (N=%lld E=%d; E must be a multiple of 4)", (long long)N, E);
    if (hipMemsetAsync(stats2_dev, 0, 2 * sizeof(float), as_stream(stream)) != hipSuccess) return set_err(CLIPMI_EHIP, "rows_stats: memset");
    const long long want = (N + 3) / 4;
    const unsigned grid = (unsigned)(want < 8 * NUM_CU ? want : 8 * NUM_CU);
    hipLaunchKernelGGL(rows_stats_kernel, dim3(grid), dim3(256), 0, as_stream(stream), db_dev, (long long)N, E,
                       reinterpret_cast<const float2*>(meta_dev), reinterpret_cast<unsigned*>(stats2_dev));
    CLIPMI_CHECK_LAUNCH("rows_stats_kernel");
    return 0;
}

extern "C" int clipmi_rows_absmax(const float* db_dev, int64_t N, int E, float* out_dev, void* stream) {
    if (!db_dev || !out_dev || N < 1 || E < 4 || E % 4 != 0) return set_err(CLIPMI_EINVAL, "rows_absmax: bad arguments (N=%lld E=%d)", (long long)N, E);
    const long long want = (N + 3) / 4;
    const unsigned grid = (unsigned)(want < 16 * NUM_CU ? want : 16 * NUM_CU);
    hipLaunchKernelGGL(rows_absmax_kernel, dim3(grid), dim3(256), 0, as_stream(stream), db_dev, (long long)N, E, out_dev);
    CLIPMI_CHECK_LAUNCH("rows_absmax_kernel");
    return 0;
}

// ---- clipmi_rows_order_by_absmax: the row order of the int8 copy (slot t holds row perm[t]), built by the
// library itself so that a C-ABI caller needs no framework sort: perm = the rows ordered by their largest |component|
// ascending, equal maxima in row order (a stable sort). Keys are the f32 bits of the maxima (non-negative floats order as
// their bit patterns); a least-significant-digit radix sort, four passes of 8 bits, each pass = per-block digit histogram ->
// one exclusive scan over (digit, block) -> stable scatter (a block keeps the order of its own items: ranks by wave ballots).
constexpr int ORD_THREADS = 256, ORD_ROUNDS = 8, ORD_TILE = ORD_THREADS * ORD_ROUNDS;

__global__ void __launch_bounds__(ORD_THREADS) order_hist_kernel(const unsigned* __restrict__ keys, long long N, int shift,
                                                                 unsigned* __restrict__ hist, unsigned nblocks) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * ORD_TILE;
    for (int r = 0; r < ORD_ROUNDS; ++r) {
        const long long i = base + r * ORD_THREADS + threadIdx.x;
        if (i < N) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];      // digit-major: one scan gives every (digit, block) base
}

// exclusive scan of n counters in place, ONE workgroup of 1024 threads (n = 256 x blocks: 0.6 M entries at 10 M rows): chunks of
// 4096 entries, four consecutive ones per thread (16-byte accesses), a wave scan + the 16 wave totals per chunk, a running carry
__global__ void __launch_bounds__(1024) order_scan_kernel(unsigned* __restrict__ v, long long n) {
    __shared__ unsigned wtot[16];
    __shared__ unsigned carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (long long base = 0; base < n; base += 4096) {
        const long long i0 = base + 4ll * tid;
        unsigned x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = i0 + j < n ? v[i0 + j] : 0u;
        const unsigned mine = x[0] + x[1] + x[2] + x[3];
        unsigned inc = mine;                               // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        unsigned before = carry_s;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        unsigned run = before + inc - mine;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < n) v[i0 + j] = run;
            run += x[j];
        }
        __syncthreads();
        if (tid == 1023) carry_s = before + inc;            // the chunk's total joins the carry
        __syncthreads();
    }
}

__global__ void __launch_bounds__(ORD_THREADS) order_scatter_kernel(const unsigned* __restrict__ keys_in, const unsigned* __restrict__ idx_in,
                                                                    long long N, int shift, const unsigned* __restrict__ offs,
                                                                    unsigned nblocks, unsigned* __restrict__ keys_out,
                                                                    unsigned* __restrict__ idx_out) {
    __shared__ unsigned run[256];              // items of this block already placed, per digit
    __shared__ unsigned wcnt[4][256];          // this round's count per (wave, digit)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    run[tid] = 0;
    const unsigned goff = offs[(size_t)tid * nblocks + blockIdx.x];        // thread t keeps digit t's global base
    __shared__ unsigned gbase[256];
    gbase[tid] = goff;
    const long long base = (long long)blockIdx.x * ORD_TILE;
    for (int r = 0; r < ORD_ROUNDS; ++r) {
#pragma unroll
        for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
        __syncthreads();
        const long long i = base + r * ORD_THREADS + tid;
        const bool live = i < N;
        const unsigned key = live ? keys_in[i] : 0u;
        const unsigned d = (key >> shift) & 255u;
        // lanes of this wave with the same digit (dead lanes match nobody): eight ballots
        unsigned long long same = __ballot(live);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot(live && ((d >> b) & 1u));
            same &= ((d >> b) & 1u) ? bal : ~bal;
        }
        const unsigned below = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (live && below == 0) wcnt[wave][d] = (unsigned)__popcll(same);
        __syncthreads();
        if (live) {
            unsigned pos = gbase[d] + run[d] + below;
            for (int w = 0; w < wave; ++w) pos += wcnt[w][d];
            keys_out[pos] = key;
            idx_out[pos] = idx_in ? idx_in[i] : (unsigned)i;
        }
        __syncthreads();
        run[tid] += wcnt[0][tid] + wcnt[1][tid] + wcnt[2][tid] + wcnt[3][tid];
        // (the next round's clear of wcnt is ordered behind this read by the barrier that follows the clear's own round start:
        //  every thread clears only its own column tid, which it alone has just read)
    }
}

static inline size_t order_blocks(int64_t N) { return (size_t)((N + ORD_TILE - 1) / ORD_TILE); }

extern "C" size_t clipmi_rows_order_workspace_bytes(int64_t N) {
    if (N < 1 || N >= (1ll << 32) - 1) return 0;
    // keys A | keys B | ids B | histogram [256][blocks]      (ids A is the caller's perm buffer)
    return (3 * (size_t)N + 256 * order_blocks(N)) * sizeof(unsigned) + 64;
}

extern "C" int clipmi_rows_order_by_absmax(const float* db_dev, int64_t N, int E, uint32_t* perm_dev, void* ws_dev, size_t ws_bytes,
                                           void* stream) {
    if (!db_dev || !perm_dev || !ws_dev || N < 1 || E < 4 || E % 4 != 0)
        return set_err(CLIPMI_EINVAL, "rows_order_by_absmax: bad arguments (N=%lld E=%d)", (long long)N, E);
    const size_t need = clipmi_rows_order_workspace_bytes(N);
    if (need == 0 || ws_bytes < need)
        return set_err(CLIPMI_EINVAL, "rows_order_by_absmax: workspace %zu B, need %zu (clipmi_rows_order_workspace_bytes; N < 2^32 - 1)", ws_bytes, need);
    unsigned* ka = static_cast<unsigned*>(ws_dev);
    unsigned* kb = ka + N;
    unsigned* ib = kb + N;
    unsigned* hist = ib + N;
    const unsigned nb = (unsigned)order_blocks(N);
    int rc = clipmi_rows_absmax(db_dev, N, E, reinterpret_cast<float*>(ka), stream);
    if (rc) return rc;
    // passes 0, 2 write (kb, ib), passes 1, 3 write (ka, perm): the last pass lands in the caller's buffer
    for (int pass = 0; pass < 4; ++pass) {
        const unsigned* kin = pass & 1 ? kb : ka;
        unsigned* kout = pass & 1 ? ka : kb;
        const unsigned* iin = pass == 0 ? nullptr : (pass & 1 ? ib : perm_dev);
        unsigned* iout = pass & 1 ? perm_dev : ib;
        hipLaunchKernelGGL(order_hist_kernel, dim3(nb), dim3(ORD_THREADS), 0, as_stream(stream), kin, (long long)N, 8 * pass, hist, nb);
        hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(1024), 0, as_stream(stream), hist, 256ll * nb);
        hipLaunchKernelGGL(order_scatter_kernel, dim3(nb), dim3(ORD_THREADS), 0, as_stream(stream), kin, iin, (long long)N, 8 * pass,
                           hist, nb, kout, iout);
    }
    CLIPMI_CHECK_LAUNCH("order_scatter_kernel");
    return 0;
}

extern "C" int clipmi_rows_to_bf16(const float* db_dev, int64_t N, int E, void* out_bf16_dev, void* stream) {
    if (!db_dev || !out_bf16_dev || N < 1 || E < 4 || E % 4 != 0)
        return set_err(CLIPMI_EINVAL, "rows_to_bf16: bad arguments (N=%lld E=%d; E must be a multiple of 4)", (long long)N, E);
    const long long n4 = (long long)N * E / 4, want = (n4 + 255) / 256;
    const unsigned grid = (unsigned)(want < 16 * NUM_CU ? want : 16 * NUM_CU);
    hipLaunchKernelGGL(rows_to_bf16_kernel, dim3(grid), dim3(256), 0, as_stream(stream), db_dev, n4, static_cast<uint2*>(out_bf16_dev));
    CLIPMI_CHECK_LAUNCH("rows_to_bf16_kernel");
    return 0;
}

extern "C" int clipmi_topk_ip_coarse_i8(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax, int64_t N,
                                        int E, float rmax, const float* q_dev, int Q, int K, int64_t id_base,
                                        float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    const CoarseCopy copy = i8_copy(db_i8_dev, meta_dev, rmax, amax);
    if (Q > COARSE_Q && E == 512 && !wide_disabled())
        return coarse_search(WidePass{copy}, db_dev, N, E, q_dev, Q, K, id_base, out_score_dev, out_id_dev, ws_dev, ws_bytes, stream);
    return coarse_search(Pass64{copy}, db_dev, N, E, q_dev, Q, K, id_base, out_score_dev, out_id_dev, ws_dev, ws_bytes, stream);
}

// The opt-in pair (ABI 8): clipmi_topk_ip_coarse_i8 with a wide pass at E = 768 as well. E = 512 and Q <= 64 ARE that function
// (and its workspace); E = 768 with more than 64 queries runs chunks of <= WIDE768_MAX_Q as one pass of the copy each.
extern "C" size_t clipmi_topk_ip_wide_workspace_bytes(int64_t N, int E, int Q, int K) {
    size_t need = clipmi_topk_ip_coarse_workspace_bytes(N, E, Q, K);          // 0 + `unsupported` under its conditions
    if (need == 0 || E != 768 || Q <= COARSE_Q) return need;
    Plan p;
    if (!coarse_plan(N, E, Q, K, p)) return need;
    const size_t wide = carve(p, wide_shape(E, Q < WIDE768_MAX_Q ? Q : WIDE768_MAX_Q), nullptr, ~(size_t)0, nullptr);
    return wide > need ? wide : need;
}

extern "C" int clipmi_topk_ip_wide_i8(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax, int64_t N,
                                      int E, float rmax, const float* q_dev, int Q, int K, int64_t id_base,
                                      float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    if (Q > COARSE_Q && E == 768)
        return coarse_search(WidePass{i8_copy(db_i8_dev, meta_dev, rmax, amax)}, db_dev, N, E, q_dev, Q, K, id_base, out_score_dev,
                             out_id_dev, ws_dev, ws_bytes, stream);
    return clipmi_topk_ip_coarse_i8(db_dev, db_i8_dev, meta_dev, amax, N, E, rmax, q_dev, Q, K, id_base, out_score_dev, out_id_dev,
                                    ws_dev, ws_bytes, stream);
}

// The event pairs of a measurement hook: created together, destroyed together (also when creation fails part-way).
namespace {
struct ScanEvents {
    static constexpr int MAX = 2 * WIDE_MAX_SEGS;
    hipEvent_t ev[MAX];
    int n = 0;
    bool create() {
        while (n < MAX && hipEventCreate(&ev[n]) == hipSuccess) ++n;
        return n == MAX;
    }
    ~ScanEvents() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
    double sum_ms(int used) const {          // the summed duration of the first `used` / 2 pairs
        double total = 0.0;
        for (int j = 0; j + 1 < used; j += 2) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, ev[j], ev[j + 1]);
            total += ms;
        }
        return total;
    }
};
}  // namespace

// Measurement hook of the wide passes (64 < Q, E = 512 or 768): the call `reps` times, chunk by chunk, with events around every
// wide scan launch; synchronises after each chunk to read its survivor counts and overflow flag (both are per-chunk state of the
// workspace). Everything reported is the LAST repetition's.
extern "C" int clipmi_dbg_topk_wide_i8_scan_ms(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax,
                                               int64_t N, int E, float rmax, const float* q_dev, int Q, int K,
                                               float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                                               void* stream, int reps, float* scan_ms, long long* survivors, int* scan_launches,
                                               int* fallback_armed) {
    if (!scan_ms || reps < 1 || Q <= COARSE_Q || (E != 512 && E != 768) || !q_dev || !out_score_dev || !out_id_dev)
        return set_err(CLIPMI_EINVAL, "dbg_topk_wide_i8_scan_ms: bad arguments (64 < Q, E = 512 or 768)");
    Plan p;
    if (N < SAMPLE_MIN_N || !coarse_plan(N, E, Q, K, p)) return set_err(CLIPMI_EUNSUPPORTED, "dbg_topk_wide_i8_scan_ms: unsupported N=%lld K=%d", (long long)N, K);
    const int chunk = wide_max_q(E);
    ScanEvents ev;
    if (!ev.create()) return set_err(CLIPMI_EHIP, "hipEventCreate");
    unsigned host[WIDE_MAX_Q > WIDE768_MAX_Q ? WIDE_MAX_Q : WIDE768_MAX_Q];
    hipStream_t st = as_stream(stream);
    const WidePass wide{i8_copy(db_i8_dev, meta_dev, rmax, amax)};
    int launches = 0, armed = 0;
    long long tot = 0;
    double total = 0.0;
    for (int r = 0; r < reps; ++r) {
        launches = 0; armed = 0; tot = 0; total = 0.0;
        for (int q0 = 0; q0 < Q; q0 += chunk) {
            const int qc = (Q - q0) < chunk ? (Q - q0) : chunk;
            int n_ev = 0;
            // a chunk of <= 64 queries (the tail of Q = k chunk + 1 ...) is still a wide pass inside a whole call: keep it one here
            if (int rc = coarse_search(wide, db_dev, N, E, q_dev + (size_t)q0 * E, qc, K, 0, out_score_dev + (size_t)q0 * K,
                                       out_id_dev + (size_t)q0 * K, ws_dev, ws_bytes, stream, ev.ev, ScanEvents::MAX, &n_ev))
                return rc;
            if (hipStreamSynchronize(st) != hipSuccess) return set_err(CLIPMI_EHIP, "hipStreamSynchronize");
            total += ev.sum_ms(n_ev);
            launches += n_ev / 2;
            CoarseWs w;
            carve(p, wide_shape(E, qc), ws_dev, ws_bytes, &w);
            unsigned flag = 0;
            if (hipMemcpy(host, w.last_m, sizeof(unsigned) * qc, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(&flag, w.flag, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
                return set_err(CLIPMI_EHIP, "hipMemcpy(wide counters)");
            for (int i = 0; i < qc; ++i) tot += host[i] < WIDE_CAP ? host[i] : WIDE_CAP;
            armed |= flag != 0;
        }
    }
    *scan_ms = (float)total;
    if (survivors) *survivors = tot;
    if (scan_launches) *scan_launches = launches;
    if (fallback_armed) *fallback_armed = armed;
    return 0;
}

// Measurement hook: a 64-query search (Q <= 64) `reps` times with events around the launches that stream the coarse copy ONCE -
// one scan per segment; *scan_ms = their summed duration, averaged over the repetitions
static int dbg_coarse_scan_ms(const void* db_dev, const CoarseCopy& copy, int64_t N, int E, const float* q_dev, int Q, int K,
                              float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes, void* stream, int reps,
                              float* scan_ms, long long* survivors) {
    if (!scan_ms || reps < 1 || Q > COARSE_Q) return set_err(CLIPMI_EINVAL, "dbg_topk_coarse_scan_ms: bad arguments");
    ScanEvents ev;
    if (!ev.create()) return set_err(CLIPMI_EHIP, "hipEventCreate");
    double total = 0.0;
    for (int i = 0; i < reps; ++i) {
        int n_ev = 0;
        if (int rc = coarse_search(Pass64{copy}, db_dev, N, E, q_dev, Q, K, 0, out_score_dev, out_id_dev, ws_dev, ws_bytes, stream,
                                   ev.ev, ScanEvents::MAX, &n_ev))
            return rc;
        if (hipStreamSynchronize(as_stream(stream)) != hipSuccess) return set_err(CLIPMI_EHIP, "hipStreamSynchronize");
        total += ev.sum_ms(n_ev);
    }
    *scan_ms = (float)(total / reps);
    if (survivors) {       // rows that survived the coarse pass, summed over the Q queries of the last call
        Plan p;
        CoarseWs w;
        coarse_plan(N, E, Q, K, p);
        carve(p, pass64_shape(E), ws_dev, ws_bytes, &w);
        unsigned host[COARSE_Q];
        if (hipMemcpy(host, w.last_m, sizeof(host), hipMemcpyDeviceToHost) != hipSuccess)
            return set_err(CLIPMI_EHIP, "hipMemcpy(gcnt)");
        long long tot = 0;
        for (int i = 0; i < Q; ++i) tot += host[i] < COARSE_CAP ? host[i] : COARSE_CAP;
        *survivors = tot;
    }
    return 0;
}

extern "C" int clipmi_dbg_topk_coarse_scan_ms(const void* db_dev, const void* db_bf16_dev, int64_t N, int E, float rmax,
                                              const float* q_dev, int Q, int K, float* out_score_dev, int64_t* out_id_dev,
                                              void* ws_dev, size_t ws_bytes, void* stream, int reps, float* scan_ms,
                                              long long* survivors) {
    return dbg_coarse_scan_ms(db_dev, {db_bf16_dev, nullptr, false, rmax, 0.f}, N, E, q_dev, Q, K, out_score_dev, out_id_dev,
                              ws_dev, ws_bytes, stream, reps, scan_ms, survivors);
}

extern "C" int clipmi_dbg_topk_coarse_i8_scan_ms(const void* db_dev, const void* db_i8_dev, const float* meta_dev, float amax,
                                                 int64_t N, int E, float rmax, const float* q_dev, int Q, int K,
                                                 float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                                                 void* stream, int reps, float* scan_ms, long long* survivors) {
    return dbg_coarse_scan_ms(db_dev, i8_copy(db_i8_dev, meta_dev, rmax, amax), N, E, q_dev, Q, K, out_score_dev, out_id_dev,
                              ws_dev, ws_bytes, stream, reps, scan_ms, survivors);
}

// Measurement hook (bench.py roofline): the same call sequence as clipmi_topk_ip, `reps` times,
// with HIP events recorded on `stream` around the MAIN scan kernel only; synchronises, and
// returns the average scan-kernel duration in milliseconds through *scan_ms. Q <= 32 (one pass).
extern "C" int clipmi_dbg_topk_scan_ms(const void* db_dev, int64_t N, int E, const float* q_dev, int Q, int K,
                                       float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                                       void* stream, int reps, float* scan_ms) {
    if (!scan_ms || reps < 1 || Q > 32) return set_err(CLIPMI_EINVAL, "dbg_topk_scan_ms: bad arguments");
    hipEvent_t ev[2];
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)
        return set_err(CLIPMI_EHIP, "hipEventCreate");
    double total = 0.0;
    int rc = 0;
    for (int i = 0; i < reps && rc == 0; ++i) {
        rc = topk_ip_impl(db_dev, CLIPMI_F32, N, E, q_dev, Q, K, 0, out_score_dev, out_id_dev, ws_dev, ws_bytes, stream, ev);
        if (rc) break;
        if (hipEventSynchronize(ev[1]) != hipSuccess) { rc = set_err(CLIPMI_EHIP, "hipEventSynchronize"); break; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev[0], ev[1]);
        total += ms;
    }
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    if (rc == 0) *scan_ms = (float)(total / reps);
    return rc;
}

extern "C" size_t clipmi_merge_topk_workspace_bytes(int R, int Q, int K) {
    (void)R; (void)Q; (void)K;
    return 256;   // the merge works out of LDS; a non-zero size keeps callers' allocation paths uniform
}

static int merge_impl(const float* scores_dev, const int64_t* ids_dev, long long rs_s, long long rs_i, int R, int Q,
                      int K, float* out_score_dev, int64_t* out_id_dev, void* stream) {
    if (!scores_dev || !ids_dev || !out_score_dev || !out_id_dev) return set_err(CLIPMI_EINVAL, "merge_topk: NULL pointer");
    if (R < 1 || Q < 1 || K < 1) return set_err(CLIPMI_EINVAL, "merge_topk: R=%d Q=%d K=%d", R, Q, K);
    const size_t lds = (size_t)R * K * 12 + 16;
    if (lds > (size_t)LDS_LIMIT) return set_err(CLIPMI_EUNSUPPORTED, "merge_topk: R*K=%d too large for one LDS pass", R * K);
    if (int rc = opt_in_lds((const void*)merge_lists_i64_kernel, lds)) return rc;
    hipLaunchKernelGGL(merge_lists_i64_kernel, dim3(Q), dim3(256), lds, as_stream(stream), scores_dev,
                       (const long long*)ids_dev, rs_s, rs_i, R, Q, K, out_score_dev, (long long*)out_id_dev);
    CLIPMI_CHECK_LAUNCH("merge_lists_i64_kernel");
    return 0;
}

extern "C" int clipmi_merge_topk(const float* scores_dev, const int64_t* ids_dev, int R, int Q, int K,
                                 float* out_score_dev, int64_t* out_id_dev, void* ws_dev, size_t ws_bytes,
                                 void* stream) {
    (void)ws_dev; (void)ws_bytes;
    return merge_impl(scores_dev, ids_dev, (long long)Q * K, (long long)Q * K, R, Q, K, out_score_dev, out_id_dev, stream);
}

// Same merge over the buffer ONE all-gather produces when every rank contributes a packed record
// [scores f32 Q*K | pad to 8 B | ids i64 Q*K]: rank r's record starts at gathered_dev + r*record_bytes.
extern "C" int clipmi_merge_topk_packed(const void* gathered_dev, size_t record_bytes, int R, int Q, int K,
                                        float* out_score_dev, int64_t* out_id_dev, void* stream) {
    const size_t ids_off = align_up((size_t)Q * K * 4, 8);
    if (!gathered_dev || record_bytes < ids_off + (size_t)Q * K * 8 || record_bytes % 8 != 0)
        return set_err(CLIPMI_EINVAL, "merge_topk_packed: record_bytes %zu for Q=%d K=%d", record_bytes, Q, K);
    const char* base = static_cast<const char*>(gathered_dev);
    return merge_impl(reinterpret_cast<const float*>(base), reinterpret_cast<const int64_t*>(base + ids_off),
                      (long long)(record_bytes / 4), (long long)(record_bytes / 8), R, Q, K, out_score_dev, out_id_dev,
                      stream);
}
