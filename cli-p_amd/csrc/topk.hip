// topk.hip — exact flat inner-product top-K over a packed [N][E] f32 matrix (gfx950).
//
// Replaces `index.search(features, k + offset + 1)` (reference query-index.py:111) with an exact
// streaming pass. HBM-bound: the matrix is read once per batch of <= 16
// queries; scores are produced by v_mfma_f32_16x16x4_f32 (exact f32, one fmaf chain per
// (row, query) in a FIXED order, restated in oracle/topk_oracle.c) and selected per wavefront
// with a threshold filter + bounded candidate buffer in LDS.
// The coarse-then-exact path on top of it: its scans of the int8 / bf16 copies are coarse_scan.hpp (included below, one
// translation unit); the sample, the exact re-scoring, the select, the launchers, the drivers and the entries are here. The
// copies themselves are built by rowcopy.hip, in the layout of i8_layout.hpp.
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
    const unsigned* rows = nullptr;   // the row-list form (LIST) only: u32 [nrows] row numbers of db, ascending
    long long n_db = 0;               // the row-list form only: the rows db holds; a list entry >= n_db is skipped
};

// PREPASS only changes the kernel's NAME (profilers average per name; the threshold pre-pass over
// a few thousand rows must not dilute the main scan's average duration).
// QG = 16-query column groups per pass (1 or 2): every DB fragment feeds QG independent MFMA
// accumulator chains. The pass stays HBM-bound up to QG = 2 (f32 MFMA: 2 x 128 instructions of 32
// cycles per 32 KiB tile per SIMD = 16 B/clk/CU against ~10 B/clk/CU of HBM), and two chains hide
// the 40-cycle dependent-accumulator latency of a single one.
//
// LIST (the row-list form, clipmi_topk_ip_rows): the launch scans the rows a list names instead of rows [0, nrows). "Row" in the
// loop below then means LIST POSITION - a.nrows is the list's length M, tile t is entries 16 t .. 16 t + 15, the bound at
// publication is against M - and only two things differ: a lane's row address comes from its list entry rows[16 t + col], and a
// published candidate carries the entry of its accumulator row as its id. An entry >= a.n_db (the matrix's rows) becomes LIST_SKIP
// when it is loaded: it addresses row 0 and is never published. The entry of a tile has to be in a register one iteration before
// the rows it addresses are requested, so the list is read TWO tiles ahead (e_cur: this tile's MFMAs and ids, e_nxt: the refill's
// addresses, e_nn: in flight); one ahead, every tile would wait out a dependent HBM round trip.
// LIST is a template parameter of this kernel and not a sibling kernel around a shared body: with the body in an inlined device
// function the compiler allocates the plain form's registers differently (156 instead of 160 VGPRs at E = 512, QG = 2; 14
// instead of 10 AGPRs at 768), and the plain form's code is to stay what it was. The `if constexpr` branches leave it so; in
// profiles the list form is scan_topk_f32_kernel<E, PREPASS, QG, true>.
//
// RT (the row type; CLIPMI_F16 storage): float, or _Float16 for a matrix of IEEE binary16 rows of pitch 2 E bytes
// behind a.db. A lane then holds elements 16t + 4g .. + 3 of its row as four halves (8 bytes per t, half the tile's registers)
// and converts them to f32 - exactly, subnormals included: the f16 denormal mode is IEEE - in front of the four MFMAs of step t,
// which are the f32 form's own: the same operand values in the same chain, so the score order holds on the converted rows. The
// ring is the f32 form's (a chunk = 8 loads, refilled where its registers fall free). Like LIST it is a template parameter with
// its branches in `if constexpr`, and for the same reason: the float instantiations' code stays what it was.
constexpr unsigned LIST_SKIP = 0xffffffffu;       // no row id: topk_ip's N < 2^32 - 1
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
template <typename RT>
__device__ __forceinline__ auto ld_row(const RT* p) {
    if constexpr (std::is_same<RT, float>::value) return ld16_f<3>(p);
    else return *reinterpret_cast<const f16x4*>(p);
}
template <int E, bool PREPASS, int QG, bool LIST = false, typename RT = float>
__global__ void __launch_bounds__(256) scan_topk_f32_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool F16 = !std::is_same<RT, float>::value;
    constexpr int NT = E / 16;      // float4 (F16: four halves) per lane per 16-row tile
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
        typename std::conditional<F16, f16x4, f32x4>::type T[NT];
        const RT* const rdb = reinterpret_cast<const RT*>(a.db);
        // LIST: this lane's entry of list tile t (positions past the end clamp to the last entry, as rows do to last_row)
        [[maybe_unused]] auto entry = [&](long long t) -> unsigned {
            long long e = t * 16 + col;
            e = e > last_row ? last_row : e;
            const unsigned v = a.rows[e];
            return (long long)v < a.n_db ? v : LIST_SKIP;
        };
        unsigned e_cur = 0, e_nxt = 0;
        if constexpr (LIST) {
            e_cur = entry(tile);
            e_nxt = entry(tile + tw);
        }
        {
            long long r = tile * 16 + col;
            r = r > last_row ? last_row : r;
            if constexpr (LIST) r = e_cur == LIST_SKIP ? 0 : (long long)e_cur;
            const RT* p = rdb + r * E + 4 * g;
#pragma unroll
            for (int t = 0; t < NT; ++t) T[t] = ld_row<RT>(p + 16 * t);
        }
        while (true) {
            const long long nxt = tile + tw;
            const bool has_next = nxt < ntiles;
            long long rn = (has_next ? nxt : tile) * 16 + col;
            rn = rn > last_row ? last_row : rn;
            [[maybe_unused]] unsigned e_nn = 0;
            if constexpr (LIST) {
                e_nn = entry(nxt + tw);                                   // two tiles ahead: consumed by the NEXT refill
                rn = e_nxt == LIST_SKIP ? 0 : (long long)e_nxt;          // (no next tile: the list's last row, all lanes)
            }
            const RT* pn = rdb + rn * E + 4 * g;

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
                    f32x4 tv;
                    if constexpr (F16) tv = __builtin_convertvector(T[t], f32x4);      // exact
                    else tv = T[t];
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.x, bq[qg].x, acc[qg], 0, 0, 0);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.y, bq[qg].y, acc[qg], 0, 0, 0);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.z, bq[qg].z, acc[qg], 0, 0, 0);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg) acc[qg] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv.w, bq[qg].w, acc[qg], 0, 0, 0);
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
                    T[t] = ld_row<RT>(pn + 16 * t);
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
                // LIST: the id of accumulator row 4g + r is the entry the lane with col = 4g + r loaded (lanes 0..15)
                [[maybe_unused]] unsigned id[4];
                if constexpr (LIST) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) id[r] = (unsigned)__shfl((int)e_cur, 4 * g + r);
#pragma unroll
                    for (int qg = 0; qg < QG; ++qg)
#pragma unroll
                        for (int r = 0; r < 4; ++r) pp[qg][r] = pp[qg][r] && id[r] != LIST_SKIP;
                }
#pragma unroll
                for (int qg = 0; qg < QG; ++qg) {
                    const int qi = qg * 16 + col;
                    uint2* qb = buf + (size_t)qi * C;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (pp[qg][r]) {
                            const int pos = atomicAdd(&cnt[qi], 1);
                            if constexpr (LIST) qb[pos] = make_uint2(__float_as_uint(acc[qg][r]), id[r]);
                            else qb[pos] = make_uint2(__float_as_uint(acc[qg][r]), (unsigned)(row0 + r));
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
            if constexpr (LIST) {
                e_cur = e_nxt;
                e_nxt = e_nn;
            }
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

}  // namespace
}  // namespace clipmi

// The coarse-then-exact path: its superset argument, coarse_prep_kernel and the three scans of the coarse copies
// (scan_coarse_kernel, scan_coarse_wide_kernel, scan_coarse_wide2_kernel) with the pieces they share. It uses f32x4,
// wave_lds_sync and CLIPMI_NT_MASK from above; the re-scoring kernels, the launchers and the drivers follow here.
#include "coarse_scan.hpp"

namespace clipmi {
namespace {
constexpr size_t RESCORE16_LDS = 512 * 4 + 4 * 16 * 68 * 4;      // rescore_pairs16_kernel (E = 512 only: the wide passes): the query + four waves' tiles of 16 row chunks

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

// The row-list form's launch (a.rows, a.n_db set; a.nrows = list entries of the launch), under a name of its own in error texts.
template <bool PREPASS>
int launch_scan_rows(int E, int QG, const ScanArgs& a, int grid, int waves, size_t lds, hipStream_t st, hipEvent_t* ev = nullptr) {
    auto go = [&](void (*kern)(ScanArgs)) {
        return launch_kernel(kern, "scan_topk_f32_kernel(rows)", dim3(grid), dim3(waves * 64), lds, st, ev, a);
    };
    if (E == 512) return QG == 2 ? go(scan_topk_f32_kernel<512, PREPASS, 2, true>) : go(scan_topk_f32_kernel<512, PREPASS, 1, true>);
    return QG == 2 ? go(scan_topk_f32_kernel<768, PREPASS, 2, true>) : go(scan_topk_f32_kernel<768, PREPASS, 1, true>);
}

// The launches over a CLIPMI_F16 matrix (a.db points at halves): the same plan, grid and LDS as the f32 forms'.
template <bool PREPASS>
int launch_scan_f16(int E, int QG, const ScanArgs& a, int grid, int waves, size_t lds, hipStream_t st, hipEvent_t* ev = nullptr) {
    auto go = [&](void (*kern)(ScanArgs)) {
        return launch_kernel(kern, "scan_topk_f32_kernel(f16)", dim3(grid), dim3(waves * 64), lds, st, ev, a);
    };
    if (E == 512)
        return QG == 2 ? go(scan_topk_f32_kernel<512, PREPASS, 2, false, _Float16>) : go(scan_topk_f32_kernel<512, PREPASS, 1, false, _Float16>);
    return QG == 2 ? go(scan_topk_f32_kernel<768, PREPASS, 2, false, _Float16>) : go(scan_topk_f32_kernel<768, PREPASS, 1, false, _Float16>);
}

template <bool PREPASS>
int launch_scan_rows_f16(int E, int QG, const ScanArgs& a, int grid, int waves, size_t lds, hipStream_t st, hipEvent_t* ev = nullptr) {
    auto go = [&](void (*kern)(ScanArgs)) {
        return launch_kernel(kern, "scan_topk_f32_kernel(f16 rows)", dim3(grid), dim3(waves * 64), lds, st, ev, a);
    };
    if (E == 512)
        return QG == 2 ? go(scan_topk_f32_kernel<512, PREPASS, 2, true, _Float16>) : go(scan_topk_f32_kernel<512, PREPASS, 1, true, _Float16>);
    return QG == 2 ? go(scan_topk_f32_kernel<768, PREPASS, 2, true, _Float16>) : go(scan_topk_f32_kernel<768, PREPASS, 1, true, _Float16>);
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
    if (db_dtype != CLIPMI_F32 && db_dtype != CLIPMI_F16)
        return set_err(CLIPMI_EUNSUPPORTED, "topk_ip: db_dtype %d (only CLIPMI_F32 and CLIPMI_F16)", db_dtype);
    const bool f16 = db_dtype == CLIPMI_F16;
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
    if (zero_async(gcnt, 128, st) != hipSuccess) return set_err(CLIPMI_EHIP, "topk_ip: zero_async");
    for (int q0 = 0; q0 < Q; q0 += p.QA) {
        const int qa = (Q - q0) < p.QA ? (Q - q0) : p.QA;
        ScanArgs a;
        a.db = static_cast<const float*>(db_dev);        // CLIPMI_F16: halves, read as such by the f16 instantiations
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
            int rc = f16 ? launch_scan_f16<true>(E, p.QG, a, p.grid_sample, p.waves, p.lds_scan, st)
                         : launch_scan<true>(E, p.QG, a, p.grid_sample, p.waves, p.lds_scan, st);
            if (rc) return rc;
            SelectArgs s;
            s.cand = cand; s.gcnt = gcnt; s.cap = p.cap; s.K = K;
            s.thr_out = thr0;
            hipLaunchKernelGGL(select_topk_kernel, dim3(qa), dim3(SEL_THREADS), p.lds_sel, st, s);
            CLIPMI_CHECK_LAUNCH("select_topk_kernel(sample)");
            a.thr_in = thr0;
        }
        a.nrows = N;
        int rc = f16 ? launch_scan_f16<false>(E, p.QG, a, p.grid, p.waves, p.lds_scan, st, scan_ev)
                     : launch_scan<false>(E, p.QG, a, p.grid, p.waves, p.lds_scan, st, scan_ev);
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

// ---- The row-list form: clipmi_topk_ip's result restricted to the rows a u32 list names. Planned by
// make_plan(M, ...): the list's length takes the place of the row count everywhere - grid, list capacity (a scan publishes every
// (query, list position) pair at most once), whether the pre-pass runs - and the workspace has clipmi_topk_ip's layout for M rows.
extern "C" size_t clipmi_topk_ip_rows_workspace_bytes(int64_t M, int E, int Q, int K) {
    return clipmi_topk_ip_workspace_bytes(M, E, Q, K);
}

static int topk_ip_rows_impl(const void* db_dev, int db_dtype, int64_t N, int E, const uint32_t* rows_dev, int64_t M,
                             const float* q_dev, int Q, int K, int64_t id_base, float* out_score_dev, int64_t* out_id_dev,
                             void* ws_dev, size_t ws_bytes, void* stream, hipEvent_t* scan_ev) {
    if (db_dtype != CLIPMI_F32 && db_dtype != CLIPMI_F16)
        return set_err(CLIPMI_EUNSUPPORTED, "topk_ip_rows: db_dtype %d (only CLIPMI_F32 and CLIPMI_F16)", db_dtype);
    const bool f16 = db_dtype == CLIPMI_F16;
    if (!q_dev || !out_score_dev || !out_id_dev) return set_err(CLIPMI_EINVAL, "topk_ip_rows: NULL pointer");
    if (N < 0 || N >= (1ll << 32) - 1) return set_err(CLIPMI_EINVAL, "topk_ip_rows: N=%lld outside 0 .. 2^32-2 rows per shard", (long long)N);
    if (M < 0 || M > N) return set_err(CLIPMI_EINVAL, "topk_ip_rows: M=%lld list entries for N=%lld rows", (long long)M, (long long)N);
    if (M > 0 && !rows_dev) return set_err(CLIPMI_EINVAL, "topk_ip_rows: NULL row list with M=%lld", (long long)M);
    Plan p;
    if (!make_plan(M, E, Q, K, p))
        return set_err(CLIPMI_EINVAL, "topk_ip_rows: unsupported M=%lld E=%d Q=%d K=%d (E in {512,768}; 1 <= K <= %d at E = 512, <= %d at E = 768)",
                       (long long)M, E, Q, K, max_k(512), max_k(768));
    hipStream_t st = as_stream(stream);
    if (M == 0) {
        const long long n = (long long)Q * K;
        hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, out_score_dev,
                           (long long*)out_id_dev, n);
        CLIPMI_CHECK_LAUNCH("fill_empty_kernel");
        return 0;
    }
    if (!db_dev || !ws_dev) return set_err(CLIPMI_EINVAL, "topk_ip_rows: NULL db or workspace");
    const size_t need_ws = clipmi_topk_ip_rows_workspace_bytes(M, E, Q, K);
    if (ws_bytes < need_ws) return set_err(CLIPMI_EWORKSPACE, "topk_ip_rows: workspace %zu < %zu", ws_bytes, need_ws);
    Arena ar(ws_dev, ws_bytes);
    uint2* cand = ar.take<uint2>((size_t)p.QA * p.cap);
    unsigned* gcnt = ar.take<unsigned>(32);
    float* thr0 = ar.take<float>(32);

    if (int rc = opt_in_lds((const void*)select_topk_kernel, p.lds_sel)) return rc;
    if (zero_async(gcnt, 128, st) != hipSuccess) return set_err(CLIPMI_EHIP, "topk_ip_rows: zero_async");
    for (int q0 = 0; q0 < Q; q0 += p.QA) {
        const int qa = (Q - q0) < p.QA ? (Q - q0) : p.QA;
        ScanArgs a;
        a.db = static_cast<const float*>(db_dev);        // CLIPMI_F16: halves, read as such by the f16 instantiations
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
        a.rows = rows_dev;
        a.n_db = N;
        if (p.sample) {
            // pre-pass over the FIRST S LIST ENTRIES (M >= SAMPLE_MIN_N >= S), never over the first S rows of the matrix: only
            // the K-th best score of rows that ARE in the list is a lower bound for the K-th best of the list - a threshold
            // from rows outside it can lie above every listed score and would silently drop results
            a.nrows = p.sample_rows;
            int rc = f16 ? launch_scan_rows_f16<true>(E, p.QG, a, p.grid_sample, p.waves, p.lds_scan, st)
                         : launch_scan_rows<true>(E, p.QG, a, p.grid_sample, p.waves, p.lds_scan, st);
            if (rc) return rc;
            SelectArgs s;
            s.cand = cand; s.gcnt = gcnt; s.cap = p.cap; s.K = K;
            s.thr_out = thr0;
            hipLaunchKernelGGL(select_topk_kernel, dim3(qa), dim3(SEL_THREADS), p.lds_sel, st, s);
            CLIPMI_CHECK_LAUNCH("select_topk_kernel(rows sample)");
            a.thr_in = thr0;
        }
        a.nrows = M;
        int rc = f16 ? launch_scan_rows_f16<false>(E, p.QG, a, p.grid, p.waves, p.lds_scan, st, scan_ev)
                     : launch_scan_rows<false>(E, p.QG, a, p.grid, p.waves, p.lds_scan, st, scan_ev);
        if (rc) return rc;
        SelectArgs s;
        s.cand = cand; s.gcnt = gcnt; s.cap = p.cap; s.K = K;
        s.id_base = id_base; s.out_s = out_score_dev + (size_t)q0 * K; s.out_i = (long long*)out_id_dev + (size_t)q0 * K;
        hipLaunchKernelGGL(select_topk_kernel, dim3(qa), dim3(SEL_THREADS), p.lds_sel, st, s);
        CLIPMI_CHECK_LAUNCH("select_topk_kernel(rows)");
    }
    return 0;
}

extern "C" int clipmi_topk_ip_rows(const void* db_dev, int db_dtype, int64_t N, int E, const uint32_t* rows_dev, int64_t M,
                                   const float* q_dev, int Q, int K, int64_t id_base, float* out_score_dev, int64_t* out_id_dev,
                                   void* ws_dev, size_t ws_bytes, void* stream) {
    return topk_ip_rows_impl(db_dev, db_dtype, N, E, rows_dev, M, q_dev, Q, K, id_base, out_score_dev, out_id_dev, ws_dev,
                             ws_bytes, stream, nullptr);
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

// The same for clipmi_topk_ip_rows (tools/subset_timing.py): events around the main list scan only. Q <= 32 (one pass).
extern "C" int clipmi_dbg_topk_rows_scan_ms(const void* db_dev, int64_t N, int E, const uint32_t* rows_dev, int64_t M,
                                            const float* q_dev, int Q, int K, float* out_score_dev, int64_t* out_id_dev,
                                            void* ws_dev, size_t ws_bytes, void* stream, int reps, float* scan_ms) {
    if (!scan_ms || reps < 1 || Q > 32 || M < 1) return set_err(CLIPMI_EINVAL, "dbg_topk_rows_scan_ms: bad arguments");
    hipEvent_t ev[2];
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)
        return set_err(CLIPMI_EHIP, "hipEventCreate");
    double total = 0.0;
    int rc = 0;
    for (int i = 0; i < reps && rc == 0; ++i) {
        rc = topk_ip_rows_impl(db_dev, CLIPMI_F32, N, E, rows_dev, M, q_dev, Q, K, 0, out_score_dev, out_id_dev, ws_dev, ws_bytes,
                               stream, ev);
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

// Both hooks above in one, for a CLIPMI_F16 matrix (tools/f16_timing.py): rows_dev == NULL times the plain scan, otherwise the
// list form over M entries. Events around the main scan only. Q <= 32 (one pass).
extern "C" int clipmi_dbg_topk_scan_f16_ms(const void* db_f16_dev, int64_t N, int E, const uint32_t* rows_dev, int64_t M,
                                           const float* q_dev, int Q, int K, float* out_score_dev, int64_t* out_id_dev,
                                           void* ws_dev, size_t ws_bytes, void* stream, int reps, float* scan_ms) {
    if (!scan_ms || reps < 1 || Q > 32 || (rows_dev && M < 1)) return set_err(CLIPMI_EINVAL, "dbg_topk_scan_f16_ms: bad arguments");
    hipEvent_t ev[2];
    if (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess)
        return set_err(CLIPMI_EHIP, "hipEventCreate");
    double total = 0.0;
    int rc = 0;
    for (int i = 0; i < reps && rc == 0; ++i) {
        rc = rows_dev ? topk_ip_rows_impl(db_f16_dev, CLIPMI_F16, N, E, rows_dev, M, q_dev, Q, K, 0, out_score_dev, out_id_dev,
                                          ws_dev, ws_bytes, stream, ev)
                      : topk_ip_impl(db_f16_dev, CLIPMI_F16, N, E, q_dev, Q, K, 0, out_score_dev, out_id_dev, ws_dev, ws_bytes,
                                     stream, ev);
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