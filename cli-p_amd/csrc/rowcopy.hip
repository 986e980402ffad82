// rowcopy.hip — the build side of a search index (gfx950): the int8 and bf16 coarse copies of the f32 matrix, the bounds the
// coarse passes need (largest row norm, largest error norm) and the row order of the int8 copy. Runs once, at index load
// time; the search itself is topk.hip (coarse_scan.hpp holds the scans that read these copies).
#include "i8_layout.hpp"
#include <math.h>

namespace clipmi {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The int8 copy, in the layout of i8_layout.hpp: one workgroup per 32-row block.
// Row r: s_r = (max |x| over r's 32-row block) / 127, q_rk = rint(x_rk / s_r) in [-127, 127], a_r = 1.001 * ||x_r - s_r q_r||_2.
// a_r is an upper bound at any magnitude: e = x - s q is exact in f64 (24 + 7 significant bits against 24), its squares are
// summed in f64 and the root is rounded up (norm_up). A block whose largest |x| is below I8_TINY (1 / s would overflow from
// 2^-121 on, and 0 * inf is a NaN the clamp codes as -127) keeps scale 1 and zero codes, as an all-zero block does: a_r = ||x_r||.
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
    const float s = mx >= I8_TINY ? mx / 127.0f : 1.0f;
    const float inv = 1.0f / s;
    signed char* oblk = out + (size_t)blk * 32 * E;
    float amax_w = 0.f;
    for (int i = 0; i < 8; ++i) {
        const int rloc = wave * 8 + i;
        const long long t = r0 + rloc;                             // slot
        const long long r = t < N ? (perm ? (long long)perm[t] : t) : N;
        double ee = 0.0;
        for (int k = lane * 4; k < E; k += 256) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < N) v = *reinterpret_cast<const float4*>(db + (size_t)r * E + k);
            float qv[4] = {rintf(v.x * inv), rintf(v.y * inv), rintf(v.z * inv), rintf(v.w * inv)};
            const float xv[4] = {v.x, v.y, v.z, v.w};
            unsigned pk = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                qv[j] = fminf(fmaxf(qv[j], -127.f), 127.f);
                const double e = fma(-(double)s, (double)qv[j], (double)xv[j]);
                ee = fma(e, e, ee);
                pk |= ((unsigned)(int)qv[j] & 0xffu) << (8 * j);
            }
            const int ks = k >> 5, h = (k >> 4) & 1, b = k & 15;
            *reinterpret_cast<unsigned*>(oblk + (size_t)ks * 1024 + (h * 32 + rloc) * 16 + b) = pk;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ee += __shfl_xor(ee, o);
        const float a_r = r < N ? norm_up(ee) * 1.001f : 0.f;
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
        const float nf = norm_up(acc);
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

// The CLIPMI_F16 matrix of an index kept in fp16: each element rounded to the nearest binary16, ties to even
// (v_cvt_f16_f32 under the default rounding mode; the f16 denormal mode is IEEE, so subnormal results are produced and kept).
// counts2[0] += elements whose value changed (f32(f16(x)) != x; a NaN that stays NaN is not a change), counts2[1] += finite
// elements that became infinite (|x| >= 65520): a wave reduction, the four wave sums through LDS, one atomic pair per workgroup.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) rows_to_f16_kernel(const float* __restrict__ db, long long n4, f16x4* __restrict__ out,
                                                          unsigned long long* __restrict__ counts2) {
    __shared__ unsigned red[2][4];
    unsigned changed = 0, over = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4*>(db)[i];
        const f16x4 h = __builtin_convertvector(v, f16x4);
        const f32x4 b = __builtin_convertvector(h, f32x4);
        out[i] = h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            changed += (v[j] == v[j] && b[j] != v[j]) ? 1u : 0u;
            over += (fabsf(v[j]) < INFINITY && fabsf(b[j]) == INFINITY) ? 1u : 0u;
        }
    }
    if (!counts2) return;                                   // uniform
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        changed += __shfl_xor(changed, o);
        over += __shfl_xor(over, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = changed;
        red[1][wave] = over;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned long long t = (unsigned long long)red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (t) atomicAdd(counts2 + threadIdx.x, t);
    }
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

}  // namespace
}  // namespace clipmi

using namespace clipmi;

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

extern "C" int clipmi_rows_stats(const float* db_dev, int64_t N, int E, const float* meta_dev, float* stats2_dev, void* stream) {
    if (!db_dev || !stats2_dev || N < 1 || E < 4 || E % 4 != 0)
        return set_err(CLIPMI_EINVAL, "rows_stats: bad arguments (N=%lld E=%d; E must be a multiple of 4)", (long long)N, E);
    if (zero_async(stats2_dev, 2 * sizeof(float), as_stream(stream)) != hipSuccess) return set_err(CLIPMI_EHIP, "rows_stats: zero_async");
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

extern "C" int clipmi_rows_to_f16(const float* db_dev, int64_t N, int E, void* out_f16_dev, uint64_t* counts2_dev, void* stream) {
    if (!db_dev || !out_f16_dev || N < 1 || E < 4 || E % 4 != 0)
        return set_err(CLIPMI_EINVAL, "rows_to_f16: bad arguments (N=%lld E=%d; E must be a multiple of 4)", (long long)N, E);
    const long long n4 = (long long)N * E / 4, want = (n4 + 255) / 256;
    const unsigned grid = (unsigned)(want < 16 * NUM_CU ? want : 16 * NUM_CU);
    hipLaunchKernelGGL(rows_to_f16_kernel, dim3(grid), dim3(256), 0, as_stream(stream), db_dev, n4, static_cast<f16x4*>(out_f16_dev),
                       reinterpret_cast<unsigned long long*>(counts2_dev));
    CLIPMI_CHECK_LAUNCH("rows_to_f16_kernel");
    return 0;
}
