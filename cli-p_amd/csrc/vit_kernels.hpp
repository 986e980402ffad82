// vit_kernels.hpp — the non-GEMM kernels of the CLIP towers (gfx950): patch extraction with the
// fused pixel normalisation, CLS/positional rows, LayerNorm, the FP8 row quantisers, token embedding
// and EOT pooling; the launchers' declarations (the attention kernels themselves: attention.hpp). Reference call sites: model.encode_image (build-index.py:49),
// model.encode_text (query-index.py:108); op list in SURVEY.md §2.1.
#pragma once
#include "gemm.hpp"

namespace clipmi {

// ---------------------------------------------------------------------------------------------
// patches: pixels [B][3][R][R] (f32 / bf16 normalised, or u8 raw) -> bf16 [B*np][patch_k],
// column k = c*P*P + py*P + px (conv1.weight flattened), zero beyond 3*P*P. One thread = 8 px.
// u8 input fuses CLIP's transform tail (x/255 - mean)/std.
// ---------------------------------------------------------------------------------------------
struct PatchArgs {
    const void* pix;
    unsigned short* out;
    int dtype, B, R, P, grid, np, patch_k;
};

static __global__ void __launch_bounds__(256) patchify_kernel(PatchArgs a) {
    const long long total = (long long)a.B * a.np * (a.patch_k / 8);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int kc = a.patch_k / 8;
    const int k8 = (int)(i % kc);
    const long long bp = i / kc;
    const int p = (int)(bp % a.np);
    const int b = (int)(bp / a.np);
    const int PP = a.P * a.P;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    float v[8];
    if ((a.P & 7) == 0 && (a.R & 7) == 0) {
        // 8 consecutive pixels of one patch row: one aligned vector load (8 B for u8, 16 B for bf16,
        // 2 x 16 B for f32) instead of 8 scalar ones
        const int k = k8 * 8;
        if (k < 3 * PP) {
            const int c = k / PP, rem = k - c * PP;
            const int py = rem / a.P, px = rem - py * a.P;
            const int y = (p / a.grid) * a.P + py, xx = (p % a.grid) * a.P + px;
            const size_t src = (((size_t)b * 3 + c) * a.R + y) * a.R + xx;
            if (a.dtype == CLIPMI_F32) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.pix) + src);
                const f32x4 hi = *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.pix) + src + 4);
                v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
            } else if (a.dtype == CLIPMI_BF16) {
                const uint4 raw = *reinterpret_cast<const uint4*>(static_cast<const unsigned short*>(a.pix) + src);
                const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[2 * j] = __uint_as_float(w[j] << 16);
                    v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
                }
            } else {
                const uint2 raw = *reinterpret_cast<const uint2*>(static_cast<const unsigned char*>(a.pix) + src);
                const float m = mean[c], s = stdv[c];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned byte = ((j < 4 ? raw.x : raw.y) >> (8 * (j & 3))) & 0xffu;
                    v[j] = ((float)byte / 255.0f - m) / s;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
        }
    } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k8 * 8 + j;
        float x = 0.f;
        if (k < 3 * PP) {
            const int c = k / PP, rem = k - c * PP;
            const int py = rem / a.P, px = rem - py * a.P;
            const int y = (p / a.grid) * a.P + py, xx = (p % a.grid) * a.P + px;
            const size_t src = (((size_t)b * 3 + c) * a.R + y) * a.R + xx;
            if (a.dtype == CLIPMI_F32) x = static_cast<const float*>(a.pix)[src];
            else if (a.dtype == CLIPMI_BF16) x = bf16_to_f32(static_cast<const unsigned short*>(a.pix)[src]);
            else x = ((float)static_cast<const unsigned char*>(a.pix)[src] / 255.0f - mean[c]) / stdv[c];
        }
        v[j] = x;
    }
    }
    uint4 o = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    *reinterpret_cast<uint4*>(a.out + ((size_t)bp * a.patch_k + k8 * 8)) = o;
}

// u8 fast path of patchify_kernel for P % 16 == 0, R % 16 == 0 and patch_k == 3 P^2 (ViT-B/32, ViT-B/16): one workgroup
// per (image, channel, patch row) stages that strip - P image rows = P*R CONTIGUOUS bytes, whole lines - in LDS and writes
// the strip's patches in OUTPUT order, 16 bytes per lane, 1 KiB contiguous per wave-instruction. patchify_kernel maps
// threads along the output without staging: a wave then reads sixteen 32-byte pieces from sixteen lines whose other 96
// bytes belong to other workgroups (2.8 TB/s of useful bytes at B = 870); mapping threads along the input instead makes
// the stores the scattered side (3.5 TB/s).
static __global__ void __launch_bounds__(256) patchify_strip_u8_kernel(PatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int gy = blockIdx.x % a.grid;
    const int c = (blockIdx.x / a.grid) % 3;
    const int b = blockIdx.x / (3 * a.grid);
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f};
    const float stdv[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const float m = mean[c], sd = stdv[c];
    const unsigned char* src = static_cast<const unsigned char*>(a.pix) + (((size_t)b * 3 + c) * a.R + (size_t)gy * a.P) * a.R;
    // the value of a pixel depends on (byte, channel) only: 256 results of patchify_kernel's expression per workgroup, then
    // one 2-byte LDS lookup per pixel (the two f32 divisions per pixel made the pass VALU-bound: ~30 instructions each)
    unsigned short* lut = reinterpret_cast<unsigned short*>(smem + a.P * a.R);
    lut[threadIdx.x] = (unsigned short)(pack_bf16x2(((float)threadIdx.x / 255.0f - m) / sd, 0.f) & 0xffffu);
    const int nchunk = (a.P * a.R) >> 4;
    for (int j = threadIdx.x; j < nchunk; j += 256)
        *reinterpret_cast<uint4*>(smem + j * 16) = *reinterpret_cast<const uint4*>(src + (size_t)j * 16);
    __syncthreads();
    const int per_patch = (a.P * a.P) >> 3, per_row = a.P >> 3;          // 8-pixel output pieces
    for (int o = threadIdx.x; o < a.grid * per_patch; o += 256) {
        const int gx = o / per_patch, rem = o - gx * per_patch;
        const int y = rem / per_row, px = (rem - y * per_row) << 3;
        const uint2 raw = *reinterpret_cast<const uint2*>(smem + y * a.R + gx * a.P + px);
        unsigned w4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned word = k < 2 ? raw.x : raw.y;
            const unsigned b0 = (word >> (16 * (k & 1))) & 0xffu, b1 = (word >> (16 * (k & 1) + 8)) & 0xffu;
            w4[k] = (unsigned)lut[b0] | ((unsigned)lut[b1] << 16);
        }
        unsigned short* dst = a.out + ((size_t)b * a.np + gy * a.grid + gx) * a.patch_k + c * a.P * a.P + y * a.P + px;
        *reinterpret_cast<uint4*>(dst) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    }
}

// x[b*L + 0][:] = class_embedding + positional_embedding[0]
static __global__ void __launch_bounds__(256) cls_rows_kernel(float* x, const float* cls, const float* pos, int B, int L, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * W) return;
    const int b = (int)(i / W), c = (int)(i - (long long)b * W);
    x[(size_t)b * L * W + c] = cls[c] + pos[c];
}

// dst[b][:] = src[b * row_step][:], rows of row16 16-byte pieces: the class-token rows of the residual stream, compact, for
// the last block's tail (encode.hip)
static __global__ void __launch_bounds__(256) gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int B,
                                                                 int row_step, int row16) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * row16) return;
    const int b = (int)(i / row16), c = (int)(i - (long long)b * row16);
    dst[(size_t)b * row16 + c] = src[(size_t)b * row_step * row16 + c];
}

// x[q*L + t][:] = token_embedding[ids[q][t]] + positional_embedding[t]; one thread = 4 floats
static __global__ void __launch_bounds__(256) text_embed_kernel(float* x, const int* ids, const float* tok, const float* pos,
                                                         int Q, int L, int W, int vocab) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int wc = W / 4;
    if (i >= (long long)Q * L * wc) return;
    const int c4 = (int)(i % wc);
    const long long row = i / wc;
    const int t = (int)(row % L);
    int id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const f32x4 e = *reinterpret_cast<const f32x4*>(tok + (size_t)id * W + c4 * 4);
    const f32x4 p = *reinterpret_cast<const f32x4*>(pos + (size_t)t * W + c4 * 4);
    *reinterpret_cast<f32x4*>(x + (size_t)row * W + c4 * 4) = e + p;
}

// rowidx[q] = q*L + (first argmax of ids[q][:])  — the EOT row of each prompt
static __global__ void eot_rows_kernel(const int* ids, int* rowidx, int Q, int L) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    int best = ids[(size_t)q * L], bi = 0;
    for (int t = 1; t < L; ++t) {
        const int v = ids[(size_t)q * L + t];
        if (v > best) { best = v; bi = t; }
    }
    rowidx[q] = q * L + bi;
}

// ---------------------------------------------------------------------------------------------
// LayerNorm(eps 1e-5) over rows of f32 x: one wave per row, values held in registers,
// two-pass mean / variance as torch does. Source row r is x[rowidx ? rowidx[r] : r*row_step].
// ---------------------------------------------------------------------------------------------
struct LnArgs {
    const float* x;
    const float* w;
    const float* b;
    void* out;            // [M][W] bf16 or f32 (dense rows)
    const int* rowidx;    // optional gather
    long long row_step;   // source row stride in ROWS when rowidx == nullptr (1 = dense, L = CLS rows)
    int M, W, out_bf16;
    // FP8 path: when out8 is set, the row goes out as OCP e4m3 + one f32 scale instead of bf16 - exactly what
    // quantize_rows_fp8_kernel would make of the bf16 row (the values are rounded to bf16 first)
    unsigned char* out8;
    float* scale8;
    // split-residual input (gemm.hpp): when x == nullptr the source rows are the split rows x3 ([W bf16 hi | W u8 lo] each)
    const void* x3;
    // split-residual OUTPUT (ln_pre of an LN-folded tower): when out_x3 is set the normalised row leaves as a split row
    // plus its canonical statistics partials [M][W/256][2] (what split_stats_kernel would make of it)
    void* out_x3;
    float* out_part;
};

static __global__ void __launch_bounds__(256) layernorm_kernel(LnArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.M) return;
    const long long src_row = a.rowidx ? (long long)a.rowidx[r] : (long long)r * a.row_step;
    const float* p = a.x + src_row * a.W;
    f32x4 v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = i * 256 + lane * 4;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < a.W) {
            if (a.x) v[i] = *reinterpret_cast<const f32x4*>(p + c);
            else v[i] = split_join(*reinterpret_cast<const uint2*>(resid_hi(a.x3, (size_t)src_row, a.W) + c),
                                   *reinterpret_cast<const unsigned*>(resid_lo(a.x3, (size_t)src_row, a.W) + c));
        }
        s += v[i].x + v[i].y + v[i].z + v[i].w;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s / (float)a.W;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = i * 256 + lane * 4;
        if (c < a.W) {
            const f32x4 d = v[i] - mean;
            q += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = rsqrtf(q / (float)a.W + 1e-5f);
    if (a.out8) {
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * 256 + lane * 4;
            if (c < a.W) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(a.w + c);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(a.b + c);
                const f32x4 y = (v[i] - mean) * rstd * g + bb;
                const unsigned lo = pack_bf16x2(y.x, y.y), hi = pack_bf16x2(y.z, y.w);     // the bf16 row, kept in v[i]
                v[i] = f32x4{__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                             __uint_as_float(hi & 0xffff0000u)};
                mx = fmaxf(fmaxf(mx, fabsf(v[i].x)), fmaxf(fabsf(v[i].y), fmaxf(fabsf(v[i].z), fabsf(v[i].w))));
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        const float sc = mx > 0.f ? mx / 448.0f : 1.0f;
        const float inv = 1.0f / sc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * 256 + lane * 4;
            if (c < a.W) {
                int pk = 0;
                pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[i].x * inv, v[i].y * inv, pk, false);
                pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[i].z * inv, v[i].w * inv, pk, true);
                *reinterpret_cast<unsigned*>(a.out8 + (size_t)r * a.W + c) = (unsigned)pk;
            }
        }
        if (lane == 0) a.scale8[r] = sc;
        return;
    }
    if (a.out_x3) {              // W % 256 == 0 (checked by the launcher): segment i = columns 256 i .. 256 i + 255
        const int nseg = a.W >> 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < nseg) {
                const int c = i * 256 + lane * 4;
                const f32x4 g = *reinterpret_cast<const f32x4*>(a.w + c);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(a.b + c);
                const f32x4 y = (v[i] - mean) * rstd * g + bb;
                uint2 nh;
                unsigned nl;
                split_make(y, nh, nl);
                *reinterpret_cast<uint2*>(resid_hi(a.out_x3, (size_t)r, a.W) + c) = nh;
                *reinterpret_cast<unsigned*>(resid_lo(a.out_x3, (size_t)r, a.W) + c) = nl;
                const float sa = ln_wave_sum(ln_lane_sum(y));
                const float sq = ln_wave_sum(ln_lane_sumsq(y));
                if (lane == 0) *reinterpret_cast<f32x2*>(a.out_part + ((size_t)r * nseg + i) * 2) = f32x2{sa, sq};
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = i * 256 + lane * 4;
        if (c < a.W) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(a.w + c);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(a.b + c);
            const f32x4 y = (v[i] - mean) * rstd * g + bb;
            if (a.out_bf16)
                *reinterpret_cast<uint2*>(static_cast<unsigned short*>(a.out) + (size_t)r * a.W + c) =
                    make_uint2(pack_bf16x2(y.x, y.y), pack_bf16x2(y.z, y.w));
            else
                *reinterpret_cast<f32x4*>(static_cast<float*>(a.out) + (size_t)r * a.W + c) = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// LN-folded layers (gemm.hpp): the stand-alone producer of the split residual and its row statistics,
//   rows = ADD ? add[m][:] + x3[m][:] : x[m][:];   x3[m] = split_make(rows) (gemm.hpp: W bf16 hi | W u8 lo),
//   part[m][j] = (sum, sum of squares) of columns 256 j .. 256 j + 255
// used where the persistent residual GEMM's own store pass is not available (the embedded rows after ln_pre; residual
// GEMMs that run on the non-persistent kernels, whose acc + bias arrive as f32 in `add`). One wave per row,
// W % 256 == 0, W <= 1024; statistics in the canonical order (same bits as gemm256p's storers).
// ---------------------------------------------------------------------------------------------
template <bool ADD>
static __global__ void __launch_bounds__(256) split_stats_kernel(const float* __restrict__ x, void* x3, float* __restrict__ part,
                                                                 int M, int W) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int nseg = W >> 8;
    const float* p = x + (size_t)r * W;
    unsigned short* const hrow = resid_hi(x3, (size_t)r, W);
    unsigned char* const lrow = resid_lo(x3, (size_t)r, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < nseg) {
            const int c = j * 256 + lane * 4;
            f32x4 v = *reinterpret_cast<const f32x4*>(p + c);
            if (ADD) v = v + split_join(*reinterpret_cast<const uint2*>(hrow + c), *reinterpret_cast<const unsigned*>(lrow + c));
            uint2 nh;
            unsigned nl;
            split_make(v, nh, nl);
            *reinterpret_cast<uint2*>(hrow + c) = nh;
            *reinterpret_cast<unsigned*>(lrow + c) = nl;
            const float sa = ln_wave_sum(ln_lane_sum(v));
            const float sq = ln_wave_sum(ln_lane_sumsq(v));
            if (lane == 0) *reinterpret_cast<f32x2*>(part + ((size_t)r * nseg + j) * 2) = f32x2{sa, sq};
        }
    }
}

// text_embed_kernel + split_stats_kernel<false> + eot_rows_kernel in ONE launch (LN-folded text towers; round 5: one prompt is a
// chain of ~65 dependent launches of ~4 us, the three head kernels were three of them). Blocks [0, ceil(M / 4)): one wave per
// row - token + positional embedding, split_make, canonical statistics, exactly the bits of the three-kernel path; block
// ceil(M / 4): the EOT rows.
static __global__ void __launch_bounds__(256) text_embed_split_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                                                      const float* __restrict__ pos, void* x3, float* __restrict__ part,
                                                                      int* __restrict__ rowidx, int Q, int L, int W, int vocab) {
    const int M = Q * L, nrb = (M + 3) / 4;
    if ((int)blockIdx.x >= nrb) {
        for (int q = threadIdx.x; q < Q; q += 256) {
            int best = ids[(size_t)q * L], bi = 0;
            for (int t = 1; t < L; ++t) {
                const int v = ids[(size_t)q * L + t];
                if (v > best) { best = v; bi = t; }
            }
            rowidx[q] = q * L + bi;
        }
        return;
    }
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int nseg = W >> 8, t = r % L;
    int id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    unsigned short* const hrow = resid_hi(x3, (size_t)r, W);
    unsigned char* const lrow = resid_lo(x3, (size_t)r, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < nseg) {
            const int c = j * 256 + lane * 4;
            const f32x4 v = *reinterpret_cast<const f32x4*>(tok + (size_t)id * W + c) + *reinterpret_cast<const f32x4*>(pos + (size_t)t * W + c);
            uint2 nh;
            unsigned nl;
            split_make(v, nh, nl);
            *reinterpret_cast<uint2*>(hrow + c) = nh;
            *reinterpret_cast<unsigned*>(lrow + c) = nl;
            const float sa = ln_wave_sum(ln_lane_sum(v));
            const float sq = ln_wave_sum(ln_lane_sumsq(v));
            if (lane == 0) *reinterpret_cast<f32x2*>(part + ((size_t)r * nseg + j) * 2) = f32x2{sa, sq};
        }
    }
}

// ---------------------------------------------------------------------------------------------
// quantize_rows_fp8_kernel: bf16 [M][K] -> OCP e4m3 [M][K] + f32 scale [M] (the A operand of gemm256f8).
// One wave per row: scale = max|x| / 448 (1 for an all-zero row), q = RNE(x * (1 / scale)) by v_cvt_pk_fp8_f32;
// dequantised value = scale * q. K % 8 == 0.
// ---------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) quantize_rows_fp8_kernel(const unsigned short* __restrict__ in,
                                                                       unsigned char* __restrict__ out,
                                                                       float* __restrict__ scale, int M, int K) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const unsigned short* x = in + (size_t)r * K;
    float mx = 0.f;
    for (int k = lane * 8; k < K; k += 512) {
        const uint4 v = *reinterpret_cast<const uint4*>(x + k);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            mx = fmaxf(mx, fmaxf(fabsf(__uint_as_float(w[j] << 16)), fabsf(__uint_as_float(w[j] & 0xffff0000u))));
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float s = mx > 0.f ? mx / 448.0f : 1.0f;
    const float inv = 1.0f / s;
    for (int k = lane * 8; k < K; k += 512) {
        const uint4 v = *reinterpret_cast<const uint4*>(x + k);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
        float f[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f[2 * j] = __uint_as_float(w[j] << 16) * inv;
            f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u) * inv;
        }
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        *reinterpret_cast<uint2*>(out + (size_t)r * K + k) = make_uint2((unsigned)lo, (unsigned)hi);
    }
    if (lane == 0) scale[r] = s;
}

// ---------------------------------------------------------------------------------------------
// MX block scales for e4m3 activations (gemm256f8.hpp BSA; round 3): 32 consecutive values of a row share the e8m0
// scale 2^(e - 7), e = floor(log2(largest |x| of the block)) - the scaled values then lie below 256 (e4m3 holds 448),
// a block of zeros takes 2^0. fp8mx_scale_byte gives the scale's e8m0 byte from the block's largest magnitude (a
// non-negative float: its exponent field - 7, clamped at 0), fp8mx_inv the exact reciprocal of the scale as a float.
// Every producer (the stand-alone pass below, the QuickGELU epilogue of gemm256p, attention52x4's output stage) uses
// these two, so the bytes do not depend on who produced them.
// ---------------------------------------------------------------------------------------------
// quantize_rows_fp8mx_kernel: bf16 [M][K] -> e4m3 [M][K] + e8m0 block scales [M][K / 32]; one wave per row, a lane
// takes 8 consecutive values per step, the four lanes of a quad make one block. K % 32 == 0. The fallback producer
// (shapes whose producing kernel has no fused form) and the reference the fused producers are tested against.
static __global__ void __launch_bounds__(256) quantize_rows_fp8mx_kernel(const unsigned short* __restrict__ in,
                                                                         unsigned char* __restrict__ out,
                                                                         unsigned char* __restrict__ bscale, int M, int K) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const unsigned short* x = in + (size_t)r * K;
    for (int k0 = 0; k0 < K; k0 += 512) {
        const int k = k0 + lane * 8;
        const bool on = k < K;
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (on) {
            const uint4 v = *reinterpret_cast<const uint4*>(x + k);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f[2 * j] = __uint_as_float(w[j] << 16);
                f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
            }
        }
        float mx = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(f[j]));
        mx = fmaxf(mx, __shfl_xor(mx, 1));
        mx = fmaxf(mx, __shfl_xor(mx, 2));
        const unsigned sb = fp8mx_scale_byte(mx);
        const float inv = fp8mx_inv(sb);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] *= inv;
        if (on) {
            *reinterpret_cast<uint2*>(out + (size_t)r * K + k) = fp8_pack8(f);
            if ((lane & 3) == 0) bscale[(size_t)r * (K >> 5) + (k >> 5)] = (unsigned char)sb;
        }
    }
}

// rows_mx_stats_kernel (FP8 towers with folded LayerNorms, round 4): f32 rows [M][W] -> the rows as e4m3 with MX block
// scales [M][W] + [M][W / 32] and their canonical statistics partials [M][W / 256][2] - what the FP8 residual GEMM's store
// pass (EPI_BIAS_RESID_LN8) leaves behind for every later layer, here for the embedding stage's rows (ln_pre's output).
// One wave per row; per 256-column segment a lane holds 4 consecutive columns: gemm.hpp ln8_row_segment. W % 256 == 0.
static __global__ void __launch_bounds__(256) rows_mx_stats_kernel(const float* __restrict__ x, unsigned char* __restrict__ x8,
                                                                   unsigned char* __restrict__ bs, float* __restrict__ part,
                                                                   int M, int W) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int nseg = W >> 8;
    for (int sg = 0; sg < nseg; ++sg) {
        const size_t col = (size_t)sg * 256 + lane * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + (size_t)r * W + col);
        unsigned p4, sb;
        float sm, sq;
        ln8_row_segment(v, p4, sb, sm, sq);
        *reinterpret_cast<unsigned*>(x8 + (size_t)r * W + col) = p4;
        if ((lane & 7) == 0) bs[(size_t)r * (W >> 5) + (col >> 5)] = (unsigned char)sb;
        if (lane == 0) *reinterpret_cast<f32x2*>(part + ((size_t)r * nseg + sg) * 2) = f32x2{sm, sq};
    }
}

// host launchers (vit_kernels.hip)
int launch_layernorm(const LnArgs& a, hipStream_t st);
// out8 / out_bs / fused (FP8 towers): when the shape's kernel has the fused form, the rows are written as e4m3 + MX block
// scales into out8 / out_bs INSTEAD of bf16 into out and *fused is set; otherwise bf16 into out as always
// (attention.hpp holds the kernels). form: which kernel reads V how; the towers run ATTN_DEFAULT, the others are the
// tests' references (clipmi_dbg_attention)
enum AttnForm {
    ATTN_PLAIN_READS = 0,     // attention_kernel<.., TR = false> (2-byte V reads) for every L <= 80
    ATTN_DEFAULT = 1,         // 49 <= L <= 52 unmasked: attention52x4_kernel; other L <= 80: attention_kernel<.., TR = true>
    ATTN_ONE_WAVE = 2,        // as ATTN_DEFAULT, but 49 <= L <= 52 unmasked on attention52_kernel
};
int launch_attention(const unsigned short* qkv, unsigned short* out, int B, int L, int heads, int causal, AttnForm form,
                     hipStream_t st, unsigned char* out8 = nullptr, unsigned char* out_bs = nullptr, bool* fused = nullptr,
                     hipEvent_t* probe_ev = nullptr);     // probe_ev[0..1]: the dispatch's own begin / end (bench probe)
int launch_patchify(const PatchArgs& a, hipStream_t st);
int launch_quantize_rows_fp8(const unsigned short* in, unsigned char* out, float* scale, int M, int K, hipStream_t st);
int launch_quantize_rows_fp8mx(const unsigned short* in, unsigned char* out, unsigned char* bscale, int M, int K, hipStream_t st);
int launch_rows_mx_stats(const float* x, unsigned char* x8, unsigned char* bs, float* part, int M, int W, hipStream_t st);

}  // namespace clipmi
