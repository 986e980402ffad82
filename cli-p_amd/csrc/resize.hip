// resize.hip — the geometry of the CLIP transform on the device (build-index.py:48): Pillow's bicubic
// resize of the shorter side to n_px + centre crop, bit for bit, for 8-bit RGB images that travel at full size.
//
// Pillow (the reference's dependency for this step; its published algorithm restated, not its code): 8-bit images are
// resampled in two passes, horizontal then vertical, each output a dot product of up to ksize taps with integer
// coefficients kk = trunc(w * 2^22 +- 0.5), accumulated in int32 from 2^21 and shifted right by 22, clipped to 0..255; the
// intermediate image between the passes is 8-bit. The coefficients depend on the sizes only; the HOST computes them
// (decode_worker.py: coeffs_window, the same float64 operations as Pillow's precompute_coeffs) for the n_px outputs per
// axis that survive the centre crop. These kernels do the integer part.
#include "common.hpp"

namespace clipmi {
namespace {

struct ResizeJob {             // mirrors clipmi_resize_job (include/clipmi.h)
    long long src_off;
    int w, h;
    int r0, nrows;
    int out_index;
    int need_h, need_v;
    int left, top;
    int hk, vk;
    long long hcoef_off, vcoef_off;
    long long tmp_off;
};

// horizontal pass: tmp[row][x][c] for the job's needed source rows and the n_px window columns.
// grid (row blocks, jobs); one thread per (row, x); per-axis coefficient block = [n_px] xmin | [n_px] cnt | [n_px][k] kk
__global__ void __launch_bounds__(256) resize_h_kernel(const unsigned char* __restrict__ raw, const ResizeJob* __restrict__ jobs,
                                                       const int* __restrict__ coef, int n_px, unsigned char* __restrict__ scratch) {
    const ResizeJob j = jobs[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / n_px, x = idx - row * n_px;
    if (row >= j.nrows) return;
    const unsigned char* src = raw + j.src_off + (size_t)(j.r0 + row) * j.w * 3;
    unsigned char* dst = scratch + j.tmp_off + ((size_t)row * n_px + x) * 3;
    if (!j.need_h) {
        const unsigned char* p = src + (size_t)(j.left + x) * 3;
        dst[0] = p[0]; dst[1] = p[1]; dst[2] = p[2];
        return;
    }
    const int* cf = coef + j.hcoef_off;
    const int xmin = cf[x], cnt = cf[n_px + x];
    const int* kk = cf + 2 * n_px + (size_t)x * j.hk;
    int a0 = 1 << (RZ_PREC - 1), a1 = a0, a2 = a0;
    const unsigned char* p = src + (size_t)xmin * 3;
    for (int k = 0; k < cnt; ++k) {
        const int c = kk[k];
        a0 += p[3 * k] * c; a1 += p[3 * k + 1] * c; a2 += p[3 * k + 2] * c;
    }
    dst[0] = rz_clip8(a0); dst[1] = rz_clip8(a1); dst[2] = rz_clip8(a2);
}

// vertical pass + planar store: out[out_index][c][y][x]
__global__ void __launch_bounds__(256) resize_v_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ coef, int n_px,
                                                       const unsigned char* __restrict__ scratch, unsigned char* __restrict__ out) {
    const ResizeJob j = jobs[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int y = idx / n_px, x = idx - y * n_px;
    if (y >= n_px) return;
    const unsigned char* tmp = scratch + j.tmp_off;
    unsigned char* o = out + (size_t)j.out_index * 3 * n_px * n_px + (size_t)y * n_px + x;
    const size_t plane = (size_t)n_px * n_px;
    if (!j.need_v) {
        const unsigned char* p = tmp + ((size_t)(j.top - j.r0 + y) * n_px + x) * 3;
        o[0] = p[0]; o[plane] = p[1]; o[2 * plane] = p[2];
        return;
    }
    const int* cf = coef + j.vcoef_off;
    const int ymin = cf[y], cnt = cf[n_px + y];
    const int* kk = cf + 2 * n_px + (size_t)y * j.vk;
    int a0 = 1 << (RZ_PREC - 1), a1 = a0, a2 = a0;
    const unsigned char* p = tmp + ((size_t)(ymin - j.r0) * n_px + x) * 3;
    const size_t rs = (size_t)n_px * 3;
    for (int k = 0; k < cnt; ++k) {
        const int c = kk[k];
        a0 += p[k * rs] * c; a1 += p[k * rs + 1] * c; a2 += p[k * rs + 2] * c;
    }
    o[0] = rz_clip8(a0); o[plane] = rz_clip8(a1); o[2 * plane] = rz_clip8(a2);
}

// ---- RGBA (clipmi_resize_crop_rgba8): Pillow resamples an image with alpha in its premultiplied mode (RGBa) and converts
// back; `convert("RGB")` then drops alpha. The same two passes over 4 bytes a pixel; a job that resamples an axis premultiplies
// every pixel the horizontal pass loads and un-premultiplies in front of the vertical pass's store. A job that resamples
// nothing is a crop that drops alpha: no round trip.
__device__ __forceinline__ unsigned rz_load_rgba(const unsigned char* p, bool premul) {
    unsigned v;
    __builtin_memcpy(&v, p, 4);
    if (!premul) return v;
    const unsigned a = v >> 24;
    unsigned o = v & 0xff000000u;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const unsigned t = ((v >> (8 * c)) & 255u) * a + 128u;
        o |= (((t >> 8) + t) >> 8) << (8 * c);
    }
    return o;
}

// The two passes over 4 bytes a pixel are written once (the `_px4` bodies) for the two pixel kinds that take them:
//   RZ_RGBA  as above: premultiplied while a job resamples, un-premultiplied and alpha dropped in front of the store
//   RZ_CMYK  (clipmi_resize_crop_cmyk8) Pillow resamples mode CMYK as four plain bands - no premultiplication - and
//            `convert("RGB")` is, per pixel, nk = 255 - K, out_c = clip8(nk - muldiv255(c, nk)) for c in C, M, Y with
//            muldiv255(a, b): t = a b + 128, ((t >> 8) + t) >> 8 (Convert.c cmyk2rgb) - applied in front of the vertical pass's
//            store, whether or not the job resamples
enum { RZ_RGBA = 0, RZ_CMYK = 1 };

__device__ __forceinline__ int rz_cmyk2rgb(int c, int nk) {
    const int t = c * nk + 128;
    const int v = nk - (((t >> 8) + t) >> 8);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

template <int KIND>
__device__ __forceinline__ void resize_h_px4(const unsigned char* __restrict__ raw, const ResizeJob* __restrict__ jobs,
                                             const int* __restrict__ coef, int n_px, unsigned char* __restrict__ scratch) {
    const ResizeJob j = jobs[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int row = idx / n_px, x = idx - row * n_px;
    if (row >= j.nrows) return;
    const bool premul = KIND == RZ_RGBA && (j.need_h || j.need_v);
    const unsigned char* src = raw + j.src_off + (size_t)(j.r0 + row) * j.w * 4;
    unsigned char* dst = scratch + j.tmp_off + ((size_t)row * n_px + x) * 4;      // (tmp_off: a multiple of 4)
    if (!j.need_h) {
        *reinterpret_cast<unsigned*>(dst) = rz_load_rgba(src + (size_t)(j.left + x) * 4, premul);
        return;
    }
    const int* cf = coef + j.hcoef_off;
    const int xmin = cf[x], cnt = cf[n_px + x];
    const int* kk = cf + 2 * n_px + (size_t)x * j.hk;
    int a0 = 1 << (RZ_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
    const unsigned char* p = src + (size_t)xmin * 4;
    for (int k = 0; k < cnt; ++k) {
        const int c = kk[k];
        const unsigned v = rz_load_rgba(p + 4 * k, KIND == RZ_RGBA);
        a0 += (int)(v & 255u) * c; a1 += (int)((v >> 8) & 255u) * c; a2 += (int)((v >> 16) & 255u) * c; a3 += (int)(v >> 24) * c;
    }
    // four byte stores, as resize_h_kernel's: with the four clips or-ed into one word hipcc (ROCm 7.2) picks v_ashr_pk_u8_i32 for
    // the lower pair and takes the upper half of its result for zero; on the MI355X B and A then carried stale bits of that
    // register wherever the tap count was odd
    dst[0] = rz_clip8(a0); dst[1] = rz_clip8(a1); dst[2] = rz_clip8(a2); dst[3] = rz_clip8(a3);
}

__global__ void __launch_bounds__(256) resize_h_rgba_kernel(const unsigned char* __restrict__ raw, const ResizeJob* __restrict__ jobs,
                                                            const int* __restrict__ coef, int n_px, unsigned char* __restrict__ scratch) {
    resize_h_px4<RZ_RGBA>(raw, jobs, coef, n_px, scratch);
}
__global__ void __launch_bounds__(256) resize_h_cmyk_kernel(const unsigned char* __restrict__ raw, const ResizeJob* __restrict__ jobs,
                                                            const int* __restrict__ coef, int n_px, unsigned char* __restrict__ scratch) {
    resize_h_px4<RZ_CMYK>(raw, jobs, coef, n_px, scratch);
}

template <int KIND>
__device__ __forceinline__ void resize_v_px4(const ResizeJob* __restrict__ jobs, const int* __restrict__ coef, int n_px,
                                             const unsigned char* __restrict__ scratch, unsigned char* __restrict__ out) {
    const ResizeJob j = jobs[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int y = idx / n_px, x = idx - y * n_px;
    if (y >= n_px) return;
    const unsigned* tmp = reinterpret_cast<const unsigned*>(scratch + j.tmp_off);
    unsigned char* o = out + (size_t)j.out_index * 3 * n_px * n_px + (size_t)y * n_px + x;
    const size_t plane = (size_t)n_px * n_px;
    int c0, c1, c2, a;
    if (!j.need_v) {
        const unsigned v = tmp[(size_t)(j.top - j.r0 + y) * n_px + x];
        c0 = v & 255u; c1 = (v >> 8) & 255u; c2 = (v >> 16) & 255u; a = v >> 24;
    } else {
        const int* cf = coef + j.vcoef_off;
        const int ymin = cf[y], cnt = cf[n_px + y];
        const int* kk = cf + 2 * n_px + (size_t)y * j.vk;
        int a0 = 1 << (RZ_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
        const unsigned* p = tmp + (size_t)(ymin - j.r0) * n_px + x;
        for (int k = 0; k < cnt; ++k) {
            const int c = kk[k];
            const unsigned v = p[(size_t)k * n_px];
            a0 += (int)(v & 255u) * c; a1 += (int)((v >> 8) & 255u) * c; a2 += (int)((v >> 16) & 255u) * c; a3 += (int)(v >> 24) * c;
        }
        c0 = rz_clip8(a0); c1 = rz_clip8(a1); c2 = rz_clip8(a2); a = rz_clip8(a3);
    }
    if (KIND == RZ_CMYK) {                                     // the fourth byte is K
        const int nk = 255 - a;
        c0 = rz_cmyk2rgb(c0, nk); c1 = rz_cmyk2rgb(c1, nk); c2 = rz_cmyk2rgb(c2, nk);
    } else if ((j.need_h || j.need_v) && a != 0 && a != 255) {        // Pillow's RGBa -> RGBA: copy at alpha 0 and 255, else clip(255 c / a)
        c0 = min(255, 255 * c0 / a); c1 = min(255, 255 * c1 / a); c2 = min(255, 255 * c2 / a);
    }
    o[0] = (unsigned char)c0; o[plane] = (unsigned char)c1; o[2 * plane] = (unsigned char)c2;
}

__global__ void __launch_bounds__(256) resize_v_rgba_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ coef, int n_px,
                                                            const unsigned char* __restrict__ scratch, unsigned char* __restrict__ out) {
    resize_v_px4<RZ_RGBA>(jobs, coef, n_px, scratch, out);
}
__global__ void __launch_bounds__(256) resize_v_cmyk_kernel(const ResizeJob* __restrict__ jobs, const int* __restrict__ coef, int n_px,
                                                            const unsigned char* __restrict__ scratch, unsigned char* __restrict__ out) {
    resize_v_px4<RZ_CMYK>(jobs, coef, n_px, scratch, out);
}

// ---- index rows (clipmi_nearest_crop_p8): Pillow resizes palette and 1-bit images with NEAREST whatever filter is asked for;
// the host computes which source column and row each of the n_px x n_px outputs takes (decode_worker.nearest_window: Pillow's
// float64 accumulation), the kernel gathers and looks the palette up. One thread per output pixel, no scratch.
struct NearestJob {            // mirrors clipmi_nearest_job (include/clipmi.h)
    long long src_off;
    int w, h;
    int out_index, reserved;
    long long pal_off, col_off, row_off;
};

__global__ void __launch_bounds__(256) nearest_p8_kernel(const unsigned char* __restrict__ raw, const NearestJob* __restrict__ jobs,
                                                         const unsigned char* __restrict__ tabs, int n_px, unsigned char* __restrict__ out) {
    const NearestJob j = jobs[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int y = idx / n_px, x = idx - y * n_px;
    if (y >= n_px) return;
    const int* it = reinterpret_cast<const int*>(tabs);
    const int sx = min(max(it[j.col_off + x], 0), j.w - 1), sy = min(max(it[j.row_off + y], 0), j.h - 1);     // (stay inside the image
    const unsigned char* pal = tabs + j.pal_off + 3 * (size_t)raw[j.src_off + (size_t)sy * j.w + sx];         // whatever the tables say)
    unsigned char* o = out + (size_t)j.out_index * 3 * n_px * n_px + (size_t)y * n_px + x;
    const size_t plane = (size_t)n_px * n_px;
    o[0] = pal[0]; o[plane] = pal[1]; o[2 * plane] = pal[2];
}

}  // namespace
}  // namespace clipmi

// the vertical pass by itself: jpeg.hip's transform entries run it behind their own horizontal pass
int clipmi::launch_resize_v_rgb8(const void* jobs_dev, int njobs, const int32_t* coef_dev, int n_px, const void* scratch_dev, void* out_dev,
                                 hipStream_t st) {
    const long long per_v = (long long)n_px * n_px;
    hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((per_v + 255) / 256), (unsigned)njobs), dim3(256), 0, st,
                       static_cast<const ResizeJob*>(jobs_dev), coef_dev, n_px, static_cast<const unsigned char*>(scratch_dev),
                       static_cast<unsigned char*>(out_dev));
    CLIPMI_CHECK_LAUNCH("resize_v_kernel");
    return 0;
}

using namespace clipmi;

extern "C" int clipmi_resize_crop_rgb8(const void* raw_dev, const void* jobs_dev, int njobs, int max_rows, const int32_t* coef_dev,
                                       int n_px, void* out_dev, void* scratch_dev, void* stream) {
    static_assert(sizeof(ResizeJob) == 80, "clipmi_resize_job layout");
    if (njobs == 0) return 0;
    if (!raw_dev || !jobs_dev || !coef_dev || !out_dev || !scratch_dev || njobs < 0 || n_px < 1 || n_px > 4096 || max_rows < 1)
        return set_err(CLIPMI_EINVAL, "resize_crop_rgb8: bad arguments");
    hipStream_t st = as_stream(stream);
    const long long per_h = (long long)max_rows * n_px;
    hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)((per_h + 255) / 256), (unsigned)njobs), dim3(256), 0, st,
                       static_cast<const unsigned char*>(raw_dev), static_cast<const ResizeJob*>(jobs_dev), coef_dev, n_px,
                       static_cast<unsigned char*>(scratch_dev));
    CLIPMI_CHECK_LAUNCH("resize_h_kernel");
    return launch_resize_v_rgb8(jobs_dev, njobs, coef_dev, n_px, scratch_dev, out_dev, st);
}

// The two entries over 4-byte pixels: the same checks and launches, each with its instantiation of the passes
template <class H, class V>
static int resize_crop_px4(const char* who, H h_kernel, V v_kernel, const void* raw_dev, const void* jobs_dev, int njobs, int max_rows,
                           const int32_t* coef_dev, int n_px, void* out_dev, void* scratch_dev, void* stream) {
    if (njobs == 0) return 0;
    if (!raw_dev || !jobs_dev || !coef_dev || !out_dev || !scratch_dev || njobs < 0 || n_px < 1 || n_px > 4096 || max_rows < 1)
        return set_err(CLIPMI_EINVAL, "%s: bad arguments", who);
    hipStream_t st = as_stream(stream);
    const long long per_h = (long long)max_rows * n_px, per_v = (long long)n_px * n_px;
    hipLaunchKernelGGL(h_kernel, dim3((unsigned)((per_h + 255) / 256), (unsigned)njobs), dim3(256), 0, st,
                       static_cast<const unsigned char*>(raw_dev), static_cast<const ResizeJob*>(jobs_dev), coef_dev, n_px,
                       static_cast<unsigned char*>(scratch_dev));
    CLIPMI_CHECK_LAUNCH("resize_h_px4");
    hipLaunchKernelGGL(v_kernel, dim3((unsigned)((per_v + 255) / 256), (unsigned)njobs), dim3(256), 0, st,
                       static_cast<const ResizeJob*>(jobs_dev), coef_dev, n_px, static_cast<const unsigned char*>(scratch_dev),
                       static_cast<unsigned char*>(out_dev));
    CLIPMI_CHECK_LAUNCH("resize_v_px4");
    return 0;
}

extern "C" int clipmi_resize_crop_rgba8(const void* raw_dev, const void* jobs_dev, int njobs, int max_rows, const int32_t* coef_dev,
                                        int n_px, void* out_dev, void* scratch_dev, void* stream) {
    return resize_crop_px4("resize_crop_rgba8", resize_h_rgba_kernel, resize_v_rgba_kernel, raw_dev, jobs_dev, njobs, max_rows, coef_dev,
                           n_px, out_dev, scratch_dev, stream);
}

extern "C" int clipmi_resize_crop_cmyk8(const void* raw_dev, const void* jobs_dev, int njobs, int max_rows, const int32_t* coef_dev,
                                        int n_px, void* out_dev, void* scratch_dev, void* stream) {
    return resize_crop_px4("resize_crop_cmyk8", resize_h_cmyk_kernel, resize_v_cmyk_kernel, raw_dev, jobs_dev, njobs, max_rows, coef_dev,
                           n_px, out_dev, scratch_dev, stream);
}

extern "C" int clipmi_nearest_crop_p8(const void* raw_dev, const void* jobs_dev, int njobs, const void* tabs_dev, int n_px,
                                      void* out_dev, void* stream) {
    static_assert(sizeof(NearestJob) == sizeof(clipmi_nearest_job) && sizeof(NearestJob) == 48, "clipmi_nearest_job layout");
    if (njobs == 0) return 0;
    if (!raw_dev || !jobs_dev || !tabs_dev || !out_dev || njobs < 0 || n_px < 1 || n_px > 4096 || (reinterpret_cast<uintptr_t>(tabs_dev) & 3))
        return set_err(CLIPMI_EINVAL, "nearest_crop_p8: bad arguments");
    const long long per = (long long)n_px * n_px;
    hipLaunchKernelGGL(nearest_p8_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)njobs), dim3(256), 0, as_stream(stream),
                       static_cast<const unsigned char*>(raw_dev), static_cast<const NearestJob*>(jobs_dev),
                       static_cast<const unsigned char*>(tabs_dev), n_px, static_cast<unsigned char*>(out_dev));
    CLIPMI_CHECK_LAUNCH("nearest_p8_kernel");
    return 0;
}
