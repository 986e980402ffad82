// common.hpp — shared host-side helpers for libclipmi.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include "../../include/clipmi.h"

namespace clipmi {

// thread-local last-error string behind clipmi_last_error()
char* err_buf();
int set_err(int code, const char* fmt, ...);

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// bump allocator over the caller's workspace
struct Arena {
    char* base;
    size_t cap, off;
    Arena(void* p, size_t bytes) : base(static_cast<char*>(p)), cap(bytes), off(0) {}
    template <typename T>
    T* take(size_t n) {
        off = align_up(off, 256);
        T* r = reinterpret_cast<T*>(base + off);
        off += n * sizeof(T);
        return r;
    }
    bool ok() const { return off <= cap; }
};

#define CLIPMI_CHECK_LAUNCH(what)                                                        \
    do {                                                                                 \
        hipError_t e__ = hipGetLastError();                                              \
        if (e__ != hipSuccess)                                                           \
            return clipmi::set_err(CLIPMI_EHIP, "%s: %s", what, hipGetErrorString(e__)); \
    } while (0)

// Development knobs. The CLIPMI_* environment variables that A/B runs and tools/ use exist only in the -DCLIPMI_DEV build
// (libclipmi_dev.so: cli-p_amd/build.py --dev); the product library reads no environment variable on any path, and the
// laboratory kernels (the wide scan's ablations and four-wave form, the folded-LayerNorm FP8 tower) are not compiled into it.
#ifdef CLIPMI_DEV
inline long long dev_knob(const char* name, long long dflt) { const char* e = getenv(name); return e && *e ? atoll(e) : dflt; }
#else
constexpr long long dev_knob(const char*, long long dflt) { return dflt; }
#endif

// resize.hip: resize_v_kernel over clipmi_resize_job records (the second pass of clipmi_resize_crop_rgb8)
int launch_resize_v_rgb8(const void* jobs_dev, int njobs, const int32_t* coef_dev, int n_px, const void* scratch_dev, void* out_dev,
                         hipStream_t st);

// Pillow's fixed point for resampling (Resample.c PRECISION_BITS = 32 - 8 - 2): a sum starts at 1 << (RZ_PREC - 1) and is clipped
// to 8 bits here. For resize.hip's passes and for jpeg.hip's fused horizontal pass, which runs in front of launch_resize_v_rgb8.
constexpr int RZ_PREC = 22;

__device__ __forceinline__ unsigned char rz_clip8(int v) {
    v >>= RZ_PREC;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

constexpr int NUM_CU = 256;           // MI355X
constexpr int LDS_BYTES = 160 * 1024; // per CU

// What an entry point has to clear, it clears with a KERNEL, not hipMemsetAsync: in a captured call the memset becomes a memset
// node, and a replay of clipmi_jpeg_decode_transform_rgb8 was seen to decode with its coefficient block still holding what the
// stream's previous kernel had filled the workspace with (every file status 4) - the kernel nodes of the same chain kept their
// order in every run (tests/test_graph_capture_gpu.py). A kernel also keeps a captured call a chain of kernel nodes only.
// [p, p + bytes) exactly; p and bytes multiples of 4 (of 16: 16-byte stores).
static __global__ void __launch_bounds__(256) zero16_kernel(uint4* __restrict__ p, size_t n16) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
static __global__ void __launch_bounds__(256) zero4_kernel(unsigned* __restrict__ p, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) p[i] = 0u;
}
inline hipError_t zero_async(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(p) | bytes) & 3) return hipErrorInvalidValue;
    const bool wide = ((reinterpret_cast<uintptr_t>(p) | bytes) & 15) == 0;
    const size_t n = bytes / (wide ? 16 : 4), want = (n + 255) / 256;
    const unsigned grid = (unsigned)(want < (size_t)NUM_CU * 8 ? want : (size_t)NUM_CU * 8);
    if (wide) hipLaunchKernelGGL(zero16_kernel, dim3(grid), dim3(256), 0, st, static_cast<uint4*>(p), n);
    else hipLaunchKernelGGL(zero4_kernel, dim3(grid), dim3(256), 0, st, static_cast<unsigned*>(p), n);
    return hipGetLastError();
}

}  // namespace clipmi
