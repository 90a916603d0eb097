// Shared device/host helpers for libossid_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ossid_hip.h"


static inline int ossid_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? OSSID_OK : OSSID_ELAUNCH;
}

// workgroups of 256 threads for a grid-stride kernel over `work` elements
static inline int grid_for(size_t work) { return (int)((work + 255) / 256 < 8192 ? (work + 255) / 256 : 8192); }

// ELU(alpha = 1) without libm's expm1f (~40 vector instructions per value -- 160 M of them per test-time frame in the head's
// convolution epilogues: ~0.13 ms of vector-ALU time): a degree-7 Taylor polynomial near zero, where exp(x) - 1 would cancel,
// and the hardware exponential elsewhere; relative error < 1e-6 (tests/test_dtoid_gpu.py holds it against torch's ELU).
#ifdef __HIPCC__
__device__ __forceinline__ float elu_fast(float x) {
#ifdef OSSID_ELU_LIBM            // (A/B and reference build: libm's expm1f)
    return x > 0.0f ? x : expm1f(x);
#endif
    const float xm = fminf(x, 0.0f);
    float p = 1.0f / 5040.0f;
    p = fmaf(p, xm, 1.0f / 720.0f);
    p = fmaf(p, xm, 1.0f / 120.0f);
    p = fmaf(p, xm, 1.0f / 24.0f);
    p = fmaf(p, xm, 1.0f / 6.0f);
    p = fmaf(p, xm, 0.5f);
    p = fmaf(p, xm, 1.0f);
    const float near0 = p * xm, far = __expf(xm) - 1.0f;
    const float neg = xm > -0.35f ? near0 : far;
    return x > 0.0f ? x : neg;
}
#endif

// csrc/wgrad_fc.hip: the decoder's few-channel 3x3 weight gradients from 2-D pixel tiles (internal: reached through
// ossid_conv_wgrad / ossid_conv_wgrad_workspace_bytes of csrc/train.hip)
bool ossid_wgrad_fewch_takes(int Cin, int Cout, int taps, int in_cs, int dy_cs);
size_t ossid_wgrad_fewch_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ossid_wgrad_fewch(const ossid_wgrad_desc* d, void* stream);

// csrc/wgrad_t9.hip: plain 3x3 weight gradients with input channels in 128s (the dense blocks' 128 -> 32, the head's layers) from
// 2-D pixel tiles, all taps from one staged patch (internal: reached through ossid_conv_wgrad(_group) and their workspace queries)
bool ossid_wgrad_t9_takes(const ossid_wgrad_desc* d);
int ossid_wgrad_t9_class(const ossid_wgrad_desc* d);      // problems of one ossid_wgrad_t9_group call share it (and the geometry)
size_t ossid_wgrad_t9_workspace_bytes(const ossid_wgrad_desc* descs, int n);
int ossid_wgrad_t9_group(const ossid_wgrad_desc* descs, int n, void* workspace, size_t workspace_bytes, void* stream);
// ... and the dense layers' 1x1 convolution (c -> 128) in blocks of 256 input channels ("jobs": at most
// ossid_wgrad_t1_max_jobs() per call, ossid_wgrad_t1_job_count says how many a list makes)
bool ossid_wgrad_t1_takes(const ossid_wgrad_desc* d);
int ossid_wgrad_t1_max_jobs(void);
int ossid_wgrad_t1_job_count(const ossid_wgrad_desc* descs, int n);
size_t ossid_wgrad_t1_workspace_bytes(const ossid_wgrad_desc* descs, int n);
int ossid_wgrad_t1_group(const ossid_wgrad_desc* descs, int n, void* workspace, size_t workspace_bytes, void* stream);

// Kernels that declare more dynamic LDS than the default limit need hipFuncAttributeMaxDynamicSharedMemorySize. It is a
// property of the FUNCTION, not of a launch: raise it to the hardware maximum ONCE per (function, device), the first
// time the function is launched (always a warm-up pass, never inside a stream capture), instead of before every launch.
// Round 1 set it per launch -- also from inside torch.cuda.graph captures, where a rocprofv3-traced run segfaulted in the
// launch path ("capture under the profiler").
struct OssidLdsAttr {
    int done[16];
};
static inline int ossid_ensure_dyn_lds(const void* fn, size_t bytes, OssidLdsAttr& st) {
    if (bytes <= 48 * 1024) return OSSID_OK;
    if (bytes > 160 * 1024) return OSSID_EINVAL;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return OSSID_ELAUNCH;
    dev &= 15;
    if (__atomic_load_n(&st.done[dev], __ATOMIC_ACQUIRE)) return OSSID_OK;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        (void)hipGetLastError();   // reported through the return value; not left behind for the caller's next HIP call
        return OSSID_ELAUNCH;
    }
    __atomic_store_n(&st.done[dev], 1, __ATOMIC_RELEASE);
    return OSSID_OK;
}
#define OSSID_ENSURE_LDS(kern, bytes)                                             \
    do {                                                                          \
        static OssidLdsAttr ossid_lds_attr_;                                      \
        const int rc_ = ossid_ensure_dyn_lds((const void*)(kern), (bytes), ossid_lds_attr_); \
        if (rc_ != OSSID_OK) return rc_;                                          \
    } while (0)

// Persistent grids: as many workgroups of 256 as are resident at once -- workgroups per CU x CUs, asked of the runtime once
// per kernel and kept in *cache (0 = not asked yet) -- each looping over its share of the tiles. dyn_lds: the kernel's dynamic
// LDS bytes (0: none, and no attribute call); cap_per_cu: at most so many workgroups per CU (0: no cap); fallback: the answer
// while the runtime cannot be asked (nothing is cached then). Workspace sizes follow from these grids.
template <typename K>
int persistent_grid(K kern, int dyn_lds, int cap_per_cu, int fallback, int* cache) {
    if (!*cache) {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess ||
            (dyn_lds && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, dyn_lds) != hipSuccess) ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, dyn_lds) != hipSuccess || per_cu <= 0)
            return fallback;
        if (cap_per_cu && per_cu > cap_per_cu) per_cu = cap_per_cu;
        *cache = per_cu * p.multiProcessorCount;
    }
    return *cache;
}

// the direct convolutions' default arithmetic: 1 = split-bf16 operands, 0 = the exact-f32 instruction (formats: csrc/pack.hip)
#ifdef OSSID_CONV_F32
#define OSSID_CONV_SB 0
#else
#define OSSID_CONV_SB 1
#endif
// 64-lane wave reductions (xor butterfly; every lane ends with the result)
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double w = __shfl_xor(v, m);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ bool fin(double v) { return fabs(v) < INFINITY; }     // false for NaN and +-inf

// a device-side element count whose producer reports overflow by leaving it above the capacity: nothing is processed then
__device__ __forceinline__ int count_or_0(const int32_t* count, int cap) { return count[0] <= cap ? count[0] : 0; }
