// What the weight-gradient kernels (csrc/train.hip, wgrad_t9.hip, wgrad_fc.hip) share beyond the matrix-core pieces of mfma.h:
// the forward's input prologue and up-sampling index map, which a weight gradient must repeat operation for operation to be
// the gradient of that forward (csrc/conv.hip's stage map and stage_write call the same two functions), and the fixed-order
// sums of partial slabs. Everything is a forced-inline function over values: a kernel's staging arrays stay its own locals.
#pragma once
#include <hip/hip_runtime.h>

// per-channel affine (+ReLU) of four channels of one REAL pixel: a multiply, then an add (never fmaf: SPEC.md fixes the order).
// Zero padding is not part of it: the tiled and few-channel kernels select zero before the load, wgrad_t9.hip's multiply the
// result by a 0 / 1 factor. How ps / pt are loaded is the caller's too (wgrad_fc.hip's need not be 16-byte aligned).
__device__ __forceinline__ float4 prologue4(float4 v, const float4& ps, const float4& pt, bool has_pre, bool relu) {
    if (has_pre) {
        v.x = v.x * ps.x + pt.x, v.y = v.y * ps.y + pt.y, v.z = v.z * ps.z + pt.z, v.w = v.w * ps.w + pt.w;
        if (relu) v.x = fmaxf(v.x, 0.f), v.y = fmaxf(v.y, 0.f), v.z = fmaxf(v.z, 0.f), v.w = fmaxf(v.w, 0.f);
    }
    return v;
}

// fused nearest-neighbour up-sampling (F.interpolate(mode="nearest") in front of the convolution): row / column i of the
// [n_dst] image is read from the [n_src] source at min(floor(i * n_src / n_dst), n_src - 1), scale = (float)n_src / n_dst
__device__ __forceinline__ int nearest_src(int i, int n_src, int n_dst, float scale) {
    return n_src == n_dst ? i : min((int)floorf((float)i * scale), n_src - 1);
}

// ---- sums of partial slabs, in a fixed order (bit-reproducible, no float atomics). Two orders are in use, and both are part
// of the results: they are different floating-point sums.
// (1) ranges: a workgroup of 256 owns 32 outputs (threadIdx.x & 31), its 8 parts (threadIdx.x >> 5) each sum one of 8
// contiguous ranges of the slabs, 8 independent loads in flight, and part 0 adds the 8 range sums in ascending order. `at` is
// the element in slab 0, `stride` the floats between slabs; a thread with live == false loads nothing. Every thread of the
// workgroup must call it (barrier inside); the total is returned to part 0, the other parts get their own range's sum.
__device__ __forceinline__ float slab_sum_ranges(const float* at, size_t stride, int nslabs, bool live) {
    __shared__ float red[8][32];
    const int col = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int per = (nslabs + 7) / 8, g0 = part * per, g1 = min(nslabs, g0 + per);
    float s = 0.0f;
    if (live) {
        int g = g0;
        for (; g + 8 <= g1; g += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = at[(size_t)(g + u) * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; g < g1; ++g) s += at[(size_t)g * stride];
    }
    red[part][col] = s;
    __syncthreads();
    if (part != 0) return s;
    float t = red[0][col];
#pragma unroll
    for (int u = 1; u < 8; ++u) t += red[u][col];
    return t;
}
// (2) strided: part p of PARTS sums slabs p, p + PARTS, ..., 8 independent loads in flight. Only this walk is shared: how the
// PARTS sums are then combined is each kernel's own (see wgrad_reduce2_kernel and wgrad_reduce_group_kernel in train.hip).
template <int PARTS>
__device__ __forceinline__ float slab_sum_strided(const float* at, size_t stride, int nslabs, int part) {
    float s = 0.0f;
    int k = part;
    for (; k + 7 * PARTS < nslabs; k += 8 * PARTS) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = at[(size_t)(k + u * PARTS) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < nslabs; k += PARTS) s += at[(size_t)k * stride];
    return s;
}
