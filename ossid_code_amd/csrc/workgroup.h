// Workgroup primitives of the scalar / LDS side, each stated once: scans, the bitonic sort, the bounding box.
// (The matrix-core side's shared pieces are in mfma.h, the wave reductions in common.h.)
#pragma once
#include "common.h"

struct OpAdd {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// 64-lane inclusive scans (lane i ends with op over lanes 0..i, or i..63 for the suffix form)
template <class T, class Op>
__device__ __forceinline__ T wave_scan_up(T v, Op op, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T w = __shfl_up(v, d);
        if (lane >= d) v = op(w, v);
    }
    return v;
}
template <class T, class Op>
__device__ __forceinline__ T wave_scan_down(T v, Op op, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T w = __shfl_down(v, d);
        if (lane + d < 64) v = op(v, w);
    }
    return v;
}
// Workgroup scans of one value per thread, NW waves. `lds` holds NW values. Return the EXCLUSIVE result (op over the threads
// before / after this one, `id` for none) and set `total` in every thread. Two barriers: lds may be reused after the call.
template <int NW, class T, class Op>
__device__ __forceinline__ T block_scan_excl(T v, Op op, T id, T* lds, T& total, bool reverse) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const T inc = reverse ? wave_scan_down(v, op, lane) : wave_scan_up(v, op, lane);
    if (lane == (reverse ? 0 : 63)) lds[wv] = inc;
    __syncthreads();
    T before = id, all = id;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const T x = lds[w];
        all = op(all, x);
        if (reverse ? w > wv : w < wv) before = op(before, x);
    }
    __syncthreads();
    total = all;
    const T nb = reverse ? __shfl_down(inc, 1) : __shfl_up(inc, 1);           // the neighbour's inclusive value
    const bool edge = reverse ? lane == 63 : lane == 0;
    return edge ? before : op(before, nb);
}

// Exclusive sums of in[0 .. n) by one workgroup of NW waves: each thread sums a contiguous segment, the segment sums are
// scanned, and put(i, offset of element i) is called for every i in the thread's segment, in index order. in[i] is read
// again just before put(i, .), so put may overwrite it. Returns the total in every thread. `lds` as for block_scan_excl.
template <int NW, class T, class I, class Put>
__device__ __forceinline__ T wg_scan_range(const T* in, I n, T* lds, Put put) {
    const I per = (n + (64 * NW - 1)) / (64 * NW), a0 = (I)threadIdx.x * per, a = a0 < n ? a0 : n, b = a + per < n ? a + per : n;
    T sum = 0;
    for (I i = a; i < b; ++i) sum += in[i];
    T total;
    T run = block_scan_excl<NW>(sum, OpAdd(), (T)0, lds, total, false);
    for (I i = a; i < b; ++i) {
        const T v = in[i];
        put(i, run);
        run += v;
    }
    return total;
}

// Ascending bitonic sort of keys[0 .. n) in LDS by the whole workgroup; n a power of two >= 2, any blockDim. The caller
// has a barrier between writing the keys and the call; the sort ends with one. Pair-indexed: each step is n / 2
// compare-exchanges, pair t on elements i = 2t - (t mod stride) and i + stride, so no thread idles behind a partner test.
__device__ __forceinline__ void wg_bitonic_sort(unsigned long long* keys, int n) {
    for (int size = 2; size <= n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += blockDim.x) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long a = keys[i], b = keys[j];
                const bool up = (i & size) == 0;
                if ((a > b) == up) keys[i] = b, keys[j] = a;
            }
            __syncthreads();
        }
}

// Bounding box of a point set: in, each thread's own minima / maxima (FLT_MAX / -FLT_MAX for none); out, the workgroup's,
// valid in every thread of wave 0. The order of the fminf / fmaxf applications is fixed -- the xor butterfly inside each
// wave, then waves 1 .. NW-1 folded onto wave 0 in index order -- because -0 / +0 and NaN operands make it observable and
// the boxes feed bit-pinned cell coordinates. One barrier; `lds` holds NW x 6 floats.
template <int NW>
__device__ __forceinline__ void wg_bbox3(float (&mn)[3], float (&mx)[3], float (*lds)[6]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int m = 32; m >= 1; m >>= 1) mn[a] = fminf(mn[a], __shfl_xor(mn[a], m)), mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], m));
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) lds[wv][a] = mn[a], lds[wv][3 + a] = mx[a];
    __syncthreads();
    if (wv != 0) return;
    for (int w = 1; w < NW; ++w)
        for (int a = 0; a < 3; ++a) mn[a] = fminf(mn[a], lds[w][a]), mx[a] = fmaxf(mx[a], lds[w][3 + a]);
}
