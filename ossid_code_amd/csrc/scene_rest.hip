// Objects at rest on a table (SPEC.md 13.16-13.18): the support heights a mesh's resting orientations are found from, and
// the height-field drop that stacks a scene's objects on the table plane. scenes.MeshAtlas.resting and
// scenes.sample_layouts(placement="rest") are the callers. No solver, no iteration, no random numbers, no float atomics:
// every result is a maximum, so it does not depend on the order of arrival and equals the numpy restatement
// (tests/ref_scene_rest.py) bit for bit.
//
// ossid_mesh_support, one launch: a workgroup of 256 threads takes SUP_DIRS directions and walks every vertex, each thread
//   keeping SUP_DIRS running maxima of ((dx x + dy y) + dz z) in f64; the waves' maxima meet in LDS. No atomic, no clear:
//   every h[d] is written once.
// ossid_scene_drop, one launch: a workgroup of DROP_THREADS threads per scene holds the scene's height field in LDS as
//   the bits of non-negative floats and places the instances one after another. Per instance two walks over its
//   triangles, one per thread and round: pass 1 finds the offset (a maximum of f64 differences), pass 2 raises the field
//   under the triangle's bounding box (an integer maximum on the bits). A box of more than DROP_COOP cells is walked by
//   the whole wave, lane by cell, instead of by its one lane -- the table-sized triangles of a coarse mesh at G = 128
//   would otherwise keep one lane busy for 16 384 cells.
// The draw list is device data the kernel does not trust: an index that leads outside an array places nothing.
#include <cmath>

#include "common.h"

namespace {

constexpr int SUP_DIRS = 8;
constexpr int DROP_THREADS = 1024;
constexpr int DROP_WAVES = DROP_THREADS / 64;
constexpr int DROP_COOP = 32;

__global__ __launch_bounds__(256) void support_kernel(const float* __restrict__ vertices, int V,
                                                      const double* __restrict__ dirs, int D, double* __restrict__ h) {
    __shared__ double part[4][SUP_DIRS];
    const int d0 = blockIdx.x * SUP_DIRS;
    double dx[SUP_DIRS], dy[SUP_DIRS], dz[SUP_DIRS], m[SUP_DIRS];
#pragma unroll
    for (int k = 0; k < SUP_DIRS; ++k) {
        const int d = d0 + k < D ? d0 + k : D - 1;        // the last group repeats its last direction; only k < D - d0 is stored
        dx[k] = dirs[3 * (size_t)d], dy[k] = dirs[3 * (size_t)d + 1], dz[k] = dirs[3 * (size_t)d + 2];
        m[k] = -INFINITY;
    }
    for (int v = threadIdx.x; v < V; v += 256) {
        const float xf = vertices[3 * (size_t)v], yf = vertices[3 * (size_t)v + 1], zf = vertices[3 * (size_t)v + 2];
        if (!(fabsf(xf) < INFINITY && fabsf(yf) < INFINITY && fabsf(zf) < INFINITY)) continue;
        const double x = (double)xf, y = (double)yf, z = (double)zf;
#pragma unroll
        for (int k = 0; k < SUP_DIRS; ++k) {
            const double t = (dx[k] * x + dy[k] * y) + dz[k] * z;
            m[k] = t > m[k] ? t : m[k];
        }
    }
#pragma unroll
    for (int k = 0; k < SUP_DIRS; ++k) {
        const double w = wave_max_f64(m[k]);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    if (threadIdx.x < SUP_DIRS && d0 + (int)threadIdx.x < D) {
        double w = part[0][threadIdx.x];
#pragma unroll
        for (int j = 1; j < 4; ++j) w = part[j][threadIdx.x] > w ? part[j][threadIdx.x] : w;
        h[d0 + threadIdx.x] = w;
    }
}

// v >= 0 (or +inf) to the nearest f32 at or above it
__device__ __forceinline__ float round_up_f32(double v) {
    const float f = (float)v;
    return (double)f < v ? __int_as_float(__float_as_int(f) + 1) : f;      // f >= 0 and finite here: the next float up
}

__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double w = __shfl_xor(v, m);
        v = w < v ? w : v;
    }
    return v;
}

// One triangle of an instance in the table frame: its box of cells clipped to the grid (empty when x0 > x1 or y0 > y1),
// whether a cell of the unclipped box lies outside the grid, and its lowest and highest z'.
struct DropTri {
    bool usable, outside;
    int x0, x1, y0, y1;
    double zmin, zmax;
};

__device__ __forceinline__ double min3(double a, double b, double c) {
    const double m = b < a ? b : a;
    return c < m ? c : m;
}
__device__ __forceinline__ double max3(double a, double b, double c) {
    const double m = b > a ? b : a;
    return c > m ? c : m;
}

// floor((lo - x0) / cell) and floor((hi - x0) / cell) clipped to [0, G - 1] while still doubles: a far vertex or a tiny cell
// makes an index no int holds. lo <= hi are finite, so neither quotient is NaN (x0 may be -inf: both are then +inf).
__device__ __forceinline__ void cell_range(double lo, double hi, double x0, double cell, int G, int& a, int& b, bool& outside) {
    const double fa = floor((lo - x0) / cell), fb = floor((hi - x0) / cell);
    const double top = (double)(G - 1);
    outside = outside || fa < 0.0 || fb > top;
    if (fb < 0.0 || fa > top) {
        a = 0, b = -1;
        return;
    }
    a = (int)(fa < 0.0 ? 0.0 : fa);
    b = (int)(fb > top ? top : fb);
}

__device__ __forceinline__ DropTri drop_tri(const float* __restrict__ vertices, const int32_t* __restrict__ faces, int v0,
                                            int nv, int f0, int f, const double* L, double x0, double cell, int G) {
    DropTri t = {};
    const int32_t* fp = faces + 3 * (size_t)(f0 + f);
    const unsigned i0 = (unsigned)fp[0], i1 = (unsigned)fp[1], i2 = (unsigned)fp[2];
    if (!(i0 < (unsigned)nv && i1 < (unsigned)nv && i2 < (unsigned)nv)) return t;      // never read outside the mesh's vertices
    double p[3][3];
    const unsigned idx[3] = {i0, i1, i2};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* vp = vertices + 3 * (size_t)(v0 + (int)idx[j]);
        const double x = (double)vp[0], y = (double)vp[1], z = (double)vp[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[j][c] = ((L[4 * c] * x + L[4 * c + 1] * y) + L[4 * c + 2] * z) + L[4 * c + 3];
            ok = ok && fin(p[j][c]);
        }
    }
    if (!ok) return t;
    t.usable = true;
    t.zmin = min3(p[0][2], p[1][2], p[2][2]);
    t.zmax = max3(p[0][2], p[1][2], p[2][2]);
    cell_range(min3(p[0][0], p[1][0], p[2][0]), max3(p[0][0], p[1][0], p[2][0]), x0, cell, G, t.x0, t.x1, t.outside);
    cell_range(min3(p[0][1], p[1][1], p[2][1]), max3(p[0][1], p[1][1], p[2][1]), x0, cell, G, t.y0, t.y1, t.outside);
    if (t.x0 > t.x1 || t.y0 > t.y1) t.x0 = 0, t.x1 = -1, t.y0 = 0, t.y1 = -1;
    return t;
}

// Calls fn(cell index, zmin, zmax) for every in-grid cell of the wave's 64 triangles: a small box by its own lane, a large
// one by all lanes. Every lane of the wave must arrive.
template <typename Fn>
__device__ __forceinline__ void drop_cells(const DropTri& t, int G, Fn fn) {
    const int lane = threadIdx.x & 63;
    const int w = t.usable ? t.x1 - t.x0 + 1 : 0, n = t.usable ? w * (t.y1 - t.y0 + 1) : 0;
    if (n > 0 && n <= DROP_COOP)
        for (int y = t.y0; y <= t.y1; ++y)
            for (int x = t.x0; x <= t.x1; ++x) fn(y * G + x, t.zmin, t.zmax);
    unsigned long long big = __ballot(n > DROP_COOP);
    while (big) {
        const int src = __ffsll((long long)big) - 1;
        big &= big - 1;
        const int bx = __shfl(t.x0, src), by = __shfl(t.y0, src), bw = __shfl(w, src), bn = __shfl(n, src);
        const double zlo = __shfl(t.zmin, src), zhi = __shfl(t.zmax, src);
        for (int k = lane; k < bn; k += 64) fn((by + k / bw) * G + bx + k % bw, zlo, zhi);
    }
}

__global__ __launch_bounds__(DROP_THREADS) void drop_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ meshes, int Vt, int Ft, int K,
                                                            const int32_t* __restrict__ instance_mesh,
                                                            const int32_t* __restrict__ scene_first,
                                                            const double* __restrict__ local, int I, int G, double cell,
                                                            double* __restrict__ drop, int32_t* __restrict__ status,
                                                            float* __restrict__ height_out) {
    extern __shared__ __align__(16) unsigned char lds[];
    double* red_off = (double*)lds;                        // [DROP_WAVES] per-wave maxima of pass 1
    double* red_low = red_off + DROP_WAVES;                // [DROP_WAVES] per-wave minima of zmin
    int* red_flag = (int*)(red_low + DROP_WAVES);          // [DROP_WAVES] bit 0: a usable triangle, bit 1: a cell outside
    int* H = red_flag + DROP_WAVES;                        // [G][G] the bits of non-negative floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int scene = blockIdx.x;
    const int cells = G * G;
    const double x0 = -((double)G * 0.5) * cell;
    for (int k = tid; k < cells; k += DROP_THREADS) H[k] = 0;
    int first = scene_first[scene], last = scene_first[scene + 1];
    if (first < 0 || last > I || first > last) first = last = 0;
    __syncthreads();
    for (int i = first; i < last; ++i) {                   // i, and everything read through it, is the workgroup's
        const int m = instance_mesh[i];
        int v0 = 0, nv = 0, f0 = 0, nf = 0;
        if (m >= 0 && m < K) {
            v0 = meshes[4 * m], nv = meshes[4 * m + 1], f0 = meshes[4 * m + 2], nf = meshes[4 * m + 3];
            if (v0 < 0 || nv < 0 || nv > Vt - v0 || f0 < 0 || nf < 0 || nf > Ft - f0) nf = 0;
        }
        double L[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) L[k] = local[12 * (size_t)i + k];
        // pass 1: the offset
        double off = -INFINITY, low = INFINITY;
        int flag = 0;
        for (int base = 0; base < nf; base += DROP_THREADS) {
            DropTri t = {};
            if (base + tid < nf) t = drop_tri(vertices, faces, v0, nv, f0, base + tid, L, x0, cell, G);
            if (t.usable) {
                flag |= t.outside ? 3 : 1;
                low = t.zmin < low ? t.zmin : low;
            }
            drop_cells(t, G, [&](int c, double zlo, double) {
                const double d = (double)__int_as_float(H[c]) - zlo;
                off = d > off ? d : off;
            });
        }
        off = wave_max_f64(off);
        low = wave_min_f64(low);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) flag |= __shfl_xor(flag, s);
        if (lane == 0) red_off[wave] = off, red_low[wave] = low, red_flag[wave] = flag;
        __syncthreads();
        for (int w = 0; w < DROP_WAVES; ++w) {
            off = red_off[w] > off ? red_off[w] : off;
            low = red_low[w] < low ? red_low[w] : low;
            flag |= red_flag[w];
        }
        const bool any = (flag & 1) != 0;
        off = -low > off ? -low : off;
        if (tid == 0) {
            drop[i] = any ? off : 0.0;
            status[i] = any ? ((flag & 2) ? 2 : 0) : 1;
        }
        // pass 2: the field under the object rises to its top
        if (any)
            for (int base = 0; base < nf; base += DROP_THREADS) {
                DropTri t = {};
                if (base + tid < nf) t = drop_tri(vertices, faces, v0, nv, f0, base + tid, L, x0, cell, G);
                drop_cells(t, G, [&](int c, double, double zhi) {
                    const int v = __float_as_int(round_up_f32(zhi + off));          // zhi + off >= 0: the bits order as ints
                    if (v > H[c]) atomicMax(&H[c], v);
                });
            }
        __syncthreads();                                   // before the next instance reads H and rewrites the scratch
    }
    if (height_out)
        for (int k = tid; k < cells; k += DROP_THREADS) height_out[(size_t)scene * cells + k] = __int_as_float(H[k]);
}

}  // namespace

extern "C" {

int ossid_mesh_support(const float* vertices, int V, const double* dirs, int D, double* h_out, void* stream) {
    if (!vertices || !dirs || !h_out || V < 1 || V > OSSID_RASTER_MAX_VERTICES || D < 1 || D > OSSID_REST_MAX_DIRS)
        return OSSID_EINVAL;
    hipLaunchKernelGGL(support_kernel, dim3((unsigned)((D + SUP_DIRS - 1) / SUP_DIRS)), dim3(256), 0, (hipStream_t)stream,
                       vertices, V, dirs, D, h_out);
    return ossid_launch_status();
}

int ossid_scene_drop(const float* vertices, const int32_t* faces, const int32_t* meshes, int Vt, int Ft, int K,
                     const int32_t* instance_mesh, const int32_t* scene_first, const double* local, int I, int S, int G,
                     double cell, double* drop, int32_t* status, float* height_out, void* stream) {
    if (!vertices || !meshes || !scene_first || S < 1 || S > OSSID_SCENE_MAX_SCENES || I < 0 ||
        I > S * OSSID_SCENE_MAX_INSTANCES || K < 1 || Vt < 1 || Vt > (1 << 29) || Ft < 0 || Ft > (1 << 29) || (Ft > 0 && !faces) ||
        G < 1 || G > OSSID_REST_MAX_GRID || !(cell > 0.0) || !(cell < INFINITY) ||
        (I > 0 && (!instance_mesh || !local || !drop || !status)))
        return OSSID_EINVAL;
    const size_t lds = (size_t)DROP_WAVES * (8 + 8 + 4) + (size_t)G * G * 4;
    OSSID_ENSURE_LDS(drop_kernel, lds);
    hipLaunchKernelGGL(drop_kernel, dim3((unsigned)S), dim3(DROP_THREADS), lds, (hipStream_t)stream, vertices, faces, meshes, Vt,
                       Ft, K, instance_mesh, scene_first, local, I, G, cell, drop, status, height_out);
    return ossid_launch_status();
}

}  // extern "C"
