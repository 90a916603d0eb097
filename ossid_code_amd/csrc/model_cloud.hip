// The scorer's model cloud from the object's mesh (SPEC.md section 9): what scripts/online_learning.py:303-311 loads from
// zephyr_model_data/{lmo,ycbv}/model_cloud_XX.npz, a file made by a zephyr script that is in neither tree. This build's own
// definition; parity with zephyr's clouds is unpinned. Every reduction below is over integers or a max / min, so every
// output is bit-reproducible and equal to the numpy restatement tests/ref_model_cloud.py.
//
// ossid_cloud_votes (9.2)       grid (pixel tiles, views). A lane takes one sample of the rasteriser's face-id image. Runs of
//                               one face along a wave are found with one shuffle and one ballot; only the first lane of a run
//                               loads the triangle, decides the side in f64 and adds the run's length with ONE integer
//                               atomicAdd (a wave never straddles two views, so the side is the run's).
// ossid_cloud_weights (9.3)     face areas in f64, their maximum by atomicMax on the double's bits (areas are >= 0: the bits
//                               order like the values), the 32.32 fixed-point weights, and their inclusive prefix sum in three
//                               launches (4096 faces per workgroup, at most 1024 workgroups, one workgroup scans the totals).
// ossid_cloud_candidates (9.4)  one thread per candidate: stratified position in the prefix sums, binary search, barycentric
//                               coordinates from the integer R2 sequence, all in f64.
// ossid_cloud_candidates_textured (9.4.1)  the same kernel with the colour taken from a UV texture at one mip level.
// ossid_cloud_fps (9.5)         ONE workgroup of 1024 threads. Lane t owns candidates t, t + 1024, ...: at most 32, their
//                               coordinates in registers (96 VGPRs of the 128 a wave has at 4 waves per SIMD), their running
//                               minimum distances in LDS (128 KiB of the CU's 160: registers cannot hold both), conflict-free
//                               (consecutive lanes, consecutive words). Per round: the distance pass, a wave maximum of the key
//                               (bits(tmp) << 32) | ~index by six shuffles, the 16 wave winners with their coordinates through
//                               a double-buffered LDS slot, one barrier. The winner's coordinates travel with the key, so no
//                               round waits for global memory.
// ossid_mesh_diameter (9.6)     all pairs in tiles of 256 x 1024, f64, the upper triangle of tiles only, atomicMax on the bits.
#include <cmath>

#include "texture.h"
#include "workgroup.h"

namespace {

constexpr int SCAN_ITEMS = 16;                        // faces per thread of the scan
constexpr int SCAN_BLOCK = 256 * SCAN_ITEMS;          // faces per workgroup: OSSID_RASTER_MAX_FACES / 4096 = 1024 totals
constexpr int FPS_THREADS = 1024;
constexpr int DIAM_TJ = 1024;

struct Tri {
    double p[3][3];
    bool ok;                                          // the three indices lie in [0, V)
};

__device__ __forceinline__ Tri load_tri(const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int f) {
    Tri t;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    t.ok = i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
    const int idx[3] = {t.ok ? i0 : 0, t.ok ? i1 : 0, t.ok ? i2 : 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) t.p[a][c] = (double)vertices[3 * (size_t)idx[a] + c];
    return t;
}

// g = (p1 - p0) x (p2 - p0), each component a b - c d
__device__ __forceinline__ void tri_normal(const Tri& t, double g[3]) {
    const double ax = t.p[1][0] - t.p[0][0], ay = t.p[1][1] - t.p[0][1], az = t.p[1][2] - t.p[0][2];
    const double bx = t.p[2][0] - t.p[0][0], by = t.p[2][1] - t.p[0][1], bz = t.p[2][2] - t.p[0][2];
    g[0] = ay * bz - az * by;
    g[1] = az * bx - ax * bz;
    g[2] = ax * by - ay * bx;
}

// ---- 9.2 votes ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cloud_votes_kernel(const int32_t* __restrict__ face_id, int hw,
                                                          const float* __restrict__ vertices, int V,
                                                          const int32_t* __restrict__ faces, int F,
                                                          const double* __restrict__ centres, int32_t* __restrict__ votes) {
    const int view = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int f = i < hw ? face_id[(size_t)view * hw + i] : -1;
    if (f < 0 || f >= F) f = -1;
    const int prev = __shfl_up(f, 1);
    const bool start = lane == 0 || prev != f;
    const unsigned long long starts = __ballot(start);
    if (!start || f < 0) return;
    // the run ends before the next start above this lane
    const unsigned long long above = lane == 63 ? 0ull : (starts >> (lane + 1)) << (lane + 1);
    const int len = (above ? __ffsll((long long)above) - 1 : 64) - lane;
    const Tri t = load_tri(vertices, V, faces, f);
    if (!t.ok) return;
    double g[3];
    tri_normal(t, g);
    const double cx = centres[3 * view], cy = centres[3 * view + 1], cz = centres[3 * view + 2];
    const double s = (g[0] * (cx - t.p[0][0]) + g[1] * (cy - t.p[0][1])) + g[2] * (cz - t.p[0][2]);
    atomicAdd(votes + 2 * (size_t)f + (s >= 0.0 ? 0 : 1), len);
}

// ---- 9.3 weights ---------------------------------------------------------------------------------------------------------------
__global__ void cloud_zero_kernel(unsigned long long* __restrict__ a) { a[0] = 0ull; }

__global__ __launch_bounds__(256) void cloud_area_kernel(const float* __restrict__ vertices, int V,
                                                         const int32_t* __restrict__ faces, int F,
                                                         const int32_t* __restrict__ votes, double* __restrict__ area,
                                                         unsigned long long* __restrict__ amax) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    double A = 0.0;
    if (f < F) {
        const Tri t = load_tri(vertices, V, faces, f);
        double g[3];
        tri_normal(t, g);
        const double s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        const bool usable = t.ok && (votes[2 * (size_t)f] > 0 || votes[2 * (size_t)f + 1] > 0) && fin(s) && s > 0.0;
        A = usable ? sqrt(s) : 0.0;
        area[f] = A;
    }
    // A >= 0: the pattern orders like the value. One atomic per wave.
    unsigned long long b = (unsigned long long)__double_as_longlong(A);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(b, m);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicMax(amax, b);
}

__global__ __launch_bounds__(256) void cloud_weight_kernel(const float* __restrict__ vertices, int V,
                                                           const int32_t* __restrict__ faces, int F,
                                                           const int32_t* __restrict__ votes, const double* __restrict__ area,
                                                           const unsigned long long* __restrict__ amax,
                                                           unsigned long long* __restrict__ weights,
                                                           float* __restrict__ normals) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const double A = area[f];
    unsigned long long w = 0ull;
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (A > 0.0) {
        const double Amax = __longlong_as_double((long long)amax[0]);
        w = (unsigned long long)floor((A / Amax) * 4294967296.0);
        const Tri t = load_tri(vertices, V, faces, f);
        double g[3];
        tri_normal(t, g);
        const bool flip = votes[2 * (size_t)f + 1] > votes[2 * (size_t)f];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double q = g[c] / A;
            n[c] = (float)(flip ? -q : q);
        }
    }
    weights[f] = w;
    normals[3 * (size_t)f] = n[0], normals[3 * (size_t)f + 1] = n[1], normals[3 * (size_t)f + 2] = n[2];
}

// Inclusive sums of 64-bit integers. FINAL = false: totals[block] = the workgroup's sum. FINAL = true: out = the inclusive
// sums, offset by totals[block] (by then the exclusive sums of the totals).
template <bool FINAL>
__global__ __launch_bounds__(256) void cloud_scan_kernel(const unsigned long long* __restrict__ w, int F,
                                                         unsigned long long* __restrict__ totals,
                                                         unsigned long long* __restrict__ out) {
    __shared__ unsigned long long sh[4];
    const size_t base = (size_t)blockIdx.x * SCAN_BLOCK + (size_t)threadIdx.x * SCAN_ITEMS;
    unsigned long long v[SCAN_ITEMS], sum = 0ull;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = base + k < (size_t)F ? w[base + k] : 0ull;
        sum += v[k];
    }
    unsigned long long total;
    const unsigned long long before = block_scan_excl<4>(sum, OpAdd(), 0ull, sh, total, false);
    if (!FINAL) {
        if (threadIdx.x == 0) totals[blockIdx.x] = total;
        return;
    }
    unsigned long long run = totals[blockIdx.x] + before;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        run += v[k];
        if (base + k < (size_t)F) out[base + k] = run;
    }
}

// exclusive sums of at most 1024 totals, in place, one workgroup
__global__ __launch_bounds__(1024) void cloud_scan_totals_kernel(unsigned long long* __restrict__ totals, int n) {
    __shared__ unsigned long long sh[16];
    unsigned long long total;
    const unsigned long long before = block_scan_excl<16>((int)threadIdx.x < n ? totals[threadIdx.x] : 0ull, OpAdd(), 0ull, sh, total, false);
    if ((int)threadIdx.x < n) totals[threadIdx.x] = before;
}

// ---- 9.4 candidates --------------------------------------------------------------------------------------------------------------
// TEX = false: colors u8 [V][3], interpolated (9.4). TEX = true: uvs f32 [V][2] interpolated the same way, then one bilinear
// fetch at level lod of the mip chain (9.4.1; the sampler is texture.h's, shared with the textured rasteriser).
template <bool TEX>
__global__ __launch_bounds__(256) void cloud_candidates_kernel(const float* __restrict__ vertices, int V,
                                                               const int32_t* __restrict__ faces, int F,
                                                               const uint8_t* __restrict__ colors,
                                                               const float* __restrict__ uvs,
                                                               const unsigned* __restrict__ mips, int tex_h, int tex_w, int lod,
                                                               const int32_t* __restrict__ votes,
                                                               const unsigned long long* __restrict__ prefix,
                                                               const float* __restrict__ normals, int K,
                                                               float* __restrict__ pts, float* __restrict__ nrm,
                                                               float* __restrict__ col, int32_t* __restrict__ face) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const unsigned long long Wt = prefix[F - 1];
    float P[3] = {0.0f, 0.0f, 0.0f}, N[3] = {0.0f, 0.0f, 0.0f}, C[3] = {0.0f, 0.0f, 0.0f};
    int f = -1;
    if (Wt != 0ull) {
        const unsigned long long q = Wt / (unsigned long long)K, tau = q * (unsigned long long)k + (q >> 1);
        int lo = 0, hi = F - 1;                        // prefix[F-1] = Wt > tau: the answer exists
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (prefix[mid] > tau) hi = mid;
            else lo = mid + 1;
        }
        f = lo;
        const uint32_t r1 = (uint32_t)k * 3242174889u, r2 = (uint32_t)k * 2447445413u;
        double u = ((double)r1 + 0.5) / 4294967296.0, v = ((double)r2 + 0.5) / 4294967296.0;
        if (u + v > 1.0) u = 1.0 - u, v = 1.0 - v;
        const double w0 = (1.0 - u) - v;
        // a weighted face has its indices in [0, V) (9.3); the face is read in the orientation its votes gave it
        const bool flip = votes[2 * (size_t)f + 1] > votes[2 * (size_t)f];
        const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + (flip ? 2 : 1)], i2 = faces[3 * (size_t)f + (flip ? 1 : 2)];
        if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double a0 = (double)vertices[3 * (size_t)i0 + c], a1 = (double)vertices[3 * (size_t)i1 + c],
                             a2 = (double)vertices[3 * (size_t)i2 + c];
                P[c] = (float)((w0 * a0 + u * a1) + v * a2);
                if constexpr (!TEX) {
                    const double c0 = (double)colors[3 * (size_t)i0 + c], c1 = (double)colors[3 * (size_t)i1 + c],
                                 c2 = (double)colors[3 * (size_t)i2 + c];
                    double a = rint((w0 * c0 + u * c1) + v * c2);
                    a = a < 0.0 ? 0.0 : (a > 255.0 ? 255.0 : a);
                    C[c] = (float)a / 255.0f;
                }
                N[c] = normals[3 * (size_t)f + c];
            }
            if constexpr (TEX) {
                double t[2], q[3];
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    t[c] = (w0 * (double)uvs[2 * (size_t)i0 + c] + u * (double)uvs[2 * (size_t)i1 + c]) +
                           v * (double)uvs[2 * (size_t)i2 + c];
                tex_bilinear(tex_level(mips, tex_h, tex_w, lod), t[0], t[1], q);
#pragma unroll
                for (int c = 0; c < 3; ++c) C[c] = (float)tex_round_u8(q[c]) / 255.0f;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) pts[3 * (size_t)k + c] = P[c], nrm[3 * (size_t)k + c] = N[c], col[3 * (size_t)k + c] = C[c];
    face[k] = f;
}

// ---- 9.5 farthest-point sampling -----------------------------------------------------------------------------------------------
struct FpsSlot {
    unsigned long long key;
    float x, y, z, pad;
};

template <int PER>
__global__ __launch_bounds__(FPS_THREADS) void cloud_fps_kernel(const float* __restrict__ pts, int K, int M,
                                                                int32_t* __restrict__ selection, float* __restrict__ radius) {
    // tmp of candidate j * 1024 + tid lives in component j % 4 of tmp4[(j / 4) * 1024 + tid]: one 16-byte LDS access per four
    // candidates, consecutive lanes on consecutive 16 bytes
    constexpr int G = (PER + 3) / 4;
    __shared__ float4 tmp4[G * FPS_THREADS];
    __shared__ FpsSlot slot[2][FPS_THREADS / 64];
    const int tid = threadIdx.x, wv = tid >> 6;
    float x[PER], y[PER], z[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = j * FPS_THREADS + tid;
        const int ic = i < K ? i : K - 1;            // a slot past the end repeats the last point: no branch, no stray read
        // volatile: three independent 32-bit loads. Merged into one 96-bit load the coordinates become register triples,
        // and 32 triples plus the working set no longer fit the 128 registers without spilling
        const volatile float* vp = pts + 3 * (size_t)ic;
        x[j] = vp[0], y[j] = vp[1], z[j] = vp[2];
    }
    // ... and starts (and stays) at 0: among equal maxima the lowest index wins, and a real candidate is lower
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) t[c] = (4 * g + c) * FPS_THREADS + tid < K ? INFINITY : 0.0f;
        tmp4[g * FPS_THREADS + tid] = make_float4(t[0], t[1], t[2], t[3]);
    }
    float px = pts[0], py = pts[1], pz = pts[2];
    if (tid == 0) selection[0] = 0, radius[0] = INFINITY;
    for (int r = 1; r < M; ++r) {
        float bt = 0.0f, bx = 0.0f, by = 0.0f, bz = 0.0f;
        int bj = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float4 o4 = tmp4[g * FPS_THREADS + tid];
            float t[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = 4 * g + c;
                if (j < PER) {
                    const float dx = x[j] - px, dy = y[j] - py, dz = z[j] - pz;
                    const float d = (dx * dx + dy * dy) + dz * dz;
                    t[c] = d < t[c] ? d : t[c];
                    const bool take = j == 0 || t[c] > bt;     // strict: the lowest of the lane's own indices stays
                    bt = take ? t[c] : bt, bj = take ? j : bj, bx = take ? x[j] : bx, by = take ? y[j] : by, bz = take ? z[j] : bz;
                }
            }
            tmp4[g * FPS_THREADS + tid] = make_float4(t[0], t[1], t[2], t[3]);
            __builtin_amdgcn_sched_barrier(0);         // one group at a time: 32 values in flight do not fit the registers
        }
        const unsigned idx = (unsigned)(bj * FPS_THREADS + tid);
        const unsigned long long key = ((unsigned long long)__float_as_uint(bt) << 32) | (unsigned long long)(~idx);
        unsigned long long best = key;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(best, m);
            best = o > best ? o : best;
        }
        FpsSlot* s = slot[r & 1];
        if (key == best) s[wv].key = key, s[wv].x = bx, s[wv].y = by, s[wv].z = bz;      // keys are distinct: one lane
        __syncthreads();
        // two slots: a wave writes slot[r & 1] again in round r + 2, after the barrier of round r + 1, which every wave
        // reaches only when it has read round r's
        int win = 0;
        unsigned long long top = s[0].key;
#pragma unroll
        for (int w = 1; w < FPS_THREADS / 64; ++w) {
            const unsigned long long o = s[w].key;
            win = o > top ? w : win, top = o > top ? o : top;
        }
        // the pick is the same in every lane: keep it in scalar registers
        px = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s[win].x)));
        py = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s[win].y)));
        pz = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(s[win].z)));
        if (tid == 0) selection[r] = (int32_t)(~(unsigned)(top & 0xffffffffull)), radius[r] = __uint_as_float((unsigned)(top >> 32));
    }
}

// ---- 9.6 diameter ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_diameter_kernel(const float* __restrict__ vertices, int V,
                                                            unsigned long long* __restrict__ out) {
    const int i0 = blockIdx.x * 256, j0 = blockIdx.y * DIAM_TJ;
    if (j0 + DIAM_TJ <= i0) return;                    // the tile lies below the diagonal: its pairs are met transposed
    __shared__ double q[DIAM_TJ][3];
    const int nj = min(DIAM_TJ, V - j0);
    for (int e = threadIdx.x; e < 3 * nj; e += 256) (&q[0][0])[e] = (double)vertices[3 * (size_t)j0 + e];
    __syncthreads();
    const int i = i0 + threadIdx.x;
    double m = 0.0;
    if (i < V) {
        const double x = (double)vertices[3 * (size_t)i], y = (double)vertices[3 * (size_t)i + 1],
                     z = (double)vertices[3 * (size_t)i + 2];
        for (int j = 0; j < nj; ++j) {
            const double dx = x - q[j][0], dy = y - q[j][1], dz = z - q[j][2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            m = d > m ? d : m;
        }
    }
    unsigned long long b = (unsigned long long)__double_as_longlong(m);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(b, s);
        b = o > b ? o : b;
    }
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicMax(out, b);
}

__global__ void mesh_diameter_root_kernel(double* __restrict__ out) { out[1] = sqrt(out[0]); }

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

template <int PER>
void launch_fps(const float* points, int K, int M, int32_t* selection, float* radius, hipStream_t s) {
    hipLaunchKernelGGL(cloud_fps_kernel<PER>, dim3(1), dim3(FPS_THREADS), 0, s, points, K, M, selection, radius);
}

}  // namespace

extern "C" {

size_t ossid_cloud_workspace_bytes(int F) {
    if (F < 1 || F > OSSID_RASTER_MAX_FACES) return 0;
    return align8((size_t)F * 8) + 8 * (size_t)(1 + 1024);     // areas, the maximum, the scan's totals
}

int ossid_cloud_votes(const int32_t* face_id, int n, int H, int W, const float* vertices, int V, const int32_t* faces, int F,
                      const double* centres, int32_t* votes, void* stream) {
    if (!face_id || !vertices || !faces || !centres || !votes || n < 1 || H <= 0 || W <= 0 ||
        (long long)H * W > OSSID_RASTER_MAX_PIXELS || V < 1 || F < 1 || F > OSSID_RASTER_MAX_FACES || n > 65535)
        return OSSID_EINVAL;
    const int hw = H * W;
    hipLaunchKernelGGL(cloud_votes_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)n), dim3(256), 0, (hipStream_t)stream,
                       face_id, hw, vertices, V, faces, F, centres, votes);
    return ossid_launch_status();
}

int ossid_cloud_weights(const float* vertices, int V, const int32_t* faces, int F, const int32_t* votes, void* workspace,
                        size_t workspace_bytes, uint64_t* weights, uint64_t* prefix, float* normals, void* stream) {
    const size_t need = ossid_cloud_workspace_bytes(F);
    if (!vertices || !faces || !votes || !workspace || !weights || !prefix || !normals || V < 1 || need == 0 ||
        workspace_bytes < need || ((uintptr_t)workspace & 7))
        return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* area = (double*)workspace;
    unsigned long long* amax = (unsigned long long*)((char*)workspace + align8((size_t)F * 8));
    unsigned long long* totals = amax + 1;
    unsigned long long* w = (unsigned long long*)weights;
    const unsigned nb = (unsigned)((F + 255) / 256), ns = (unsigned)((F + SCAN_BLOCK - 1) / SCAN_BLOCK);
    hipLaunchKernelGGL(cloud_zero_kernel, dim3(1), dim3(1), 0, s, amax);
    hipLaunchKernelGGL(cloud_area_kernel, dim3(nb), dim3(256), 0, s, vertices, V, faces, F, votes, area, amax);
    hipLaunchKernelGGL(cloud_weight_kernel, dim3(nb), dim3(256), 0, s, vertices, V, faces, F, votes, area, amax, w, normals);
    hipLaunchKernelGGL(cloud_scan_kernel<false>, dim3(ns), dim3(256), 0, s, w, F, totals, (unsigned long long*)prefix);
    hipLaunchKernelGGL(cloud_scan_totals_kernel, dim3(1), dim3(1024), 0, s, totals, (int)ns);
    hipLaunchKernelGGL(cloud_scan_kernel<true>, dim3(ns), dim3(256), 0, s, w, F, totals, (unsigned long long*)prefix);
    return ossid_launch_status();
}

int ossid_cloud_candidates(const float* vertices, int V, const int32_t* faces, int F, const uint8_t* colors,
                           const int32_t* votes, const uint64_t* prefix, const float* normals, int K, float* points_out,
                           float* normals_out, float* colors_out, int32_t* face_out, void* stream) {
    if (!vertices || !faces || !colors || !votes || !prefix || !normals || !points_out || !normals_out || !colors_out ||
        !face_out || V < 1 || F < 1 || F > OSSID_RASTER_MAX_FACES || K < 1 || K > OSSID_CLOUD_MAX_CANDIDATES)
        return OSSID_EINVAL;
    hipLaunchKernelGGL(cloud_candidates_kernel<false>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       vertices, V, faces, F, colors, (const float*)nullptr, (const unsigned*)nullptr, 1, 1, 0, votes,
                       (const unsigned long long*)prefix, normals, K, points_out, normals_out, colors_out, face_out);
    return ossid_launch_status();
}

int ossid_cloud_candidates_textured(const float* vertices, int V, const int32_t* faces, int F, const float* uvs, const void* mips,
                                    size_t mip_bytes, int Ht, int Wt, int lod, const int32_t* votes, const uint64_t* prefix,
                                    const float* normals, int K, float* points_out, float* normals_out, float* colors_out,
                                    int32_t* face_out, void* stream) {
    const size_t tex = ossid_texture_mip_bytes(Ht, Wt);
    if (!vertices || !faces || !uvs || !mips || !votes || !prefix || !normals || !points_out || !normals_out || !colors_out ||
        !face_out || V < 1 || F < 1 || F > OSSID_RASTER_MAX_FACES || K < 1 || K > OSSID_CLOUD_MAX_CANDIDATES || tex == 0 ||
        mip_bytes < tex || ((uintptr_t)mips & 3) != 0 || lod < 0 || lod > tex_top_level(Ht, Wt))
        return OSSID_EINVAL;
    hipLaunchKernelGGL(cloud_candidates_kernel<true>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       vertices, V, faces, F, (const uint8_t*)nullptr, uvs, (const unsigned*)mips, Ht, Wt, lod, votes,
                       (const unsigned long long*)prefix, normals, K, points_out, normals_out, colors_out, face_out);
    return ossid_launch_status();
}

int ossid_cloud_fps(const float* points, int K, int M, int32_t* selection, float* radius, void* stream) {
    if (!points || !selection || !radius || M < 1 || M > OSSID_CLOUD_MAX_POINTS || K < M || K > OSSID_CLOUD_MAX_CANDIDATES)
        return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int per = (K + FPS_THREADS - 1) / FPS_THREADS;      // candidates per lane, rounded up to a power of two
    if (per <= 1) launch_fps<1>(points, K, M, selection, radius, s);
    else if (per <= 2) launch_fps<2>(points, K, M, selection, radius, s);
    else if (per <= 4) launch_fps<4>(points, K, M, selection, radius, s);
    else if (per <= 8) launch_fps<8>(points, K, M, selection, radius, s);
    else if (per <= 16) launch_fps<16>(points, K, M, selection, radius, s);
    else launch_fps<32>(points, K, M, selection, radius, s);
    return ossid_launch_status();
}

int ossid_mesh_diameter(const float* vertices, int V, double* out, void* stream) {
    if (!vertices || !out || V < 1 || V > OSSID_MESH_DIAMETER_MAX_VERTICES) return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cloud_zero_kernel, dim3(1), dim3(1), 0, s, (unsigned long long*)out);
    hipLaunchKernelGGL(mesh_diameter_kernel, dim3((unsigned)((V + 255) / 256), (unsigned)((V + DIAM_TJ - 1) / DIAM_TJ)), dim3(256),
                       0, s, vertices, V, (unsigned long long*)out);
    hipLaunchKernelGGL(mesh_diameter_root_kernel, dim3(1), dim3(1), 0, s, out);
    return ossid_launch_status();
}

}  // extern "C"
