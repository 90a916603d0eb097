// Depth-only rasteriser of a triangle mesh at a batch of poses (SPEC.md section 7), the renderer of the per-frame loop:
// scripts/online_learning.py:485-493 (zephyr.utils.renderer.Renderer: addObject, obj_nodes[id].matrix = pose,
// render(depth_only=True) -- pyrender's OpenGL rasterisation of the mesh).
//
// Three launches on the caller's stream, nothing read back:
//   prepare   one thread per (vertex, pose): transform, project, snap to 1/256 pixel -> a 16-byte record {sx, sy, 1/Z f64}
//             in the workspace (a vertex is shared by ~6 triangles: done once, not per incident triangle); the same
//             grid-stride kernel clears depth_out, viewed as uint32, to +inf and zeroes the statistics;
//   triangles one lane per (triangle, pose): three 16-byte gathers, int64 area, orientation, bounding box clipped to the
//             frame, exit when the box holds no sample (most triangles of a BOP mesh are sub-pixel). A box of at most
//             COOP_MIN samples is walked by its lane; a larger one is walked by the whole wave, 8x8 samples per step, one
//             such triangle after the other (ballot, broadcast by shuffles). Calls with few triangles get fewer
//             triangles per wave (tpw) so that their large triangles spread over the CUs, and several waves per
//             workgroup that share each large box by rows of tiles. Depth goes into the z-buffer by
//             atomicMin on the float's bits (positive floats order like their bit patterns) behind a plain load: values
//             only fall, so a sample that is already hidden costs no atomic, and a stale load only costs a useless one;
//   resolve   +inf -> 0.
// A minimum does not depend on the order of arrival: the image is bit-reproducible whatever the schedule.
//
// ossid_raster_color (SPEC 7.11-7.12; the template renders of datasets/render_dataset.py:251-331) runs the same vertex
// stage and the same triangle walk over a visibility buffer: one 64-bit key (bits(z) << 32 | face index) per sample in
// the workspace, so that the minimum is the nearest depth and, among equal depths, the lowest face index. Its resolve
// redoes the winner's setup per pixel, recomputes the exact edge functions and interpolates the vertex colours
// perspective-correctly. ossid_template_reduce (7.13) is the s x s box filter that makes a template of such a render.
//
// ossid_raster_textured (SPEC 7.16-7.17; BOP models whose colour lives in a UV texture) is ossid_raster_color with another
// resolve: the same prepare and triangle launches, then per covered pixel the perspective-correct (u, v) at the sample and
// at its right and lower neighbour, a mip level from their largest difference, and one bilinear fetch (texture.h) from the
// chain csrc/texture.hip built.
//
// The arithmetic of a sample (vertex stage, setup, edge functions, depth, colour) lives in raster_common.h, shared with
// csrc/scene.hip.
#include <cmath>

#include "raster_common.h"
#include "texture.h"

namespace {

constexpr int TARGET_WAVES = 2048;    // 256 CUs x 8: below this many full waves the triangles are spread thinner
constexpr int MAX_WAVES = 16;         // waves per workgroup that share the large boxes of a call with few triangles
constexpr int RESIDENT_WAVES = 8192;  // 256 CUs x 32: extra waves per workgroup are added only while all stay resident

__global__ __launch_bounds__(256) void raster_prepare_kernel(const float* __restrict__ vertices, int V,
                                                             const float* __restrict__ transforms, int N, float fx, float fy,
                                                             float cx, float cy, float z_near, VRec* __restrict__ rec,
                                                             unsigned* __restrict__ zbuf, size_t npix,
                                                             int32_t* __restrict__ stats) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < npix; i += nthreads) zbuf[i] = ZFAR;
    if (stats && tid < (size_t)4 * N) stats[tid] = 0;
    const size_t nv = (size_t)N * V;
    for (size_t i = tid; i < nv; i += nthreads) {
        const int pose = (int)(i / V), k = (int)(i - (size_t)pose * V);
        rec[i] = project_vertex(vertices, k, transforms + 16 * (size_t)pose, fx, fy, cx, cy, z_near);
    }
}

// The same with one camera per pose (intrinsics f32 [N][4] = fx, fy, cx, cy) and the visibility buffer cleared to KFAR.
__global__ __launch_bounds__(256) void raster_prepare_color_kernel(const float* __restrict__ vertices, int V,
                                                                   const float* __restrict__ transforms, int N,
                                                                   const float* __restrict__ intrinsics, float z_near,
                                                                   VRec* __restrict__ rec, unsigned long long* __restrict__ keys,
                                                                   size_t npix, int32_t* __restrict__ stats) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < npix; i += nthreads) keys[i] = KFAR;
    if (stats && tid < (size_t)4 * N) stats[tid] = 0;
    const size_t nv = (size_t)N * V;
    for (size_t i = tid; i < nv; i += nthreads) {
        const int pose = (int)(i / V), k = (int)(i - (size_t)pose * V);
        const float* c = intrinsics + 4 * (size_t)pose;
        rec[i] = project_vertex(vertices, k, transforms + 16 * (size_t)pose, c[0], c[1], c[2], c[3], z_near);
    }
}

// Sample of pixel (x, y): coverage, perspective-correct depth, buffer update. Returns whether it was covered. ZB is
// unsigned (z-buffer: the float's bits) or unsigned long long (visibility buffer: bits << 32 | face, SPEC 7.11).
template <typename ZB>
__device__ __forceinline__ bool shade(const Tri& t, double area, int x, int y, int o, int W, ZB* __restrict__ zb, unsigned face) {
    unsigned zbits;
    if (!sample_depth(t, area, x, y, o, zbits)) return false;
    ZB* p = zb + (size_t)y * W + x;
    if constexpr (sizeof(ZB) == 4) {
        if (zbits < *p) atomicMin(p, zbits);
    } else {
        // one 8-byte load (never two halves of different keys); keys only fall, so a stale one costs a useless atomic
        const unsigned long long key = ((unsigned long long)zbits << 32) | face;
        if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
    }
    return true;
}

template <typename ZB>
__global__ __launch_bounds__(64 * MAX_WAVES) void raster_tri_kernel(const int32_t* __restrict__ faces, int F, int V,
                                                        const VRec* __restrict__ rec, int H, int W, int o, int tpw,
                                                        ZB* __restrict__ zbuf, int32_t* __restrict__ stats) {
    // every wave of the workgroup sets up the same tpw triangles; wave 0 walks the small boxes and keeps the statistics,
    // all waves share the large boxes
    const int pose = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __shared__ unsigned long long cov_large;
    if (nw > 1) {
        if (threadIdx.x == 0) cov_large = 0ull;
        __syncthreads();
    }
    const long long tri = (long long)blockIdx.x * tpw + lane;
    const VRec* vr = rec + (size_t)pose * V;
    ZB* zb = zbuf + (size_t)pose * H * W;
    Tri t = {};
    long long A = 0;
    int n_bad = 0, n_degen = 0, n_cov = 0, n_large = 0;
    bool large = false;
    if (lane < tpw && tri < F) {
        const unsigned i0 = (unsigned)faces[3 * tri], i1 = (unsigned)faces[3 * tri + 1], i2 = (unsigned)faces[3 * tri + 2];
        bool bad = i0 >= (unsigned)V || i1 >= (unsigned)V || i2 >= (unsigned)V;   // never read outside the records
        VRec a = {}, b = {}, c = {};
        if (!bad) {
            a = vr[i0], b = vr[i1], c = vr[i2];
            bad = a.sx == INT_MIN || b.sx == INT_MIN || c.sx == INT_MIN;
        }
        if (bad) {
            n_bad = 1;
        } else if (!tri_setup(a, b, c, o, H, W, t, A)) {
            n_degen = 1;
        } else if (t.xa <= t.xb && t.ya <= t.yb) {
            large = (long long)(t.xb - t.xa + 1) * (t.yb - t.ya + 1) > COOP_MIN;
            if (large) {
                n_large = 1;
            } else if (wv == 0) {
                bool cov = false;
                for (int y = t.ya; y <= t.yb; ++y)
                    for (int x = t.xa; x <= t.xb; ++x) cov |= shade(t, (double)A, x, y, o, W, zb, (unsigned)tri);
                n_cov = cov;
            }
        }
    }
    // large boxes: the whole wave walks each, 8 x 8 samples per step
    unsigned long long todo = __ballot(large);
    const int lx = lane & 7, ly = lane >> 3;
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        Tri s;
        s.x0 = __shfl(t.x0, src), s.y0 = __shfl(t.y0, src), s.x1 = __shfl(t.x1, src), s.y1 = __shfl(t.y1, src);
        s.x2 = __shfl(t.x2, src), s.y2 = __shfl(t.y2, src);
        s.r0 = __shfl(t.r0, src), s.r1 = __shfl(t.r1, src), s.r2 = __shfl(t.r2, src);
        s.xa = __shfl(t.xa, src), s.ya = __shfl(t.ya, src), s.xb = __shfl(t.xb, src), s.yb = __shfl(t.yb, src);
        const double area = (double)__shfl(A, src);
        const unsigned face = (unsigned)(blockIdx.x * tpw + src);
        bool cov = false;
        for (int y0 = s.ya + 8 * wv; y0 <= s.yb; y0 += 8 * nw)
            for (int x0 = s.xa; x0 <= s.xb; x0 += 8) {
                const int x = x0 + lx, y = y0 + ly;
                if (x <= s.xb && y <= s.yb) cov |= shade(s, area, x, y, o, W, zb, face);
            }
        if (__ballot(cov) != 0ull && lane == src) n_cov = 1;
    }
    if (nw > 1) {
        if (n_cov && large) atomicOr(&cov_large, 1ull << lane);
        __syncthreads();
        if (large) n_cov = (int)((cov_large >> lane) & 1ull);
    }
    if (stats && wv == 0) {
        n_bad = wave_sum_i32(n_bad), n_degen = wave_sum_i32(n_degen), n_cov = wave_sum_i32(n_cov), n_large = wave_sum_i32(n_large);
        if (lane == 0) {                     // integer sums: independent of the order of arrival
            int32_t* st = stats + 4 * pose;
            if (n_bad) atomicAdd(st, n_bad);
            if (n_degen) atomicAdd(st + 1, n_degen);
            if (n_cov) atomicAdd(st + 2, n_cov);
            if (n_large) atomicAdd(st + 3, n_large);
        }
    }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(unsigned* __restrict__ zbuf, size_t npix) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256)
        if (zbuf[i] == ZFAR) zbuf[i] = 0u;
}

// SPEC 7.11-7.12, one thread per (pose, pixel): the winner's setup again (three records, area, the A < 0 swap -- the
// colours swap with the vertices), the exact edge functions at the sample, colour in f64 with the written parenthesisation.
__global__ __launch_bounds__(256) void raster_resolve_color_kernel(const unsigned long long* __restrict__ keys,
                                                                   const int32_t* __restrict__ faces, int V,
                                                                   const VRec* __restrict__ rec,
                                                                   const unsigned char* __restrict__ colors, int H, int W, int o,
                                                                   size_t npix, unsigned char* __restrict__ color_out,
                                                                   float* __restrict__ depth_out, int32_t* __restrict__ face_out) {
    const size_t hw = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        float z = 0.0f;
        int face = -1, c[3] = {0, 0, 0};
        if (key != KFAR) {
            const int pose = (int)(i / hw);
            const int pix = (int)(i - (size_t)pose * hw), y = pix / W, x = pix - y * W;
            face = (int)(unsigned)key;                   // written by a usable triangle: its indices lie in [0, V)
            z = __uint_as_float((unsigned)(key >> 32));
            const size_t f = (size_t)face;
            sample_color(rec + (size_t)pose * V, colors, faces[3 * f], faces[3 * f + 1], faces[3 * f + 2], x, y, o, c);
        }
        depth_out[i] = z;
        color_out[3 * i] = (unsigned char)c[0], color_out[3 * i + 1] = (unsigned char)c[1], color_out[3 * i + 2] = (unsigned char)c[2];
        if (face_out) face_out[i] = face;
    }
}

// (u, v) of triangle a b d (after the swap; UVs uv0 uv1 uv2 travel with them) at the fixed-point sample (px, py), SPEC
// 7.16: the edge functions are affine, so the integers are exact outside the triangle too. Returns the denominator.
__device__ __forceinline__ double uv_at(const VRec& a, const VRec& b, const VRec& d, const float* __restrict__ uv0,
                                        const float* __restrict__ uv1, const float* __restrict__ uv2, int px, int py, double& u,
                                        double& v) {
    long long w0, w1, w2;
    edge_in(a.sx, a.sy, b.sx, b.sy, px, py, w2);
    edge_in(b.sx, b.sy, d.sx, d.sy, px, py, w0);
    edge_in(d.sx, d.sy, a.sx, a.sy, px, py, w1);
    const double b0 = (double)w0 * a.rz, b1 = (double)w1 * b.rz, b2 = (double)w2 * d.rz;
    const double den = (b0 + b1) + b2;
    u = ((b0 * (double)uv0[0] + b1 * (double)uv1[0]) + b2 * (double)uv2[0]) / den;
    v = ((b0 * (double)uv0[1] + b1 * (double)uv1[1]) + b2 * (double)uv2[1]) / den;
    return den;
}

// SPEC 7.16-7.17, one thread per (pose, pixel): the winner's setup again as sample_color does it (the UVs swap with the
// vertices), (u, v) at the sample and at the samples of the right and lower neighbour, the level by comparison with
// powers of two, the bilinear fetch of texture.h.
__global__ __launch_bounds__(256) void raster_resolve_textured_kernel(
    const unsigned long long* __restrict__ keys, const int32_t* __restrict__ faces, int V, const VRec* __restrict__ rec,
    const float* __restrict__ uvs, const unsigned* __restrict__ mips, int Ht, int Wt, int H, int W, int o, size_t npix,
    unsigned char* __restrict__ color_out, float* __restrict__ depth_out, int32_t* __restrict__ face_out,
    int32_t* __restrict__ lod_out) {
    const size_t hw = (size_t)H * W;
    const int top = tex_top_level(Ht, Wt);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        float z = 0.0f;
        int face = -1, lod = -1, c[3] = {0, 0, 0};
        if (key != KFAR) {
            const int pose = (int)(i / hw);
            const int pix = (int)(i - (size_t)pose * hw), y = pix / W, x = pix - y * W;
            face = (int)(unsigned)key;                   // written by a usable triangle: its indices lie in [0, V)
            z = __uint_as_float((unsigned)(key >> 32));
            const size_t f = (size_t)face;
            const VRec* vr = rec + (size_t)pose * V;
            int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
            VRec a = vr[i0], b = vr[i1], d = vr[i2];
            const long long A = (long long)(b.sx - a.sx) * (long long)(d.sy - a.sy) - (long long)(b.sy - a.sy) * (long long)(d.sx - a.sx);
            if (A < 0) {
                const VRec s = b;
                b = d, d = s;
                const int j = i1;
                i1 = i2, i2 = j;
            }
            const float *uv0 = uvs + 2 * (size_t)i0, *uv1 = uvs + 2 * (size_t)i1, *uv2 = uvs + 2 * (size_t)i2;
            const int px = 256 * x + o, py = 256 * y + o;
            double u, v, ux, vx, uy, vy;
            uv_at(a, b, d, uv0, uv1, uv2, px, py, u, v);
            const double denx = uv_at(a, b, d, uv0, uv1, uv2, px + 256, py, ux, vx);
            const double deny = uv_at(a, b, d, uv0, uv1, uv2, px, py + 256, uy, vy);
            const double dsx = fabs((ux - u) * (double)Wt), dtx = fabs((vx - v) * (double)Ht);
            const double dsy = fabs((uy - u) * (double)Wt), dty = fabs((vy - v) * (double)Ht);
            lod = top;
            if (denx > 0.0 && deny > 0.0 && fin(dsx) && fin(dtx) && fin(dsy) && fin(dty)) {
                const double m0 = dsx > dtx ? dsx : dtx, m1 = dsy > dty ? dsy : dty;
                lod = tex_select_level(m0 > m1 ? m0 : m1, top);
            }
            double q[3];
            tex_bilinear(tex_level(mips, Ht, Wt, lod), u, v, q);
            c[0] = tex_round_u8(q[0]), c[1] = tex_round_u8(q[1]), c[2] = tex_round_u8(q[2]);
        }
        depth_out[i] = z;
        color_out[3 * i] = (unsigned char)c[0], color_out[3 * i + 1] = (unsigned char)c[1], color_out[3 * i + 2] = (unsigned char)c[2];
        if (face_out) face_out[i] = face;
        if (lod_out) lod_out[i] = lod;
    }
}

// SPEC 7.13, one thread per output pixel: the s x s box over a supersampled render, uncovered samples count as 0.
__global__ __launch_bounds__(256) void template_reduce_kernel(const unsigned char* __restrict__ color,
                                                              const float* __restrict__ depth, int N, int T, int s,
                                                              float* __restrict__ img_out, float* __restrict__ mask_out) {
    const size_t nout = (size_t)N * T * T;
    const int S = s * T, s2 = s * s;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nout; i += (size_t)gridDim.x * 256) {
        const int n = (int)(i / ((size_t)T * T));
        const int pix = (int)(i - (size_t)n * T * T), y = pix / T, x = pix - y * T;
        int sum[3] = {0, 0, 0}, cnt = 0;
        for (int dy = 0; dy < s; ++dy) {
            const size_t row = ((size_t)n * S + (size_t)(y * s + dy)) * S + (size_t)x * s;
            for (int dx = 0; dx < s; ++dx)
                if (depth[row + dx] > 0.0f) {
                    const unsigned char* c = color + 3 * (row + dx);
                    sum[0] += c[0], sum[1] += c[1], sum[2] += c[2], ++cnt;
                }
        }
        for (int ch = 0; ch < 3; ++ch)
            img_out[((size_t)n * 3 + ch) * T * T + pix] = (float)((sum[ch] + s2 / 2) / s2) / 255.0f;
        mask_out[i] = (float)cnt / (float)s2;
    }
}

bool sizes_ok(int V, int F, int N) {
    return V >= 1 && V <= OSSID_RASTER_MAX_VERTICES && F >= 0 && F <= OSSID_RASTER_MAX_FACES && N >= 1 &&
           N <= OSSID_RASTER_MAX_POSES;
}

bool frame_ok(int H, int W, float pixel_offset, float z_near) {
    return H > 0 && W > 0 && (long long)H * W <= OSSID_RASTER_MAX_PIXELS && pixel_offset >= 0.0f && pixel_offset <= 1.0f &&
           z_near >= 0.0f && std::isfinite(z_near);
}

int grid_for(size_t work) { return (int)((work + 255) / 256 < 8192 ? (work + 255) / 256 : 8192); }

template <typename ZB>
void launch_triangles(const int32_t* faces, int F, int V, int N, const VRec* rec, int H, int W, int o, ZB* zbuf, int32_t* stats,
                      hipStream_t s) {
    long long tpw = ((long long)F * N + TARGET_WAVES - 1) / TARGET_WAVES;
    tpw = tpw < 1 ? 1 : (tpw > 64 ? 64 : tpw);
    const long long groups = (F + tpw - 1) / tpw;
    // more waves per workgroup only once each wave is down to one triangle: every wave repeats the setup
    long long nw = tpw == 1 ? RESIDENT_WAVES / (groups * N) : 1;
    nw = nw < 1 ? 1 : (nw > MAX_WAVES ? MAX_WAVES : nw);
    hipLaunchKernelGGL(raster_tri_kernel<ZB>, dim3((unsigned)groups, N), dim3(64 * (unsigned)nw), 0, s, faces, F, V, rec, H, W, o,
                       (int)tpw, zbuf, stats);
}

}  // namespace

extern "C" {

size_t ossid_raster_workspace_bytes(int V, int F, int N) {
    if (!sizes_ok(V, F, N)) return 0;
    return (size_t)N * (size_t)V * sizeof(VRec);
}

int ossid_raster_depth(const float* vertices, int V, const int32_t* faces, int F, const float* transforms, int N, float fx,
                       float fy, float cx, float cy, int H, int W, float pixel_offset, float z_near, void* workspace,
                       size_t workspace_bytes, float* depth_out, int32_t* stats, void* stream) {
    const size_t need = ossid_raster_workspace_bytes(V, F, N);
    if (need == 0 || !vertices || (F > 0 && !faces) || !transforms || !workspace || workspace_bytes < need || !depth_out ||
        ((uintptr_t)workspace & 15) != 0 || !frame_ok(H, W, pixel_offset, z_near))
        return OSSID_EINVAL;
    const int o = (int)std::nearbyint((double)pixel_offset * 256.0);       // round half to even
    const size_t npix = (size_t)N * H * W, nv = (size_t)N * V;
    hipStream_t s = (hipStream_t)stream;
    VRec* rec = (VRec*)workspace;
    unsigned* zbuf = (unsigned*)depth_out;
    hipLaunchKernelGGL(raster_prepare_kernel, dim3(grid_for(npix > nv ? npix : nv)), dim3(256), 0, s, vertices, V, transforms, N,
                       fx, fy, cx, cy, z_near, rec, zbuf, npix, stats);
    if (F > 0) launch_triangles(faces, F, V, N, rec, H, W, o, zbuf, stats, s);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(grid_for(npix)), dim3(256), 0, s, zbuf, npix);
    return ossid_launch_status();
}

size_t ossid_raster_color_workspace_bytes(int V, int F, int N, int H, int W) {
    if (!sizes_ok(V, F, N) || H <= 0 || W <= 0 || (long long)H * W > OSSID_RASTER_MAX_PIXELS) return 0;
    return (size_t)N * (size_t)V * sizeof(VRec) + (size_t)N * (size_t)H * (size_t)W * sizeof(unsigned long long);
}

int ossid_raster_color(const float* vertices, int V, const int32_t* faces, int F, const uint8_t* colors,
                       const float* transforms, int N, const float* intrinsics, int H, int W, float pixel_offset, float z_near,
                       void* workspace, size_t workspace_bytes, uint8_t* color_out, float* depth_out, int32_t* face_id_out,
                       int32_t* stats, void* stream) {
    const size_t need = ossid_raster_color_workspace_bytes(V, F, N, H, W);
    if (need == 0 || !vertices || (F > 0 && !faces) || !colors || !transforms || !intrinsics || !workspace ||
        workspace_bytes < need || !color_out || !depth_out || ((uintptr_t)workspace & 15) != 0 ||
        !frame_ok(H, W, pixel_offset, z_near))
        return OSSID_EINVAL;
    const int o = (int)std::nearbyint((double)pixel_offset * 256.0);
    const size_t npix = (size_t)N * H * W, nv = (size_t)N * V;
    hipStream_t s = (hipStream_t)stream;
    VRec* rec = (VRec*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + nv * sizeof(VRec));
    hipLaunchKernelGGL(raster_prepare_color_kernel, dim3(grid_for(npix > nv ? npix : nv)), dim3(256), 0, s, vertices, V,
                       transforms, N, intrinsics, z_near, rec, keys, npix, stats);
    if (F > 0) launch_triangles(faces, F, V, N, rec, H, W, o, keys, stats, s);
    hipLaunchKernelGGL(raster_resolve_color_kernel, dim3(grid_for(npix)), dim3(256), 0, s, keys, faces, V, rec, colors, H, W, o,
                       npix, color_out, depth_out, face_id_out);
    return ossid_launch_status();
}

int ossid_raster_textured(const float* vertices, int V, const int32_t* faces, int F, const float* uvs, const void* mips,
                          size_t mip_bytes, int Ht, int Wt, const float* transforms, int N, const float* intrinsics, int H, int W,
                          float pixel_offset, float z_near, void* workspace, size_t workspace_bytes, uint8_t* color_out,
                          float* depth_out, int32_t* face_id_out, int32_t* lod_out, int32_t* stats, void* stream) {
    const size_t need = ossid_raster_color_workspace_bytes(V, F, N, H, W), tex = ossid_texture_mip_bytes(Ht, Wt);
    if (need == 0 || tex == 0 || !vertices || (F > 0 && !faces) || !uvs || !mips || mip_bytes < tex ||
        ((uintptr_t)mips & 3) != 0 || !transforms || !intrinsics || !workspace || workspace_bytes < need || !color_out ||
        !depth_out || ((uintptr_t)workspace & 15) != 0 || !frame_ok(H, W, pixel_offset, z_near))
        return OSSID_EINVAL;
    const int o = (int)std::nearbyint((double)pixel_offset * 256.0);
    const size_t npix = (size_t)N * H * W, nv = (size_t)N * V;
    hipStream_t s = (hipStream_t)stream;
    VRec* rec = (VRec*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + nv * sizeof(VRec));
    // the prepare and triangle stages are ossid_raster_color's: key, depth, face and statistics are 7.11's
    hipLaunchKernelGGL(raster_prepare_color_kernel, dim3(grid_for(npix > nv ? npix : nv)), dim3(256), 0, s, vertices, V,
                       transforms, N, intrinsics, z_near, rec, keys, npix, stats);
    if (F > 0) launch_triangles(faces, F, V, N, rec, H, W, o, keys, stats, s);
    hipLaunchKernelGGL(raster_resolve_textured_kernel, dim3(grid_for(npix)), dim3(256), 0, s, keys, faces, V, rec, uvs,
                       (const unsigned*)mips, Ht, Wt, H, W, o, npix, color_out, depth_out, face_id_out, lod_out);
    return ossid_launch_status();
}

int ossid_template_reduce(const uint8_t* color, const float* depth, int N, int T, int s, float* img_out, float* mask_out,
                          void* stream) {
    if (!color || !depth || !img_out || !mask_out || N < 1 || N > OSSID_RASTER_MAX_POSES || T < 1 || T > 512 || s < 1 || s > 8)
        return OSSID_EINVAL;
    hipLaunchKernelGGL(template_reduce_kernel, dim3(grid_for((size_t)N * T * T)), dim3(256), 0, (hipStream_t)stream, color, depth,
                       N, T, s, img_out, mask_out);
    return ossid_launch_status();
}

}  // extern "C"
