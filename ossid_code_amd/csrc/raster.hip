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
// sets the winner up again per pixel (raster_common.h's winner_of), recomputes the exact edge functions and interpolates
// the vertex colours perspective-correctly. ossid_template_reduce (7.13) is the s x s box filter that makes a template of
// such a render.
//
// ossid_raster_textured (SPEC 7.16-7.17; BOP models whose colour lives in a UV texture) is ossid_raster_color with another
// resolve: the same visibility_pass (refusals, workspace, prepare and triangle launches), then per covered pixel the
// perspective-correct (u, v) at the sample and at its right and lower neighbour, a mip level from their largest
// difference, and one bilinear fetch (texture.h) from the chain csrc/texture.hip built: raster_common.h's sample_texture,
// the one csrc/scene.hip calls for a textured winner.
//
// What csrc/scene.hip needs as well lives in raster_common.h: the arithmetic of a sample (vertex stage, setup, edge
// functions, depth, colour, texture), fetch_triangle, the 64-bit shade, wave_walk, the winner's setup and the frame check.
// This file keeps what is its own: the launch geometry, the z-buffer shade, the coverage statistic and the resolves.
#include <cmath>

#include "raster_common.h"

namespace {

constexpr int TARGET_WAVES = 2048;    // 256 CUs x 8: below this many full waves the triangles are spread thinner
constexpr int MAX_WAVES = 16;         // waves per workgroup that share the large boxes of a call with few triangles
constexpr int RESIDENT_WAVES = 8192;  // 256 CUs x 32: extra waves per workgroup are added only while all stay resident

// Where a pose's camera comes from: the call's one camera (ossid_raster_depth), or intrinsics f32 [N][4] = fx, fy, cx, cy.
struct Camera {
    float fx, fy, cx, cy;
};
struct OneCamera {
    Camera c;
    __device__ Camera at(int) const { return c; }
};
struct CameraPerPose {
    const float* __restrict__ k;
    __device__ Camera at(int pose) const {
        const float* c = k + 4 * (size_t)pose;
        return {c[0], c[1], c[2], c[3]};
    }
};

// ZB is unsigned (z-buffer: the float's bits, cleared to ZFAR) or unsigned long long (visibility buffer, cleared to KFAR).
template <typename ZB, typename Cams>
__global__ __launch_bounds__(256) void raster_prepare_kernel(const float* __restrict__ vertices, int V,
                                                             const float* __restrict__ transforms, int N, Cams cams, float z_near,
                                                             VRec* __restrict__ rec, ZB* __restrict__ zbuf, size_t npix,
                                                             int32_t* __restrict__ stats) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < npix; i += nthreads) zbuf[i] = sizeof(ZB) == 4 ? (ZB)ZFAR : (ZB)KFAR;
    if (stats && tid < (size_t)4 * N) stats[tid] = 0;
    const size_t nv = (size_t)N * V;
    for (size_t i = tid; i < nv; i += nthreads) {
        const int pose = (int)(i / V), k = (int)(i - (size_t)pose * V);
        const Camera c = cams.at(pose);
        rec[i] = project_vertex(vertices, k, transforms + 16 * (size_t)pose, c.fx, c.fy, c.cx, c.cy, z_near);
    }
}

// The z-buffer form of raster_common.h's shade: the float's bits alone, no face.
__device__ __forceinline__ bool shade(const Tri& t, double area, int x, int y, int o, int W, unsigned* __restrict__ zb, unsigned) {
    unsigned zbits;
    if (!sample_depth(t, area, x, y, o, zbits)) return false;
    unsigned* p = zb + (size_t)y * W + x;
    if (zbits < *p) atomicMin(p, zbits);
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
    ZB* zb = zbuf + (size_t)pose * H * W;
    Tri t = {};
    long long A = 0;
    const TriKind kind = lane < tpw && tri < F ? fetch_triangle(faces + 3 * tri, V, rec + (size_t)pose * V, o, H, W, t, A) : TRI_EMPTY;
    const bool large = kind == TRI_LARGE;
    int n_bad = kind == TRI_BAD, n_degen = kind == TRI_DEGENERATE, n_cov = 0, n_large = large;
    if (kind == TRI_SMALL && wv == 0) {
        bool cov = false;
        for (int y = t.ya; y <= t.yb; ++y)
            for (int x = t.xa; x <= t.xb; ++x) cov |= shade(t, (double)A, x, y, o, W, zb, (unsigned)tri);
        n_cov = cov;
    }
    wave_walk(t, A, large, wv, nw, [&](const Tri& s, double area, int src, int, int x, int y, bool in) {
        const bool cov = in && shade(s, area, x, y, o, W, zb, (unsigned)(blockIdx.x * tpw + src));
        if (__ballot(cov) != 0ull && lane == src) n_cov = 1;
    });
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

// One thread per (pose, pixel) of a visibility buffer: the key's decode, then depth, colour, face and the optional level.
// shade_winner(vr, i0, i1, i2, x, y, c) colours the sample of the winning face and returns its level.
template <typename ShadeWinner>
__device__ __forceinline__ void resolve_pixels(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ faces, int V,
                                               const VRec* __restrict__ rec, int H, int W, size_t npix,
                                               unsigned char* __restrict__ color_out, float* __restrict__ depth_out,
                                               int32_t* __restrict__ face_out, int32_t* __restrict__ lod_out,
                                               ShadeWinner shade_winner) {
    const size_t hw = (size_t)H * W;
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
            lod = shade_winner(rec + (size_t)pose * V, faces[3 * f], faces[3 * f + 1], faces[3 * f + 2], x, y, c);
        }
        depth_out[i] = z;
        color_out[3 * i] = (unsigned char)c[0], color_out[3 * i + 1] = (unsigned char)c[1], color_out[3 * i + 2] = (unsigned char)c[2];
        if (face_out) face_out[i] = face;
        if (lod_out) lod_out[i] = lod;
    }
}

// SPEC 7.11-7.12: the winner's vertex colours, interpolated perspective-correctly.
__global__ __launch_bounds__(256) void raster_resolve_color_kernel(const unsigned long long* __restrict__ keys,
                                                                   const int32_t* __restrict__ faces, int V,
                                                                   const VRec* __restrict__ rec,
                                                                   const unsigned char* __restrict__ colors, int H, int W, int o,
                                                                   size_t npix, unsigned char* __restrict__ color_out,
                                                                   float* __restrict__ depth_out, int32_t* __restrict__ face_out) {
    resolve_pixels(keys, faces, V, rec, H, W, npix, color_out, depth_out, face_out, nullptr,
                   [&](const VRec* vr, int i0, int i1, int i2, int x, int y, int c[3]) {
                       sample_color(vr, colors, i0, i1, i2, x, y, o, c);
                       return -1;
                   });
}

// SPEC 7.16-7.17: the winner's texture, by raster_common.h's sample_texture.
__global__ __launch_bounds__(256) void raster_resolve_textured_kernel(
    const unsigned long long* __restrict__ keys, const int32_t* __restrict__ faces, int V, const VRec* __restrict__ rec,
    const float* __restrict__ uvs, const unsigned* __restrict__ mips, int Ht, int Wt, int H, int W, int o, size_t npix,
    unsigned char* __restrict__ color_out, float* __restrict__ depth_out, int32_t* __restrict__ face_out,
    int32_t* __restrict__ lod_out) {
    resolve_pixels(keys, faces, V, rec, H, W, npix, color_out, depth_out, face_out, lod_out,
                   [&](const VRec* vr, int i0, int i1, int i2, int x, int y, int c[3]) {
                       return sample_texture(vr, i0, i1, i2, uvs, mips, Ht, Wt, x, y, o, c);
                   });
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

// The visibility pass of ossid_raster_color and ossid_raster_textured (SPEC 7.11): their common refusals, the workspace
// cut into records and keys, the prepare and triangle launches; then the caller's resolve(keys, rec, o, npix, stream).
template <typename Resolve>
int visibility_pass(const float* vertices, int V, const int32_t* faces, int F, const float* transforms, int N,
                    const float* intrinsics, int H, int W, float pixel_offset, float z_near, void* workspace,
                    size_t workspace_bytes, uint8_t* color_out, float* depth_out, int32_t* stats, hipStream_t s, Resolve resolve) {
    const size_t need = ossid_raster_color_workspace_bytes(V, F, N, H, W);
    if (need == 0 || !vertices || (F > 0 && !faces) || !transforms || !intrinsics || !workspace || workspace_bytes < need ||
        !color_out || !depth_out || ((uintptr_t)workspace & 15) != 0 || !raster_frame_ok(H, W, pixel_offset, z_near))
        return OSSID_EINVAL;
    const int o = snap_offset(pixel_offset);
    const size_t npix = (size_t)N * H * W, nv = (size_t)N * V;
    VRec* rec = (VRec*)workspace;
    unsigned long long* keys = (unsigned long long*)((char*)workspace + nv * sizeof(VRec));
    hipLaunchKernelGGL((raster_prepare_kernel<unsigned long long, CameraPerPose>), dim3(grid_for(npix > nv ? npix : nv)), dim3(256), 0,
                       s, vertices, V, transforms, N, CameraPerPose{intrinsics}, z_near, rec, keys, npix, stats);
    if (F > 0) launch_triangles(faces, F, V, N, rec, H, W, o, keys, stats, s);
    resolve(keys, rec, o, npix, s);
    return ossid_launch_status();
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
        ((uintptr_t)workspace & 15) != 0 || !raster_frame_ok(H, W, pixel_offset, z_near))
        return OSSID_EINVAL;
    const int o = snap_offset(pixel_offset);
    const size_t npix = (size_t)N * H * W, nv = (size_t)N * V;
    hipStream_t s = (hipStream_t)stream;
    VRec* rec = (VRec*)workspace;
    unsigned* zbuf = (unsigned*)depth_out;
    hipLaunchKernelGGL((raster_prepare_kernel<unsigned, OneCamera>), dim3(grid_for(npix > nv ? npix : nv)), dim3(256), 0, s, vertices,
                       V, transforms, N, OneCamera{{fx, fy, cx, cy}}, z_near, rec, zbuf, npix, stats);
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
    if (!colors) return OSSID_EINVAL;
    return visibility_pass(vertices, V, faces, F, transforms, N, intrinsics, H, W, pixel_offset, z_near, workspace, workspace_bytes,
                           color_out, depth_out, stats, (hipStream_t)stream,
                           [&](const unsigned long long* keys, const VRec* rec, int o, size_t npix, hipStream_t s) {
                               hipLaunchKernelGGL(raster_resolve_color_kernel, dim3(grid_for(npix)), dim3(256), 0, s, keys, faces, V,
                                                  rec, colors, H, W, o, npix, color_out, depth_out, face_id_out);
                           });
}

int ossid_raster_textured(const float* vertices, int V, const int32_t* faces, int F, const float* uvs, const void* mips,
                          size_t mip_bytes, int Ht, int Wt, const float* transforms, int N, const float* intrinsics, int H, int W,
                          float pixel_offset, float z_near, void* workspace, size_t workspace_bytes, uint8_t* color_out,
                          float* depth_out, int32_t* face_id_out, int32_t* lod_out, int32_t* stats, void* stream) {
    const size_t tex = ossid_texture_mip_bytes(Ht, Wt);
    if (tex == 0 || !uvs || !mips || mip_bytes < tex || ((uintptr_t)mips & 3) != 0) return OSSID_EINVAL;
    return visibility_pass(vertices, V, faces, F, transforms, N, intrinsics, H, W, pixel_offset, z_near, workspace, workspace_bytes,
                           color_out, depth_out, stats, (hipStream_t)stream,
                           [&](const unsigned long long* keys, const VRec* rec, int o, size_t npix, hipStream_t s) {
                               hipLaunchKernelGGL(raster_resolve_textured_kernel, dim3(grid_for(npix)), dim3(256), 0, s, keys, faces,
                                                  V, rec, uvs, (const unsigned*)mips, Ht, Wt, H, W, o, npix, color_out, depth_out,
                                                  face_id_out, lod_out);
                           });
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
