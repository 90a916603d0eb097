// Shadow maps for lit scenes (SPEC.md 13.13): one depth map per (scene, light slot), the scene's own draw list seen from
// the light, drawn with raster_common.h's machinery -- 1/256-pixel snapped coordinates, tri_setup / edge_in with their
// ownership rule, small boxes by one lane, large ones by wave_walk -- so that a map is exact and bit-reproducible as the
// render is. csrc/scene_light.hip's shadowed pass looks the maps up (13.14); scenes.shadow_views places the views (13.15).
//
// ossid_scene_shadow_maps, two launches on the caller's stream, nothing read back, no workspace:
//   clear      every sample to ZFAR;
//   triangles  one wave per row of the caller's work list (scene * 4 + slot, instance, first face), one lane per face of
//              the 64 from `first face`. The lane projects its triangle's three vertices itself: the f32 camera point
//              (camera_point, the bits the shading pass interpolates), then scene_shadow.h's light_project in f64 -- a
//              vertex is projected once per triangle that uses it, about six times, and no record outlives the launch.
//              The depth of a covered sample is perspective-correct for a point light (sample_depth) and affine for a
//              directional one, rounded to f32, and reduced by a 32-bit atomicMin on its bits behind a plain load: every
//              stored depth is a positive float (Qz > z_near_l > 0), so the unsigned order is the numeric one, and a
//              minimum does not depend on the order of arrival.
// The work list, like instance and face in the shading pass, is device data the kernel does not trust: a row that leads
// outside an array is skipped.
#include <cmath>

#include "scene_shadow.h"

namespace {

__global__ __launch_bounds__(256) void shadow_clear_kernel(unsigned* __restrict__ map, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) map[i] = ZFAR;
}

// 13.13's vertex stage for atlas row k: the record's rz holds 1 / Qz for a point light, Qz for a directional one.
__device__ __forceinline__ VRec shadow_vertex(const float* __restrict__ vertices, int k, const float* __restrict__ T,
                                              const LightView& lv, double z_near_l) {
    float X, Y, Z;
    camera_point(vertices, k, T, X, Y, Z);
    double qz, u, v;
    const bool ok = light_project(lv, (double)X, (double)Y, (double)Z, z_near_l, qz, u, v) && fabs(u) < 1048576.0 &&
                    fabs(v) < 1048576.0;
    VRec r;
    r.sx = ok ? (int)rint(u * 256.0) : INT_MIN;
    r.sy = ok ? (int)rint(v * 256.0) : 0;
    r.rz = ok ? (lv.point ? 1.0 / qz : qz) : 0.0;
    return r;
}

// Coverage of the sample of map pixel (x, y) by t and, when covered, the bits of its f32 light-space depth.
__device__ __forceinline__ bool shadow_depth(const Tri& t, double area, bool point, int x, int y, unsigned& zbits) {
    if (point) return sample_depth(t, area, x, y, SHADOW_O, zbits);
    const int px = 256 * x + SHADOW_O, py = 256 * y + SHADOW_O;
    long long w0, w1, w2;
    const bool in2 = edge_in(t.x0, t.y0, t.x1, t.y1, px, py, w2);
    const bool in0 = edge_in(t.x1, t.y1, t.x2, t.y2, px, py, w0);
    const bool in1 = edge_in(t.x2, t.y2, t.x0, t.y0, px, py, w1);
    if (!(in0 && in1 && in2)) return false;
    const double num = ((double)w0 * t.r0 + (double)w1 * t.r1) + (double)w2 * t.r2;
    zbits = __float_as_uint((float)(num / area));
    return true;
}

__device__ __forceinline__ void shadow_store(const Tri& t, double area, bool point, int x, int y, int Ws,
                                             unsigned* __restrict__ zb) {
    unsigned zbits;
    if (!shadow_depth(t, area, point, x, y, zbits)) return;
    unsigned* p = zb + (size_t)y * Ws + x;
    // depths only fall, so a stale load costs a useless atomic
    if (zbits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, zbits);
}

__global__ __launch_bounds__(256) void shadow_tri_kernel(ossid_scene_desc d, const float* __restrict__ lights,
                                                         const float* __restrict__ light_views,
                                                         const int32_t* __restrict__ items, int n, int Hs, int Ws,
                                                         double z_near_l, unsigned* __restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (item >= n) return;                                 // whole waves leave: nothing below synchronises the workgroup
    const int ls = __builtin_amdgcn_readfirstlane(items[3 * (size_t)item]);
    const int inst = __builtin_amdgcn_readfirstlane(items[3 * (size_t)item + 1]);
    const int first = __builtin_amdgcn_readfirstlane(items[3 * (size_t)item + 2]);
    // the row's values are the wave's: every return below is taken by all 64 lanes or by none
    if (ls < 0 || ls >= d.S * OSSID_SCENE_MAX_LIGHTS) return;
    const int scene = ls / OSSID_SCENE_MAX_LIGHTS;
    if (inst < 0 || inst < d.scene_first[scene] || inst >= d.scene_first[scene + 1] || inst >= d.I) return;
    const int m = d.instance_mesh[inst];
    if (m < 0 || m >= d.K) return;
    const int v0 = d.meshes[4 * m], nv = d.meshes[4 * m + 1], f0 = d.meshes[4 * m + 2], nf = d.meshes[4 * m + 3];
    if (v0 < 0 || nv < 0 || nv > d.Vt - v0 || f0 < 0 || nf < 0 || nf > d.Ft - f0 || first < 0 || first >= nf) return;
    const LightView lv = load_light_view(light_views + 16 * (size_t)ls, lights[8 * (size_t)ls + 3] != 0.0f);
    const float* T = d.transforms + 16 * (size_t)inst;
    const int fc = first + lane;
    Tri t = {};
    long long A = 0;
    TriKind kind = TRI_EMPTY;
    if (fc < nf) {
        const int32_t* f = d.faces + 3 * (size_t)(f0 + fc);
        const unsigned i0 = (unsigned)f[0], i1 = (unsigned)f[1], i2 = (unsigned)f[2];
        kind = TRI_BAD;
        if (i0 < (unsigned)nv && i1 < (unsigned)nv && i2 < (unsigned)nv) {     // never read outside the mesh's vertices
            const VRec a = shadow_vertex(d.vertices, v0 + (int)i0, T, lv, z_near_l);
            const VRec b = shadow_vertex(d.vertices, v0 + (int)i1, T, lv, z_near_l);
            const VRec c = shadow_vertex(d.vertices, v0 + (int)i2, T, lv, z_near_l);
            if (a.sx != INT_MIN && b.sx != INT_MIN && c.sx != INT_MIN) {       // no clipping: an unusable vertex casts nothing
                if (!tri_setup(a, b, c, SHADOW_O, Hs, Ws, t, A)) kind = TRI_DEGENERATE;
                else if (t.xa > t.xb || t.ya > t.yb) kind = TRI_EMPTY;
                else kind = (long long)(t.xb - t.xa + 1) * (t.yb - t.ya + 1) > COOP_MIN ? TRI_LARGE : TRI_SMALL;
            }
        }
    }
    unsigned* zb = map + (size_t)ls * Hs * Ws;
    if (kind == TRI_SMALL)
        for (int y = t.ya; y <= t.yb; ++y)
            for (int x = t.xa; x <= t.xb; ++x) shadow_store(t, (double)A, lv.point, x, y, Ws, zb);
    wave_walk(t, A, kind == TRI_LARGE, 0, 1, [&](const Tri& s, double area, int, int, int x, int y, bool in_box) {
        if (in_box) shadow_store(s, area, lv.point, x, y, Ws, zb);
    });
}

}  // namespace

extern "C" {

int ossid_scene_shadow_maps(const ossid_scene_desc* desc_host, const float* lights, const float* light_views,
                            const int32_t* items, int n, int Hs, int Ws, float z_near_l, uint32_t* shadow_map, void* stream) {
    if (!desc_host || !lights || !light_views || !shadow_map || n < 0 || n > (1 << 30) || (n > 0 && !items) ||
        !shadow_map_ok(Hs, Ws, z_near_l))
        return OSSID_EINVAL;
    const ossid_scene_desc d = *desc_host;
    if (!lit_desc_ok(d)) return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t samples = (size_t)d.S * OSSID_SCENE_MAX_LIGHTS * Hs * Ws;
    hipLaunchKernelGGL(shadow_clear_kernel, dim3(grid_for(samples)), dim3(256), 0, s, shadow_map, samples);
    if (n > 0 && d.I > 0)
        hipLaunchKernelGGL(shadow_tri_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, d, lights, light_views, items, n, Hs,
                           Ws, (double)z_near_l, shadow_map);
    return ossid_launch_status();
}

}  // extern "C"
