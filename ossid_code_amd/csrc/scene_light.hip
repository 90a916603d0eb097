// Light for rendered scenes (SPEC.md 13.10-13.11): smooth vertex normals per mesh and a deferred shading pass over a
// rendered batch. csrc/scene.hip draws unlit -- a visible pixel carries the model's own colour -- and stays as it is; the
// pass here runs after it, on its outputs, and is opt-in (scenes.render_scenes(lights=...)).
//
// ossid_mesh_vertex_normals, three launches on the caller's stream, nothing read back:
//   clear       the int64 [V][3] accumulators;
//   accumulate  one thread per face: n = (P1 - P0) x (P2 - P0) in f64 from the f32 coordinates (twice the face's area
//               long: the sum is area-weighted), q = llrint(ldexp(n, shift)), one 64-bit INTEGER atomicAdd per component
//               and vertex. Integer sums do not depend on the order of arrival: the normals are bit-reproducible;
//   finish      one thread per vertex: the sum as f64, normalised, rounded to f32; (0, 0, 0) for an empty sum.
//
// ossid_scene_light, one launch, one thread per (scene, pixel), no LDS, no random numbers: the pixel's winner (instance,
// face) is set up again with raster_common.h's project_vertex / winner_of / winner_weights -- the functions the render ran,
// so the weights are the render's bits and no workspace outlives it --, the camera-space point and the vertex normals are
// interpolated with them, and ambient + Lambert + Blinn-Phong (exponent 2^e by e squarings) of at most four lights per
// scene is applied to the albedo in f64 in the written order (-ffp-contract=off; / and sqrt correctly rounded).
// instance and face are device data the kernel does not trust: a pixel whose values lead outside an array is copied
// through unchanged.
//
// ossid_scene_light_shadowed (SPEC 13.14) is the same kernel with another visibility hook: light_pixel states steps 1-8
// once and asks `vis` how much of each light arrives; NoShadow answers 1, ShadowLookup taps the light's shadow map
// (csrc/scene_shadow.hip draws it) nine times around the texel the surface point projects into.
#include <cmath>

#include "scene_shadow.h"

namespace {

// ---- vertex normals (SPEC 13.10) ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void normals_clear_kernel(long long* __restrict__ acc, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) acc[i] = 0;
}

__global__ __launch_bounds__(256) void normals_accumulate_kernel(const float* __restrict__ vertices,
                                                                 const int32_t* __restrict__ faces, int V, int F, int shift,
                                                                 long long* __restrict__ acc) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < (size_t)F; t += (size_t)gridDim.x * 256) {
        const unsigned i0 = (unsigned)faces[3 * t], i1 = (unsigned)faces[3 * t + 1], i2 = (unsigned)faces[3 * t + 2];
        if (i0 >= (unsigned)V || i1 >= (unsigned)V || i2 >= (unsigned)V) continue;      // never read outside the vertices
        const float *p0 = vertices + 3 * (size_t)i0, *p1 = vertices + 3 * (size_t)i1, *p2 = vertices + 3 * (size_t)i2;
        const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
        const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
        const double n[3] = {ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx};
        if (!(fin(n[0]) && fin(n[1]) && fin(n[2]))) continue;
        const unsigned idx[3] = {i0, i1, i2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long q = (long long)rint(ldexp(n[c], shift));
            if (q == 0) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                atomicAdd((unsigned long long*)(acc + 3 * (size_t)idx[k] + c), (unsigned long long)q);   // two's complement
        }
    }
}

__global__ __launch_bounds__(256) void normals_finish_kernel(const long long* __restrict__ acc, int V,
                                                             float* __restrict__ normals_out) {
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < (size_t)V; v += (size_t)gridDim.x * 256) {
        const double sx = (double)acc[3 * v], sy = (double)acc[3 * v + 1], sz = (double)acc[3 * v + 2];
        const double nn = (sx * sx + sy * sy) + sz * sz;
        float x = 0.0f, y = 0.0f, z = 0.0f;
        if (nn > 0.0) {
            const double len = sqrt(nn);
            x = (float)(sx / len), y = (float)(sy / len), z = (float)(sz / len);
        }
        normals_out[3 * v] = x, normals_out[3 * v + 1] = y, normals_out[3 * v + 2] = z;
    }
}

// ---- shading pass (SPEC 13.11) -------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}

// n' = R n with the f32 rows of T, f32 in 3.4's order.
__device__ __forceinline__ void rotate_normal(const float* __restrict__ normals, int k, const float* __restrict__ T, float n[3]) {
    const float x = normals[3 * (size_t)k], y = normals[3 * (size_t)k + 1], z = normals[3 * (size_t)k + 2];
    n[0] = (T[0] * x + T[1] * y) + T[2] * z;
    n[1] = (T[4] * x + T[5] * y) + T[6] * z;
    n[2] = (T[8] * x + T[9] * y) + T[10] * z;
}

__device__ __forceinline__ int round_u8(double v) {
    const double r = rint(v);
    return r >= 255.0 ? 255 : (r > 0.0 ? (int)r : 0);      // NaN fails both comparisons: 0
}

// The visibility hook of light_pixel: vis(scene * 4 + slot, the light is a point light, P, ndl, blocked) is the share of
// the light that reaches the surface point P, in [0, 1]; it adds its blocked taps to `blocked`. ossid_scene_light's hook:
// every light arrives whole, and x * 1.0 is x, so its bits are those of the unhooked expressions.
struct NoShadow {
    static constexpr bool shadowed = false;
    __device__ __forceinline__ double operator()(int, bool, const double*, double, int&) const { return 1.0; }
};

// ossid_scene_light_shadowed's hook, SPEC 13.14: nine taps of the light's shadow map around the texel P projects into.
struct ShadowLookup {
    static constexpr bool shadowed = true;
    const unsigned* map;          // [S][4][Hs][Ws], ossid_scene_shadow_maps'
    const float* views;           // [S][4][16]
    const int32_t* enable;        // [S][4]
    const float* params;          // [S][2] = (beta0, beta1)
    int Hs, Ws;
    double z_near_l;

    __device__ __forceinline__ double operator()(int ls, bool point, const double* P, double ndl, int& blocked) const {
        if (enable[ls] == 0) return 1.0;
        const LightView lv = load_light_view(views + 16 * (size_t)ls, point);
        double qz, u, v;
        if (!light_project(lv, P[0], P[1], P[2], z_near_l, qz, u, v)) return 1.0;
        const double texel = point ? qz / lv.a : 1.0 / lv.a;
        const double s2 = 1.0 - ndl * ndl;
        const double tn = sqrt(s2 > 0.0 ? s2 : 0.0) / ndl;
        const float* beta = params + 2 * (size_t)(ls / OSSID_SCENE_MAX_LIGHTS);
        const double bias = texel * ((double)beta[0] + (double)beta[1] * (tn < 8.0 ? tn : 8.0));
        const double thr = qz - bias;
        // floor(u) as an integer; past either border by two texels or more no tap is inside, whatever the value
        const double fu = floor(u), fv = floor(v);
        const int ix = fu < -2.0 ? -2 : (fu > (double)(Ws + 1) ? Ws + 1 : (int)fu);
        const int iy = fv < -2.0 ? -2 : (fv > (double)(Hs + 1) ? Hs + 1 : (int)fv);
        const unsigned* zb = map + (size_t)ls * Hs * Ws;
        int k = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int x = ix + dx, y = iy + dy;
                if (x < 0 || x >= Ws || y < 0 || y >= Hs) continue;
                const unsigned zbits = zb[(size_t)y * Ws + x];
                k += zbits != ZFAR && (double)__uint_as_float(zbits) < thr;      // a NaN on either side blocks nothing
            }
        blocked += k;
        return (double)(9 - k) / 9.0;
    }
};

// Steps 1-8 of SPEC 13.11 for pixel (x, y) of `scene`, whose albedo is c: false (nothing written) when inst or fc leads
// outside an array or to a triangle the render cannot have drawn; otherwise c becomes the lit colour and nrm the normal,
// and `blocked` grows by what vis counted. Stated once for both entries: they differ in vis alone.
template <typename Vis>
__device__ __forceinline__ bool light_pixel(const ossid_scene_desc& d, const float* __restrict__ normals,
                                            const float* __restrict__ lights, const int32_t* __restrict__ n_lights,
                                            const float* __restrict__ ambient, const float* __restrict__ material, int scene,
                                            int inst, int fc, int x, int y, int o, int c[3], float nrm[3], const Vis& vis,
                                            int& blocked) {
    if (inst < d.scene_first[scene] || inst >= d.scene_first[scene + 1] || inst >= d.I) return false;
    const int m = d.instance_mesh[inst];
    if (m < 0 || m >= d.K) return false;
    const int v0 = d.meshes[4 * m], nv = d.meshes[4 * m + 1], f0 = d.meshes[4 * m + 2], nf = d.meshes[4 * m + 3];
    if (v0 < 0 || nv < 0 || nv > d.Vt - v0 || f0 < 0 || nf < 0 || nf > d.Ft - f0 || fc < 0 || fc >= nf) return false;
    const int32_t* f = d.faces + 3 * (size_t)(f0 + fc);
    const unsigned u0 = (unsigned)f[0], u1 = (unsigned)f[1], u2 = (unsigned)f[2];
    if (u0 >= (unsigned)nv || u1 >= (unsigned)nv || u2 >= (unsigned)nv) return false;
    const int k0 = v0 + (int)u0, k1 = v0 + (int)u1, k2 = v0 + (int)u2;       // atlas rows, in the order of the faces row
    const float* T = d.transforms + 16 * (size_t)inst;
    const float* cam = d.cams + 4 * (size_t)scene;
    const VRec vr[3] = {project_vertex(d.vertices, k0, T, cam[0], cam[1], cam[2], cam[3], d.z_near),
                        project_vertex(d.vertices, k1, T, cam[0], cam[1], cam[2], cam[3], d.z_near),
                        project_vertex(d.vertices, k2, T, cam[0], cam[1], cam[2], cam[3], d.z_near)};
    if (vr[0].sx == INT_MIN || vr[1].sx == INT_MIN || vr[2].sx == INT_MIN) return false;
    const long long A = (long long)(vr[1].sx - vr[0].sx) * (long long)(vr[2].sy - vr[0].sy) -
                        (long long)(vr[1].sy - vr[0].sy) * (long long)(vr[2].sx - vr[0].sx);
    if (A == 0) return false;
    // 1. the winner's setup and weights, the render's own
    const Winner w = winner_of(vr, 0, 1, 2);
    const bool swapped = w.i1 != 1;
    double b0, b1, b2;
    const double den = winner_weights(w, 256 * x + o, 256 * y + o, b0, b1, b2);
    // 2. the surface point from the f32 camera points, permuted as the swap permuted the vertices
    float p0[3], pa[3], pb[3];
    camera_point(d.vertices, k0, T, p0[0], p0[1], p0[2]);
    camera_point(d.vertices, k1, T, pa[0], pa[1], pa[2]);
    camera_point(d.vertices, k2, T, pb[0], pb[1], pb[2]);
    float n0[3], na[3], nb[3];
    rotate_normal(normals, k0, T, n0);
    rotate_normal(normals, k1, T, na);
    rotate_normal(normals, k2, T, nb);
    double P[3], N[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // both orders are summed and one is kept: a select between the six f32 inputs becomes a table in scratch memory
        const double pn = (b0 * (double)p0[k] + b1 * (double)pa[k]) + b2 * (double)pb[k];
        const double ps = (b0 * (double)p0[k] + b1 * (double)pb[k]) + b2 * (double)pa[k];
        P[k] = (swapped ? ps : pn) / den;
        // 3. the camera-space vertex normals, interpolated without the division
        const double nn = (b0 * (double)n0[k] + b1 * (double)na[k]) + b2 * (double)nb[k];
        const double ns = (b0 * (double)n0[k] + b1 * (double)nb[k]) + b2 * (double)na[k];
        N[k] = swapped ? ns : nn;
    }
    // 4. its length, or the face's normal (13.4's n, in the order of the faces row) when there is none
    double NN = dot3(N[0], N[1], N[2], N[0], N[1], N[2]);
    if (!(NN > 0.0) || !fin(NN)) {
        const double ax = (double)pa[0] - (double)p0[0], ay = (double)pa[1] - (double)p0[1], az = (double)pa[2] - (double)p0[2];
        const double bx = (double)pb[0] - (double)p0[0], by = (double)pb[1] - (double)p0[1], bz = (double)pb[2] - (double)p0[2];
        N[0] = ay * bz - az * by, N[1] = az * bx - ax * bz, N[2] = ax * by - ay * bx;
        NN = dot3(N[0], N[1], N[2], N[0], N[1], N[2]);
    }
    double Nh[3] = {0.0, 0.0, 0.0};
    if (NN > 0.0) {
        const double len = sqrt(NN);
        Nh[0] = N[0] / len, Nh[1] = N[1] / len, Nh[2] = N[2] / len;
    }
    // 5. the view direction; the surface is two-sided
    const double plen = sqrt(dot3(P[0], P[1], P[2], P[0], P[1], P[2]));
    const double Vh[3] = {-P[0] / plen, -P[1] / plen, -P[2] / plen};
    if (dot3(Nh[0], Nh[1], Nh[2], Vh[0], Vh[1], Vh[2]) < 0.0) Nh[0] = -Nh[0], Nh[1] = -Nh[1], Nh[2] = -Nh[2];
    // 6. the lights, in order
    const float* amb = ambient + 3 * (size_t)scene;
    double E[3] = {(double)amb[0], (double)amb[1], (double)amb[2]}, Sp[3] = {0.0, 0.0, 0.0};
    const float ef = material[2 * (size_t)inst + 1];
    const int e = !(ef > 0.0f) ? 0 : (ef >= 10.0f ? 10 : (int)ef);
    const int nl = min(max(n_lights[scene], 0), OSSID_SCENE_MAX_LIGHTS);
    for (int l = 0; l < nl; ++l) {
        const float* L = lights + 8 * ((size_t)scene * OSSID_SCENE_MAX_LIGHTS + l);
        double D[3] = {(double)L[0], (double)L[1], (double)L[2]};
        if (L[3] != 0.0f) D[0] = D[0] - P[0], D[1] = D[1] - P[1], D[2] = D[2] - P[2];
        const double dd = dot3(D[0], D[1], D[2], D[0], D[1], D[2]);
        if (!(dd > 0.0) || !fin(dd)) continue;
        const double dl = sqrt(dd);
        const double Lh[3] = {D[0] / dl, D[1] / dl, D[2] / dl};
        const double ndl = dot3(Nh[0], Nh[1], Nh[2], Lh[0], Lh[1], Lh[2]);
        if (!(ndl > 0.0)) continue;
        const double I[3] = {(double)L[4], (double)L[5], (double)L[6]};
        const double vs = vis(scene * OSSID_SCENE_MAX_LIGHTS + l, L[3] != 0.0f, P, ndl, blocked);
        const double dif = ndl * vs;
        E[0] = E[0] + I[0] * dif, E[1] = E[1] + I[1] * dif, E[2] = E[2] + I[2] * dif;
        const double Hh[3] = {Lh[0] + Vh[0], Lh[1] + Vh[1], Lh[2] + Vh[2]};
        const double hh = dot3(Hh[0], Hh[1], Hh[2], Hh[0], Hh[1], Hh[2]);
        if (!(hh > 0.0)) continue;
        const double hl = sqrt(hh);
        const double ndh = dot3(Nh[0], Nh[1], Nh[2], Hh[0] / hl, Hh[1] / hl, Hh[2] / hl);
        if (!(ndh > 0.0)) continue;
        double p = ndh;
        for (int k = 0; k < e; ++k) p = p * p;             // ndh^(2^e) by exact squarings
        p = p * vs;
        Sp[0] = Sp[0] + I[0] * p, Sp[1] = Sp[1] + I[1] * p, Sp[2] = Sp[2] + I[2] * p;
    }
    // 7., 8.
    const double ks = (double)material[2 * (size_t)inst];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = round_u8((double)c[k] * E[k] + 255.0 * (ks * Sp[k]));
        nrm[k] = (float)Nh[k];
    }
    return true;
}

template <typename Vis>
__global__ __launch_bounds__(256) void scene_light_kernel(ossid_scene_desc d, const float* __restrict__ normals,
                                                          const unsigned char* albedo, const int32_t* __restrict__ instance,
                                                          const int32_t* __restrict__ face, const float* __restrict__ lights,
                                                          const int32_t* __restrict__ n_lights, const float* __restrict__ ambient,
                                                          const float* __restrict__ material, unsigned char* lit_out,
                                                          float* __restrict__ normal_out, int o, Vis vis,
                                                          unsigned char* __restrict__ blocked_out) {
    const size_t hw = (size_t)d.H * d.W, npix = (size_t)d.S * hw;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (size_t)gridDim.x * 256) {
        // albedo and lit_out may be one buffer (neither is __restrict__): the pixel is read whole before it is written
        int c[3] = {albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2]};
        float nrm[3] = {0.0f, 0.0f, 0.0f};
        const int inst = instance[i];
        int blocked = 0;
        if (inst >= 0) {                                   // the background is not relit
            const int scene = (int)(i / hw);
            const int pix = (int)(i - (size_t)scene * hw), y = pix / d.W, x = pix - y * d.W;
            int lit[3] = {c[0], c[1], c[2]};
            float n[3];
            int k = 0;
            if (light_pixel(d, normals, lights, n_lights, ambient, material, scene, inst, face[i], x, y, o, lit, n, vis, k)) {
                c[0] = lit[0], c[1] = lit[1], c[2] = lit[2];
                nrm[0] = n[0], nrm[1] = n[1], nrm[2] = n[2];
                blocked = k;
            }
        }
        lit_out[3 * i] = (unsigned char)c[0], lit_out[3 * i + 1] = (unsigned char)c[1], lit_out[3 * i + 2] = (unsigned char)c[2];
        if (normal_out) normal_out[3 * i] = nrm[0], normal_out[3 * i + 1] = nrm[1], normal_out[3 * i + 2] = nrm[2];
        if constexpr (Vis::shadowed) {
            if (blocked_out) blocked_out[i] = (unsigned char)blocked;      // at most 4 lights x 9 taps
        }
    }
}

}  // namespace

extern "C" {

size_t ossid_mesh_vertex_normals_workspace_bytes(int V) {
    return V < 1 || V > MAX_TOTAL ? 0 : (size_t)V * 3 * sizeof(long long);
}

int ossid_mesh_vertex_normals(const float* vertices, const int32_t* faces, int V, int F, int shift, void* workspace,
                              size_t workspace_bytes, float* normals_out, void* stream) {
    const size_t need = ossid_mesh_vertex_normals_workspace_bytes(V);
    if (need == 0 || !workspace || workspace_bytes < need || ((uintptr_t)workspace & 7) != 0) return OSSID_EINVAL;
    if (!vertices || !normals_out || F < 0 || F > OSSID_RASTER_MAX_FACES || (F > 0 && !faces) || shift > 1000 || shift < -1000)
        return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    long long* acc = (long long*)workspace;
    hipLaunchKernelGGL(normals_clear_kernel, dim3(grid_for((size_t)V * 3)), dim3(256), 0, s, acc, (size_t)V * 3);
    if (F > 0)
        hipLaunchKernelGGL(normals_accumulate_kernel, dim3(grid_for((size_t)F)), dim3(256), 0, s, vertices, faces, V, F, shift, acc);
    hipLaunchKernelGGL(normals_finish_kernel, dim3(grid_for((size_t)V)), dim3(256), 0, s, acc, V, normals_out);
    return ossid_launch_status();
}

int ossid_scene_light(const ossid_scene_desc* desc_host, const float* normals, const uint8_t* albedo, const int32_t* instance,
                      const int32_t* face, const float* lights, const int32_t* n_lights, const float* ambient,
                      const float* material, uint8_t* lit_out, float* normal_out, void* stream) {
    if (!desc_host || !normals || !albedo || !instance || !face || !lights || !n_lights || !ambient || !material || !lit_out)
        return OSSID_EINVAL;
    const ossid_scene_desc d = *desc_host;
    if (!lit_desc_ok(d)) return OSSID_EINVAL;
    hipLaunchKernelGGL(scene_light_kernel<NoShadow>, dim3(grid_for((size_t)d.S * d.H * d.W)), dim3(256), 0, (hipStream_t)stream, d,
                       normals, albedo, instance, face, lights, n_lights, ambient, material, lit_out, normal_out,
                       snap_offset(d.pixel_offset), NoShadow(), (unsigned char*)nullptr);
    return ossid_launch_status();
}

int ossid_scene_light_shadowed(const ossid_scene_desc* desc_host, const float* normals, const uint8_t* albedo,
                               const int32_t* instance, const int32_t* face, const float* lights, const int32_t* n_lights,
                               const float* ambient, const float* material, const uint32_t* shadow_map, const float* light_views,
                               const int32_t* enable, int Hs, int Ws, float z_near_l, const float* shadow_params,
                               uint8_t* lit_out, float* normal_out, uint8_t* blocked_out, void* stream) {
    if (!desc_host || !normals || !albedo || !instance || !face || !lights || !n_lights || !ambient || !material || !lit_out ||
        !shadow_map || !light_views || !enable || !shadow_params || !shadow_map_ok(Hs, Ws, z_near_l))
        return OSSID_EINVAL;
    const ossid_scene_desc d = *desc_host;
    if (!lit_desc_ok(d)) return OSSID_EINVAL;
    const ShadowLookup vis = {shadow_map, light_views, enable, shadow_params, Hs, Ws, (double)z_near_l};
    hipLaunchKernelGGL(scene_light_kernel<ShadowLookup>, dim3(grid_for((size_t)d.S * d.H * d.W)), dim3(256), 0,
                       (hipStream_t)stream, d, normals, albedo, instance, face, lights, n_lights, ambient, material, lit_out,
                       normal_out, snap_offset(d.pixel_offset), vis, blocked_out);
    return ossid_launch_status();
}

}  // extern "C"
