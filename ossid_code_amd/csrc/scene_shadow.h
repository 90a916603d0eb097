// A light's view of a scene (SPEC.md 13.13-13.15) as far as csrc/scene_shadow.hip, which draws the shadow maps, and
// csrc/scene_light.hip, which looks them up, share it: the view row, the light-space point and its projection -- one
// statement, so that a surface point lands in the map where the vertices around it were drawn --, the map's limits and the
// checks of a scene descriptor both entries make.
#pragma once
#include "raster_common.h"

namespace {

constexpr int MAX_TOTAL = 1 << 29;          // atlas vertices / faces, as csrc/scene.hip: 3 * index stays inside int32
constexpr int SHADOW_MAX_SIDE = 4096;       // Hs, Ws
constexpr int SHADOW_O = 128;               // the maps' samples sit at pixel centres, in 1/256 pixel

// One row of light_views f32 [S][4][16] = (R row-major 9, t 3, a, b, cx, cy) as f64, and the light's kind.
struct LightView {
    double r[9], t[3], a, b, cx, cy;
    bool point;
};

__device__ __forceinline__ LightView load_light_view(const float* __restrict__ row, bool point) {
    LightView v;
#pragma unroll
    for (int k = 0; k < 9; ++k) v.r[k] = (double)row[k];
    v.t[0] = (double)row[9], v.t[1] = (double)row[10], v.t[2] = (double)row[11];
    v.a = (double)row[12], v.b = (double)row[13], v.cx = (double)row[14], v.cy = (double)row[15];
    v.point = point;
    return v;
}

// Q = R P + t in the written order and its projection (13.13): pinhole for a point light, orthographic for a directional
// one. True iff Qz > z_near_l and Q, u, v are finite; NaN fails the comparisons.
__device__ __forceinline__ bool light_project(const LightView& v, double px, double py, double pz, double z_near_l, double& qz,
                                              double& u, double& w) {
    const double qx = ((v.r[0] * px + v.r[1] * py) + v.r[2] * pz) + v.t[0];
    const double qy = ((v.r[3] * px + v.r[4] * py) + v.r[5] * pz) + v.t[1];
    qz = ((v.r[6] * px + v.r[7] * py) + v.r[8] * pz) + v.t[2];
    if (v.point) {
        u = (qx / qz) * v.a + v.cx, w = (qy / qz) * v.b + v.cy;
    } else {
        u = qx * v.a + v.cx, w = qy * v.b + v.cy;
    }
    return qz > z_near_l && fin(qx) && fin(qy) && fin(qz) && fin(u) && fin(w);
}

// What ossid_scene_light and the shadow entries refuse of a descriptor before a launch.
inline bool lit_desc_ok(const ossid_scene_desc& d) {
    if (d.S < 1 || d.S > OSSID_SCENE_MAX_SCENES || d.K < 1 || d.Vt < 1 || d.Vt > MAX_TOTAL || d.Ft < 0 || d.Ft > MAX_TOTAL ||
        d.I < 0 || (long long)d.I > (long long)d.S * OSSID_SCENE_MAX_INSTANCES ||
        !raster_frame_ok(d.H, d.W, d.pixel_offset, d.z_near))
        return false;
    return d.vertices && (d.Ft == 0 || d.faces) && d.meshes && d.scene_first && d.cams &&
           (d.I == 0 || (d.instance_mesh && d.transforms));
}

inline bool shadow_map_ok(int Hs, int Ws, float z_near_l) {
    return Hs >= 1 && Hs <= SHADOW_MAX_SIDE && Ws >= 1 && Ws <= SHADOW_MAX_SIDE && z_near_l > 0.0f && std::isfinite(z_near_l);
}

}  // namespace
