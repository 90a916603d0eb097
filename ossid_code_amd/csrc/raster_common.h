// The rasteriser (SPEC.md section 7) as far as csrc/raster.hip (one mesh per image) and csrc/scene.hip (many instances
// per image) share it: the vertex stage, the snapped 1/256-pixel record, the triangle after setup and the exact edge
// function with its ownership rule; fetch_triangle (a lane's triangle, checked, set up and classified), the 64-bit shade
// and wave_walk (the large boxes of a wave, 8 x 8 samples per step); winner_of / winner_weights, the setup every resolve
// redoes for the triangle that won a pixel, with both of its surfaces: sample_color (vertex colours) and sample_texture
// (UVs, level and one bilinear fetch of texture.h's chain); and the host's snap_offset and raster_frame_ok. Both files
// evaluate a sample with these and the same written f64 expressions, which is what makes a scene image, per pixel, the
// bits of the winning instance's own render (SPEC 13.3).
#pragma once
#include <limits.h>

#include <cmath>

#include "common.h"
#include "texture.h"

namespace {

constexpr int COOP_MIN = 64;          // clipped boxes with more samples than one wave covers in a step go to the wave
constexpr unsigned ZFAR = 0x7f800000u;
constexpr unsigned long long KFAR = ~0ull;   // empty visibility key: above every (bits(z) << 32 | face)

struct __attribute__((aligned(16))) VRec {
    int sx, sy;      // snapped window coordinates (1/256 pixel); sx == INT_MIN: unusable vertex
    double rz;       // 1 / (double) Z
};
static_assert(sizeof(VRec) == 16, "vertex record");

// Camera-space point of vertex k under transform T (f32 [4][4] row-major), f32 in the written order (SPEC 7.2).
__device__ __forceinline__ void camera_point(const float* __restrict__ vertices, int k, const float* __restrict__ T, float& X,
                                             float& Y, float& Z) {
    const float x = vertices[3 * (size_t)k], y = vertices[3 * (size_t)k + 1], z = vertices[3 * (size_t)k + 2];
    X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// SPEC 7.2 for vertex k under transform T and one camera.
__device__ __forceinline__ VRec project_vertex(const float* __restrict__ vertices, int k, const float* __restrict__ T, float fx,
                                               float fy, float cx, float cy, float z_near) {
    float X, Y, Z;
    camera_point(vertices, k, T, X, Y, Z);
    const float u = (X / Z) * fx + cx, v = (Y / Z) * fy + cy;
    const bool ok = (Z > z_near) && isfinite(X) && isfinite(Y) && isfinite(Z) && (fabsf(u) < 1048576.0f) &&
                    (fabsf(v) < 1048576.0f);      // NaN u, v fail the comparisons
    VRec r;
    r.sx = ok ? (int)rintf(u * 256.0f) : INT_MIN;
    r.sy = ok ? (int)rintf(v * 256.0f) : 0;
    r.rz = ok ? 1.0 / (double)Z : 0.0;
    return r;
}

// One triangle after setup: vertices ordered so that the area A is positive.
struct Tri {
    int x0, y0, x1, y1, x2, y2;
    double r0, r1, r2;
    int xa, ya, xb, yb;      // clipped box of pixels whose sample can lie inside (inclusive)
};

// E_ab(p) = dx (py - ay) - dy (px - ax). dx, dy and both offsets fit 31 bits (29-bit coordinates; a sample of the
// clipped box lies within the triangle's extent), so each product is a 32 x 32 -> 64 multiply and the int64 result exact.
__device__ __forceinline__ bool edge_in(int ax, int ay, int bx, int by, int px, int py, long long& e) {
    const int dx = bx - ax, dy = by - ay;
    e = (long long)dx * (long long)(py - ay) - (long long)dy * (long long)(px - ax);
    return e > 0 || (e == 0 && (dy > 0 || (dy == 0 && dx < 0)));
}

// Setup of a usable triangle a, b, c (none has sx == INT_MIN) for an H x W frame sampled at 256 p + o: false when it is
// degenerate (A == 0); otherwise t and A > 0, with the A < 0 swap of b and c done. t's box may be empty (xa > xb or ya > yb).
__device__ __forceinline__ bool tri_setup(VRec a, VRec b, VRec c, int o, int H, int W, Tri& t, long long& A) {
    A = (long long)(b.sx - a.sx) * (long long)(c.sy - a.sy) - (long long)(b.sy - a.sy) * (long long)(c.sx - a.sx);
    if (A == 0) return false;
    if (A < 0) {
        const VRec s = b;
        b = c, c = s, A = -A;
    }
    t.x0 = a.sx, t.y0 = a.sy, t.x1 = b.sx, t.y1 = b.sy, t.x2 = c.sx, t.y2 = c.sy;
    t.r0 = a.rz, t.r1 = b.rz, t.r2 = c.rz;
    // pixels x with min <= 256 x + o <= max: ceil and floor by arithmetic shifts
    t.xa = max(0, (min(min(t.x0, t.x1), t.x2) - o + 255) >> 8);
    t.xb = min(W - 1, (max(max(t.x0, t.x1), t.x2) - o) >> 8);
    t.ya = max(0, (min(min(t.y0, t.y1), t.y2) - o + 255) >> 8);
    t.yb = min(H - 1, (max(max(t.y0, t.y1), t.y2) - o) >> 8);
    return true;
}

// Coverage of the sample of pixel (x, y) by t and, when covered, the bits of its perspective-correct f32 depth.
__device__ __forceinline__ bool sample_depth(const Tri& t, double area, int x, int y, int o, unsigned& zbits) {
    const int px = 256 * x + o, py = 256 * y + o;
    long long w0, w1, w2;
    const bool in2 = edge_in(t.x0, t.y0, t.x1, t.y1, px, py, w2);
    const bool in0 = edge_in(t.x1, t.y1, t.x2, t.y2, px, py, w0);
    const bool in1 = edge_in(t.x2, t.y2, t.x0, t.y0, px, py, w1);
    if (!(in0 && in1 && in2)) return false;
    const double den = ((double)w0 * t.r0 + (double)w1 * t.r1) + (double)w2 * t.r2;
    zbits = __float_as_uint((float)(area / den));
    return true;
}

// What fetch_triangle found.
enum TriKind { TRI_BAD, TRI_DEGENERATE, TRI_EMPTY, TRI_SMALL, TRI_LARGE };

// The triangle with the indices f[0..2] into the nv records vr: bad when an index or a vertex is unusable, degenerate
// when A == 0, empty when its clipped box holds no sample; otherwise t and A are set and the box decides who walks it.
__device__ __forceinline__ TriKind fetch_triangle(const int32_t* __restrict__ f, int nv, const VRec* __restrict__ vr, int o, int H,
                                                  int W, Tri& t, long long& A) {
    const unsigned i0 = (unsigned)f[0], i1 = (unsigned)f[1], i2 = (unsigned)f[2];
    bool bad = i0 >= (unsigned)nv || i1 >= (unsigned)nv || i2 >= (unsigned)nv;      // never read outside the records
    VRec a = {}, b = {}, c = {};
    if (!bad) {
        // all three records whole before any is tested: returning between the loads splits each gather into three
        a = vr[i0], b = vr[i1], c = vr[i2];
        bad = a.sx == INT_MIN || b.sx == INT_MIN || c.sx == INT_MIN;
    }
    if (bad) return TRI_BAD;
    if (!tri_setup(a, b, c, o, H, W, t, A)) return TRI_DEGENERATE;
    if (t.xa > t.xb || t.ya > t.yb) return TRI_EMPTY;
    return (long long)(t.xb - t.xa + 1) * (t.yb - t.ya + 1) > COOP_MIN ? TRI_LARGE : TRI_SMALL;
}

// Sample of pixel (x, y) against a visibility buffer: coverage, perspective-correct depth, the pixel's key
// bits(z) << 32 | low (SPEC 7.11, 13.3). Returns whether it was covered.
__device__ __forceinline__ bool shade(const Tri& t, double area, int x, int y, int o, int W, unsigned long long* __restrict__ zb,
                                      unsigned low) {
    unsigned zbits;
    if (!sample_depth(t, area, x, y, o, zbits)) return false;
    unsigned long long* p = zb + (size_t)y * W + x;
    // one 8-byte load (never two halves of different keys); keys only fall, so a stale one costs a useless atomic
    const unsigned long long key = ((unsigned long long)zbits << 32) | low;
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
    return true;
}

// Lane src's triangle and area in every lane.
__device__ __forceinline__ Tri tri_from_lane(const Tri& t, long long A, int src, double& area) {
    Tri s;
    s.x0 = __shfl(t.x0, src), s.y0 = __shfl(t.y0, src), s.x1 = __shfl(t.x1, src), s.y1 = __shfl(t.y1, src);
    s.x2 = __shfl(t.x2, src), s.y2 = __shfl(t.y2, src);
    s.r0 = __shfl(t.r0, src), s.r1 = __shfl(t.r1, src), s.r2 = __shfl(t.r2, src);
    s.xa = __shfl(t.xa, src), s.ya = __shfl(t.ya, src), s.xb = __shfl(t.xb, src), s.yb = __shfl(t.yb, src);
    area = (double)__shfl(A, src);
    return s;
}

// Large boxes: the whole wave walks each lane's `large` triangle, one after the other, 8 x 8 samples per step. Waves that
// share the boxes take every rows-th row of tiles, this one from row0. step(s, area, src, x0, x, y, in) runs in all 64
// lanes once per tile: s and area are lane src's, (x, y) is the lane's sample, x0 the tile's first column, `in` whether
// the sample lies inside the box.
template <typename Step>
__device__ __forceinline__ void wave_walk(const Tri& t, long long A, bool large, int row0, int rows, Step step) {
    unsigned long long todo = __ballot(large);
    const int lx = threadIdx.x & 7, ly = (threadIdx.x & 63) >> 3;
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        double area;
        const Tri s = tri_from_lane(t, A, src, area);
        for (int y0 = s.ya + 8 * row0; y0 <= s.yb; y0 += 8 * rows)
            for (int x0 = s.xa; x0 <= s.xb; x0 += 8) {
                const int x = x0 + lx, y = y0 + ly;
                step(s, area, src, x0, x, y, x <= s.xb && y <= s.yb);
            }
    }
}

// The triangle that won a pixel, set up again for its resolve: the three records of the face i0 i1 i2 with the A < 0
// swap done, the indices permuted with them so that whatever is interpolated (colours, UVs) swaps with the vertices.
struct Winner {
    VRec a, b, d;
    int i0, i1, i2;
};

__device__ __forceinline__ Winner winner_of(const VRec* __restrict__ vr, int i0, int i1, int i2) {
    Winner w = {vr[i0], vr[i1], vr[i2], i0, i1, i2};
    const long long A = (long long)(w.b.sx - w.a.sx) * (long long)(w.d.sy - w.a.sy) -
                        (long long)(w.b.sy - w.a.sy) * (long long)(w.d.sx - w.a.sx);
    if (A < 0) {
        const VRec s = w.b;
        w.b = w.d, w.d = s;
        w.i1 = i2, w.i2 = i1;
    }
    return w;
}

// Perspective weights of w's vertices at the fixed-point sample (px, py) and their sum, the denominator (SPEC 7.12,
// 7.16): the edge functions are affine, so the integers are exact outside the triangle too.
__device__ __forceinline__ double winner_weights(const Winner& w, int px, int py, double& b0, double& b1, double& b2) {
    long long w0, w1, w2;
    edge_in(w.a.sx, w.a.sy, w.b.sx, w.b.sy, px, py, w2);
    edge_in(w.b.sx, w.b.sy, w.d.sx, w.d.sy, px, py, w0);
    edge_in(w.d.sx, w.d.sy, w.a.sx, w.a.sy, px, py, w1);
    b0 = (double)w0 * w.a.rz, b1 = (double)w1 * w.b.rz, b2 = (double)w2 * w.d.rz;
    return (b0 + b1) + b2;
}

// Colour of the sample of pixel (x, y) of the winning triangle i0 i1 i2 (indices into rec / colors), SPEC 7.12: f64 in
// the written parenthesisation.
__device__ __forceinline__ void sample_color(const VRec* __restrict__ vr, const unsigned char* __restrict__ colors, int i0,
                                             int i1, int i2, int x, int y, int o, int c[3]) {
    const Winner w = winner_of(vr, i0, i1, i2);
    double b0, b1, b2;
    const double den = winner_weights(w, 256 * x + o, 256 * y + o, b0, b1, b2);
    const unsigned char *c0 = colors + 3 * (size_t)w.i0, *c1 = colors + 3 * (size_t)w.i1, *c2 = colors + 3 * (size_t)w.i2;
    for (int ch = 0; ch < 3; ++ch) {
        const double v = ((b0 * (double)c0[ch] + b1 * (double)c1[ch]) + b2 * (double)c2[ch]) / den;
        c[ch] = min(255, max(0, (int)rint(v)));
    }
}

// (u, v) of the winner w at the fixed-point sample (px, py), SPEC 7.16. Returns the denominator.
__device__ __forceinline__ double uv_at(const Winner& w, const float* __restrict__ uvs, int px, int py, double& u, double& v) {
    double b0, b1, b2;
    const double den = winner_weights(w, px, py, b0, b1, b2);
    const float *uv0 = uvs + 2 * (size_t)w.i0, *uv1 = uvs + 2 * (size_t)w.i1, *uv2 = uvs + 2 * (size_t)w.i2;
    u = ((b0 * (double)uv0[0] + b1 * (double)uv1[0]) + b2 * (double)uv2[0]) / den;
    v = ((b0 * (double)uv0[1] + b1 * (double)uv1[1]) + b2 * (double)uv2[1]) / den;
    return den;
}

// Colour of the sample of pixel (x, y) of the winning triangle i0 i1 i2 (indices into rec / uvs) from the Ht x Wt chain
// at mips, SPEC 7.16-7.17: (u, v) at the sample and at the samples of the right and lower neighbour, the level by
// comparison with powers of two, the bilinear fetch of texture.h. Returns the level fetched.
__device__ __forceinline__ int sample_texture(const VRec* __restrict__ vr, int i0, int i1, int i2, const float* __restrict__ uvs,
                                              const unsigned* __restrict__ mips, int Ht, int Wt, int x, int y, int o, int c[3]) {
    const int top = tex_top_level(Ht, Wt);
    const Winner w = winner_of(vr, i0, i1, i2);
    const int px = 256 * x + o, py = 256 * y + o;
    double u, v, ux, vx, uy, vy;
    uv_at(w, uvs, px, py, u, v);
    const double denx = uv_at(w, uvs, px + 256, py, ux, vx);
    const double deny = uv_at(w, uvs, px, py + 256, uy, vy);
    const double dsx = fabs((ux - u) * (double)Wt), dtx = fabs((vx - v) * (double)Ht);
    const double dsy = fabs((uy - u) * (double)Wt), dty = fabs((vy - v) * (double)Ht);
    int lod = top;
    if (denx > 0.0 && deny > 0.0 && fin(dsx) && fin(dtx) && fin(dsy) && fin(dty)) {
        const double m0 = dsx > dtx ? dsx : dtx, m1 = dsy > dty ? dsy : dty;
        lod = tex_select_level(m0 > m1 ? m0 : m1, top);
    }
    double q[3];
    tex_bilinear(tex_level(mips, Ht, Wt, lod), u, v, q);
    c[0] = tex_round_u8(q[0]), c[1] = tex_round_u8(q[1]), c[2] = tex_round_u8(q[2]);
    return lod;
}

// 256 * pixel_offset as the integer the samples are taken at: round half to even.
inline int snap_offset(float pixel_offset) { return (int)std::nearbyint((double)pixel_offset * 256.0); }

// The frame and sampling arguments every render entry point takes; NaN fails each comparison and is refused.
inline bool raster_frame_ok(int H, int W, float pixel_offset, float z_near) {
    return H > 0 && W > 0 && (long long)H * W <= OSSID_RASTER_MAX_PIXELS && pixel_offset >= 0.0f && pixel_offset <= 1.0f &&
           z_near >= 0.0f && std::isfinite(z_near);
}

}  // namespace
