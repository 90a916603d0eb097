// The rasteriser's arithmetic (SPEC.md section 7), shared by csrc/raster.hip (one mesh per image) and csrc/scene.hip (many
// instances per image): the vertex stage, the snapped 1/256-pixel record, the triangle after setup and the exact edge
// function with its ownership rule. Both files evaluate a sample with these and the same written f64 expressions, which
// is what makes a scene image, per pixel, the bits of the winning instance's own render (SPEC 13.3).
#pragma once
#include <limits.h>

#include "common.h"

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

// Colour of the sample of pixel (x, y) of the winning triangle i0 i1 i2 (indices into rec / colors), SPEC 7.12: the setup
// again (the colours swap with the vertices), the exact edge functions, f64 in the written parenthesisation.
__device__ __forceinline__ void sample_color(const VRec* __restrict__ vr, const unsigned char* __restrict__ colors, int i0,
                                             int i1, int i2, int x, int y, int o, int c[3]) {
    VRec a = vr[i0], b = vr[i1], d = vr[i2];
    const long long A = (long long)(b.sx - a.sx) * (long long)(d.sy - a.sy) - (long long)(b.sy - a.sy) * (long long)(d.sx - a.sx);
    if (A < 0) {
        const VRec s = b;
        b = d, d = s;
        const int j = i1;
        i1 = i2, i2 = j;
    }
    const int px = 256 * x + o, py = 256 * y + o;
    long long w0, w1, w2;
    edge_in(a.sx, a.sy, b.sx, b.sy, px, py, w2);
    edge_in(b.sx, b.sy, d.sx, d.sy, px, py, w0);
    edge_in(d.sx, d.sy, a.sx, a.sy, px, py, w1);
    const double b0 = (double)w0 * a.rz, b1 = (double)w1 * b.rz, b2 = (double)w2 * d.rz;
    const double den = (b0 + b1) + b2;
    const unsigned char *c0 = colors + 3 * (size_t)i0, *c1 = colors + 3 * (size_t)i1, *c2 = colors + 3 * (size_t)i2;
    for (int ch = 0; ch < 3; ++ch) {
        const double v = ((b0 * (double)c0[ch] + b1 * (double)c1[ch]) + b2 * (double)c2[ch]) / den;
        c[ch] = min(255, max(0, (int)rint(v)));
    }
}

}  // namespace
