// The texture sampler (SPEC.md 7.15-7.17), shared by csrc/raster.hip (the textured resolve) and csrc/model_cloud.hip (the
// textured cloud candidates), as raster_common.h is shared: the mip chain's layout, level selection by comparison with
// exact powers of two, and the clamp-to-edge bilinear fetch in f64 with the written parenthesisation. No library
// transcendental anywhere.
//
// The mip buffer holds the levels one after the other, 4 bytes per texel (R, G, B, 0), row 0 the top row of the image:
// level l has h_l x w_l texels, h_0 x w_0 = Ht x Wt, h_{l+1} = (h_l + 1) >> 1, w_{l+1} = (w_l + 1) >> 1, down to 1 x 1,
// and starts at texel offset sum_{k<l} h_k w_k. A texel is one aligned 32-bit load.
#pragma once
#include <math.h>

#include "common.h"

namespace {

struct TexLevel {
    const unsigned* texels;
    int h, w;
};

// The index of the top (1 x 1) level of an Ht x Wt texture.
__host__ __device__ __forceinline__ int tex_top_level(int Ht, int Wt) {
    int l = 0;
    while (Ht > 1 || Wt > 1) Ht = (Ht + 1) >> 1, Wt = (Wt + 1) >> 1, ++l;
    return l;
}

// Texels of all levels of an Ht x Wt texture (at most 8192^2 * 4/3 + a few rows: below 2^27).
__host__ __device__ __forceinline__ size_t tex_total_texels(int Ht, int Wt) {
    size_t n = (size_t)Ht * (size_t)Wt;
    while (Ht > 1 || Wt > 1) Ht = (Ht + 1) >> 1, Wt = (Wt + 1) >> 1, n += (size_t)Ht * (size_t)Wt;
    return n;
}

// Level l (0 <= l <= top; the caller clamps) of the chain that starts at mips.
__device__ __forceinline__ TexLevel tex_level(const unsigned* __restrict__ mips, int Ht, int Wt, int l) {
    size_t off = 0;
    for (int k = 0; k < l; ++k) off += (size_t)Ht * (size_t)Wt, Ht = (Ht + 1) >> 1, Wt = (Wt + 1) >> 1;
    TexLevel t;
    t.texels = mips + off, t.h = Ht, t.w = Wt;
    return t;
}

// SPEC 7.16: the smallest l with rho <= 2^l, at most `top`. rho is finite and >= 0 (the caller sends everything else to
// the top level); 2^l is exact in f64.
__device__ __forceinline__ int tex_select_level(double rho, int top) {
    int l = 0;
    double p = 1.0;
    while (l < top && rho > p) p *= 2.0, ++l;
    return l;
}

// floor(s), floor(s) + 1 clamped to [0, n - 1]; fs is an integer-valued finite double
__device__ __forceinline__ int tex_clamp(double fs, int n) {
    return fs < 0.0 ? 0 : (fs > (double)(n - 1) ? n - 1 : (int)fs);
}

// SPEC 7.17: bilinear, clamp-to-edge, of level lv at (u, v), v upwards -> c[3] in f64, unrounded. s = u w - 0.5,
// t = (1 - v) h - 0.5; the weights come from floor; the four-tap sum is 14.1's. A non-finite s or t gives 0: no texel
// is read at an index that was never clamped.
__device__ __forceinline__ void tex_bilinear(const TexLevel& lv, double u, double v, double c[3]) {
    const double s = u * (double)lv.w - 0.5, t = (1.0 - v) * (double)lv.h - 0.5;
    c[0] = c[1] = c[2] = 0.0;
    if (!(fin(s) && fin(t))) return;
    const double fs = floor(s), ft = floor(t);
    const double wx = s - fs, wy = t - ft;
    const int x0 = tex_clamp(fs, lv.w), x1 = tex_clamp(fs + 1.0, lv.w);
    const int y0 = tex_clamp(ft, lv.h), y1 = tex_clamp(ft + 1.0, lv.h);
    const unsigned p00 = lv.texels[(size_t)y0 * lv.w + x0], p10 = lv.texels[(size_t)y0 * lv.w + x1];
    const unsigned p01 = lv.texels[(size_t)y1 * lv.w + x0], p11 = lv.texels[(size_t)y1 * lv.w + x1];
    const double w00 = (1.0 - wx) * (1.0 - wy), w10 = wx * (1.0 - wy), w01 = (1.0 - wx) * wy, w11 = wx * wy;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const int sh = 8 * ch;
        c[ch] = ((double)((p00 >> sh) & 255u) * w00 + (double)((p10 >> sh) & 255u) * w10) +
                ((double)((p01 >> sh) & 255u) * w01 + (double)((p11 >> sh) & 255u) * w11);
    }
}

// rint (half to even) clamped to [0, 255]; the input is finite (a convex sum of bytes, or 0)
__device__ __forceinline__ int tex_round_u8(double a) {
    const double r = rint(a);
    return r < 0.0 ? 0 : (r > 255.0 ? 255 : (int)r);
}

}  // namespace
