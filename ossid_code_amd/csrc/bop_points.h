// SPEC.md 8.7's point arithmetic, stated once: csrc/bop_eval.hip (MSSD / MSPD) and csrc/pose_select.hip (section 16's
// distance) both compose G = pose_gt . S, transform a point and square a distance through these, so the two cannot drift
// apart. f64 throughout, the written order of operations (the library is built with -ffp-contract=off).
#pragma once
#include "common.h"

// G = [R_gt . S_R | R_gt . S_t + t_gt]: rows 0..2 of the 4x4 product as 12 doubles, row-major [3][4]. Pg and Sm are
// row-major 4x4; each element (a0 b0 + a1 b1) + a2 b2, the translation ((a0 b0 + a1 b1) + a2 b2) + t.
__device__ __forceinline__ void bop_compose(const double* __restrict__ Pg, const double* __restrict__ Sm, double* G) {
    for (int r = 0; r < 3; ++r) {
        const double a0 = Pg[4 * r], a1 = Pg[4 * r + 1], a2 = Pg[4 * r + 2];
        for (int col = 0; col < 3; ++col) G[4 * r + col] = (a0 * Sm[col] + a1 * Sm[4 + col]) + a2 * Sm[8 + col];
        G[4 * r + 3] = ((a0 * Sm[3] + a1 * Sm[7]) + a2 * Sm[11]) + Pg[4 * r + 3];
    }
}

// p = ((r0 x + r1 y) + r2 z) + t under the [3][4] transform T
__device__ __forceinline__ void bop_transform(const double* T, double x, double y, double z, double& X, double& Y, double& Z) {
    X = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    Y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    Z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// q = (dx dx + dy dy) + dz dz; a NaN counts as +inf
__device__ __forceinline__ double bop_sqdist(double Xe, double Ye, double Ze, double Xg, double Yg, double Zg) {
    const double dx = Xe - Xg, dy = Ye - Yg, dz = Ze - Zg;
    const double q = (dx * dx + dy * dy) + dz * dz;
    return q == q ? q : (double)INFINITY;
}
