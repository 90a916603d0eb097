// The uniform cell grid of the exact nearest-neighbour searches (ICP's target cloud, the dense refinement's model levels):
// sizing, cell coordinates and the 27-cell probe, stated once. The counting sort that fills a grid stays with its kernel
// (count and place differ: LDS atomics over register-held points, global atomics over a global array); its scan is
// workgroup.h's.
#pragma once
#include <limits.h>

#include "common.h"

struct CellGrid {
    float lo[3], inv_h;                      // the box's minimum corner, 1 / cell edge (0: the one-cell grid)
    int n[3];
};

// f32 cell coordinate of one axis, clamped to [-2, n + 1] (NaN -> -2): a coordinate more than one cell outside the box
// has no cell in reach, and the probe's ranges [c - 1, c + 1] & [0, n - 1] come out empty for it.
__device__ __forceinline__ int cell_axis(float x, float lo, float inv_h, int n) {
    return (int)fminf(fmaxf(floorf((x - lo) * inv_h), -2.0f), (float)(n + 1));
}

// The cell a point of the set is placed in. Its coordinates are >= 0 (lo is the minimum); rounding of (hi - lo) * inv_h
// can reach n, which stays within one cell of every query that can accept the point, so it is clamped to n - 1.
__device__ __forceinline__ int cell_of(const CellGrid& g, float x, float y, float z) {
    const int cx = min(max(cell_axis(x, g.lo[0], g.inv_h, g.n[0]), 0), g.n[0] - 1);
    const int cy = min(max(cell_axis(y, g.lo[1], g.inv_h, g.n[1]), 0), g.n[1] - 1);
    const int cz = min(max(cell_axis(z, g.lo[2], g.inv_h, g.n[2]), 0), g.n[2] - 1);
    return (cz * g.n[1] + cy) * g.n[0] + cx;
}

// Grid over the box [mn, mx] for queries that accept a pair when its f32 squared distance is <= thr^2. Cell edge
// h >= thr * (1 + 1/16) + maxabs * 2^-14: for any accepted pair every axis has |dx| <= thr, and the f32 rounding of
// (x - lo) * inv_h (relative 2^-23 per operation on coordinates up to maxabs) stays far below the margin, so the two f32
// cell coordinates of each axis differ by less than 1 before the floor and the pair lies in adjacent cells: the 27-cell
// probe finds everything the brute force accepts. h is grown by 5/4 until the grid has at most max_cells cells (a larger
// cell keeps the probe exact). If growth does not get there (|coords| near FLT_MAX) the grid collapses to one cell,
// every coordinate maps to it (inv_h = 0) and the probe is the brute force.
__device__ inline CellGrid cell_grid_size(const float* mn, const float* mx, float thr, int max_cells) {
    float maxabs = 0.0f;
    for (int a = 0; a < 3; ++a) maxabs = fmaxf(maxabs, fmaxf(fabsf(mn[a]), fabsf(mx[a])));
    float h = thr * (1.0f + 1.0f / 16.0f) + maxabs * (1.0f / 16384.0f);
    float nf[3];
    for (int guard = 0; guard < 256; ++guard) {
        double cells = 1.0;
        for (int a = 0; a < 3; ++a) {
            nf[a] = floorf((mx[a] - mn[a]) / h) + 1.0f;
            cells *= (double)nf[a];
        }
        if (cells <= (double)max_cells) break;
        h *= 1.25f;
    }
    float inv_h = 1.0f / h;
    if (!(nf[0] * nf[1] * nf[2] <= (float)max_cells)) {
        nf[0] = nf[1] = nf[2] = 1.0f;
        inv_h = 0.0f;
    }
    CellGrid g;
    for (int a = 0; a < 3; ++a) g.lo[a] = mn[a], g.n[a] = (int)nf[a];
    g.inv_h = inv_h;
    return g;
}

struct CellHit {
    float d2;                                // `worst` and j == INT_MAX when no candidate beat it
    int j, pos;                              // the point's index (its .w bits) and its position in the sorted array
};

// Nearest sorted point of (x, y, z) among the 27 cells around it: the lexicographic minimum of (d2, index), so the order
// inside a cell is free; only d2 <= worst counts at all (NaN never does). The cells of one x-run are contiguous in the
// sorted array. Cells supplies the storage: run(first, last, b, e) sets the positions [b, e) of cells first .. last,
// point(p) returns the sorted point p as (x, y, z, index bits).
template <class Cells>
__device__ __forceinline__ CellHit cell_probe(const CellGrid& g, const Cells& cells, float x, float y, float z, float worst) {
    const int cx = cell_axis(x, g.lo[0], g.inv_h, g.n[0]), cy = cell_axis(y, g.lo[1], g.inv_h, g.n[1]),
              cz = cell_axis(z, g.lo[2], g.inv_h, g.n[2]);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.n[0] - 1);
    CellHit h = {worst, INT_MAX, -1};
    if (x0 > x1) return h;
    for (int zc = max(cz - 1, 0); zc <= min(cz + 1, g.n[2] - 1); ++zc)
        for (int yc = max(cy - 1, 0); yc <= min(cy + 1, g.n[1] - 1); ++yc) {
            const int row = (zc * g.n[1] + yc) * g.n[0];
            int b, e;
            cells.run(row + x0, row + x1, b, e);
            for (int p = b; p < e; ++p) {
                const float4 q = cells.point(p);
                const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const int j = __float_as_int(q.w);
                if (d2 < h.d2 || (d2 == h.d2 && j < h.j)) h.d2 = d2, h.j = j, h.pos = p;
            }
        }
    return h;
}
