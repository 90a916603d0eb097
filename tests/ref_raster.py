"""Independent numpy restatement of SPEC.md section 7 (mesh depth rendering), the yardstick of csrc/raster.hip, and the
test mesh: ref_icp's ellipsoid with a bump as two closed icospheres, so that ref_icp.render_into (an analytic ray-caster)
is a ground truth for the image.

The vertex stage is float32 in the written order, the triangle stage integer (Python / int64: exact), the depth float64
in the written parenthesisation. Triangles whose clipped box holds no sample are set aside with array operations (the
test is exact either way); the others are walked one by one.
"""
import numpy as np

import ref_icp as ri

F32 = np.float32


# ---- the mesh ---------------------------------------------------------------------------------------------------------
def icosphere(level):
    """Unit icosphere after `level` 1-to-4 subdivisions -> (V f64 [10 * 4^level + 2, 3], F int32 [20 * 4^level, 3]),
    closed, consistently wound (outward)."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
             (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(v, dtype=np.float64) / np.sqrt(1.0 + g * g) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
    for _ in range(level):
        middle = {}

        def mid(i, j):
            key = (i, j) if i < j else (j, i)
            if key not in middle:
                m = verts[i] + verts[j]
                verts.append(m / np.sqrt(m @ m))
                middle[key] = len(verts) - 1
            return middle[key]
        nxt = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nxt.extend(((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)))
        faces = nxt
    return np.stack(verts), np.asarray(faces, dtype=np.int32)


def ellipsoid_mesh(level):
    V, F = icosphere(level)
    return V * ri.AXES, F


def bump_mesh(level):
    """Ellipsoid (AXES) and bump (BUMP_R at BUMP_C) concatenated: 2 * 20 * 4^level triangles."""
    V, F = icosphere(level)
    return np.concatenate([V * ri.AXES, ri.BUMP_C + ri.BUMP_R * V]), np.concatenate([F, F + np.int32(len(V))])


# ---- SPEC 7 -------------------------------------------------------------------------------------------------------------
def vertex_stage(vertices, pose, cam_K, z_near, scale=1.0):
    """-> (sx int64 [V], sy int64 [V], rz f64 [V], usable bool [V]); unusable vertices carry zeros."""
    P = (np.asarray(vertices, dtype=np.float64) * float(scale)).astype(F32)
    T = np.asarray(pose, dtype=np.float64).astype(F32)
    fx, fy, cx, cy = F32(cam_K[0][0]), F32(cam_K[1][1]), F32(cam_K[0][2]), F32(cam_K[1][2])
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        X = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
        Y = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
        Z = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
        u = (X / Z) * fx + cx
        v = (Y / Z) * fy + cy
        ok = (Z > F32(z_near)) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(u) & np.isfinite(v)
        ok &= (np.abs(u) < F32(2.0 ** 20)) & (np.abs(v) < F32(2.0 ** 20))
        sx = np.rint(np.where(ok, u, F32(0)) * F32(256)).astype(np.int64)
        sy = np.rint(np.where(ok, v, F32(0)) * F32(256)).astype(np.int64)
        rz = np.where(ok, 1.0 / np.where(ok, Z, F32(1)).astype(np.float64), 0.0)
    return sx, sy, rz, ok


def _edge(ax, ay, bx, by, px, py):
    """Edge function of a -> b at the samples and the inside test with the ownership rule."""
    dx, dy = bx - ax, by - ay
    E = dx * (py - ay) - dy * (px - ax)
    if dy > 0 or (dy == 0 and dx < 0):
        return E, E >= 0
    return E, E > 0


def render(vertices, faces, pose, cam_K, hw, pixel_offset=0.5, z_near=0.05, scale=1.0):
    """-> (depth f32 [H,W], coverage count int32 [H,W], stats int64 [3] = unusable, degenerate, covering triangles)."""
    H, W = int(hw[0]), int(hw[1])
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    sx, sy, rz, ok = vertex_stage(vertices, pose, cam_K, z_near, scale)
    o = int(np.rint(256.0 * float(F32(pixel_offset))))
    depth = np.full((H, W), np.inf, dtype=F32)
    count = np.zeros((H, W), dtype=np.int32)
    stats = np.zeros(3, dtype=np.int64)
    if len(faces) == 0:
        return np.zeros((H, W), dtype=F32), count, stats
    usable = ok[faces].all(1)
    stats[0] = int((~usable).sum())
    tx, ty = sx[faces], sy[faces]
    area = (tx[:, 1] - tx[:, 0]) * (ty[:, 2] - ty[:, 0]) - (ty[:, 1] - ty[:, 0]) * (tx[:, 2] - tx[:, 0])
    stats[1] = int((usable & (area == 0)).sum())
    # pixel x is sampled at 256 x + o: those with min <= 256 x + o <= max, inside the frame
    xa = np.maximum(0, -((-(tx.min(1) - o)) // 256))
    xb = np.minimum(W - 1, (tx.max(1) - o) // 256)
    ya = np.maximum(0, -((-(ty.min(1) - o)) // 256))
    yb = np.minimum(H - 1, (ty.max(1) - o) // 256)
    todo = np.nonzero(usable & (area != 0) & (xa <= xb) & (ya <= yb))[0]
    for k in todo:
        i0, i1, i2 = (int(i) for i in faces[k])
        A = int(area[k])
        if A < 0:
            i1, i2, A = i2, i1, -A
        x0, y0, x1, y1, x2, y2 = (int(q) for q in (sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]))
        px = (np.arange(int(xa[k]), int(xb[k]) + 1, dtype=np.int64) * 256 + o)[None, :]
        py = (np.arange(int(ya[k]), int(yb[k]) + 1, dtype=np.int64) * 256 + o)[:, None]
        w0, in0 = _edge(x1, y1, x2, y2, px, py)
        w1, in1 = _edge(x2, y2, x0, y0, px, py)
        w2, in2 = _edge(x0, y0, x1, y1, px, py)
        inside = in0 & in1 & in2
        if not inside.any():
            continue
        stats[2] += 1
        den = (w0.astype(np.float64) * rz[i0] + w1.astype(np.float64) * rz[i1]) + w2.astype(np.float64) * rz[i2]
        z = (float(A) / den[inside]).astype(F32)
        win = depth[int(ya[k]):int(yb[k]) + 1, int(xa[k]):int(xb[k]) + 1]
        win[inside] = np.minimum(win[inside], z)
        count[int(ya[k]):int(yb[k]) + 1, int(xa[k]):int(xb[k]) + 1] += inside
    depth[np.isinf(depth)] = F32(0)
    return depth, count, stats


# ---- image helpers for the comparisons with the analytic ray-caster ---------------------------------------------------
def dilate(mask, r=1):
    """True where a True pixel lies within Chebyshev distance r."""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape
    p = np.pad(m, r)
    out = np.zeros_like(m)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def boundary_band(mask):
    """Pixels within one pixel (Chebyshev) of the silhouette's boundary: a pixel of the other class in their 3x3."""
    m = np.asarray(mask, dtype=bool)
    return dilate(m) & dilate(~m)


def interior(mask, r=2):
    """Covered pixels with no uncovered pixel within Chebyshev distance r."""
    m = np.asarray(mask, dtype=bool)
    return m & ~dilate(~m, r)


def pose_at(t, axis=(0.3, 1.0, 0.2), deg=25.0):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ri.rot(axis, deg), t
    return T
