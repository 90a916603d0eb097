"""A numpy restatement of SPEC.md 13.16 and 13.18 (csrc/scene_rest.hip): the support heights of a mesh, the height-field
drop and the composition of a rest layout's transforms. Float64 throughout, in the written order of operations, rounded up
to float32 exactly where the kernel rounds: test infrastructure, slow and plain. Every result is a maximum, so the loops'
order does not matter and the device's results are these bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64


def support_heights(vertices, dirs):
    """13.16 -> f64 [D]: per direction the largest ((dx x + dy y) + dz z) over the vertices with three finite coordinates,
    from the (double) f32 coordinates; -inf without one. A term that is NaN never replaces the running maximum."""
    V = np.asarray(vertices, dtype=F32).reshape(-1, 3)
    V = V[np.isfinite(V).all(1)].astype(F64)
    D = np.asarray(dirs, dtype=F64).reshape(-1, 3)
    h = np.full(len(D), -np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(len(D)):
            t = (D[d, 0] * V[:, 0] + D[d, 1] * V[:, 1]) + D[d, 2] * V[:, 2]
            t = t[~np.isnan(t)]
            if len(t):
                h[d] = t.max()
    return h


def round_up_f32(v):
    """The nearest f32 at or above the f64 v >= 0."""
    with np.errstate(over="ignore"):
        f = F32(v)
    if F64(f) < v:
        f = np.nextafter(f, F32(np.inf))
    return f


def _cell_range(lo, hi, x0, cell, G):
    """-> (first, last, outside): floor((lo - x0) / cell) .. floor((hi - x0) / cell) clipped to [0, G - 1] (first > last:
    empty) and whether an unclipped index lies outside."""
    with np.errstate(over="ignore"):
        fa, fb = np.floor((lo - x0) / cell), np.floor((hi - x0) / cell)
    outside = bool(fa < 0.0 or fb > G - 1)
    if fb < 0.0 or fa > G - 1:
        return 0, -1, outside
    return int(max(fa, 0.0)), int(min(fb, float(G - 1))), outside


def triangles(mesh, L, G, cell):
    """The usable triangles of one instance in the table frame -> list of (zmin, zmax, ix0, ix1, iy0, iy1, outside); the
    box is empty (ix0 > ix1) when no cell of it is in the grid. mesh = (vertices f32 [V,3], faces int [F,3])."""
    V = np.asarray(mesh[0], dtype=F32).reshape(-1, 3).astype(F64)
    F = np.asarray(mesh[1]).reshape(-1, 3).astype(np.int64)
    L = np.asarray(L, dtype=F64).reshape(3, 4)
    x0 = -(float(G) * 0.5) * float(cell)
    with np.errstate(invalid="ignore", over="ignore"):
        P = np.stack([((L[c, 0] * V[:, 0] + L[c, 1] * V[:, 1]) + L[c, 2] * V[:, 2]) + L[c, 3] for c in range(3)], 1)
    out = []
    for f in F:
        if f.min() < 0 or f.max() >= len(V):
            continue
        p = P[f]
        if not np.isfinite(p).all():
            continue
        ax, bx, ox = _cell_range(p[:, 0].min(), p[:, 0].max(), x0, cell, G)
        ay, by, oy = _cell_range(p[:, 1].min(), p[:, 1].max(), x0, cell, G)
        if ax > bx or ay > by:
            ax, bx, ay, by = 0, -1, 0, -1
        out.append((p[:, 2].min(), p[:, 2].max(), ax, bx, ay, by, ox or oy))
    return out


def drop(meshes, instance_mesh, scene_first, local, G, cell, history=None):
    """13.18 -> (drop f64 [I], status int32 [I], height f32 [S,G,G]). meshes: list of (vertices, faces) per atlas row; an
    instance_mesh outside it, like a mesh without a usable triangle, gives status 1 and drop 0. history, a list, receives
    per instance (scene, H before it f32 [G,G], its triangles, its offset) for the tests of the guarantee."""
    instance_mesh = np.asarray(instance_mesh).reshape(-1)
    scene_first = np.asarray(scene_first).reshape(-1)
    local = np.asarray(local, dtype=F64).reshape(-1, 3, 4)
    I, S = len(instance_mesh), len(scene_first) - 1
    out_drop, status = np.zeros(I), np.zeros(I, np.int32)
    height = np.zeros((S, G, G), F32)
    for s in range(S):
        H = height[s]
        a, b = int(scene_first[s]), int(scene_first[s + 1])
        if a < 0 or b > I or a > b:
            continue
        for i in range(a, b):
            m = int(instance_mesh[i])
            tris = triangles(meshes[m], local[i], G, cell) if 0 <= m < len(meshes) else []
            if not tris:
                status[i] = 1
                continue
            off = -min(t[0] for t in tris)
            for zmin, _zmax, ax, bx, ay, by, _o in tris:
                if ax <= bx:
                    off = max(off, float((H[ay:by + 1, ax:bx + 1].astype(F64) - zmin).max()))
            if history is not None:
                history.append((s, H.copy(), tris, off))
            for _zmin, zmax, ax, bx, ay, by, _o in tris:
                if ax <= bx:
                    v = round_up_f32(zmax + off)
                    H[ay:by + 1, ax:bx + 1] = np.maximum(H[ay:by + 1, ax:bx + 1], v)
            out_drop[i] = off
            status[i] = 2 if any(t[6] for t in tris) else 0
    return out_drop, status, height


def compose(table_pose, drop_i, local_i):
    """13.18 -> f64 [4,4]: table_pose . translate(0, 0, drop) . local (completed by the row 0 0 0 1)."""
    M, D = np.eye(4), np.eye(4)
    M[:3] = np.asarray(local_i, dtype=F64).reshape(3, 4)
    D[2, 3] = float(drop_i)
    return np.asarray(table_pose, dtype=F64).reshape(4, 4) @ (D @ M)


def cube(h):
    """The cube [-h, h]^3: (vertices f32 [8,3], faces int32 [12,3])."""
    V = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], F32)
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int32)
    return V, F


def box(a, b, c):
    """The box of edges a x b x c about the origin."""
    V, F = cube(0.5)
    return (V * np.array([a, b, c], F32)).astype(F32), F


def place(x=0.0, y=0.0, R=None, scale=1.0):
    """A local map f64 [3,4]: rotation (identity) times scale, the position (x, y) and a z' translation of 0."""
    L = np.zeros((3, 4))
    L[:, :3] = (np.eye(3) if R is None else np.asarray(R, dtype=F64)) * float(scale)
    L[0, 3], L[1, 3] = x, y
    return L
