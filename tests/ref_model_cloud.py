"""Independent numpy restatement of SPEC.md section 9 (the model cloud from a mesh), the yardstick of csrc/model_cloud.hip.

Everything is float64 in the written parenthesisation (numpy does not contract a * b - c * d), integers are Python / uint64,
the thinning is float32. Each function takes the PREVIOUS stage's output, so a test can restate stage by stage from what the
kernels produced; sample() chains them and renders the views itself with ref_raster_color through the cameras it is given.
"""
import numpy as np

import ref_raster_color as rc

F32 = np.float32
R1, R2 = 3242174889, 2447445413            # 9.4: round(2^32 / g), round(2^32 / g^2), g the plastic number; both odd
TWO32 = 4294967296.0


def f32_vertices(vertices, scale=1.0):
    """Mesh's rule: f32(v * scale), the product in float64."""
    return (np.asarray(vertices, dtype=np.float64) * float(scale)).astype(F32)


def face_cross(V32, faces):
    """g = (p1 - p0) x (p2 - p0) in f64 from the f32 vertices, each component a b - c d -> (g [F,3], p0, p1, p2)."""
    P = np.asarray(V32, dtype=F32).astype(np.float64)
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    p0, p1, p2 = P[Fc[:, 0]], P[Fc[:, 1]], P[Fc[:, 2]]
    a, b = p1 - p0, p2 - p0
    g = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return g, p0, p1, p2


def camera_centres(rotations, distance):
    """c_v = -R_v^T (0, 0, distance): minus `distance` times the third row of R_v."""
    R = np.asarray(rotations, dtype=np.float64)
    return -(R[:, 2, :] * float(distance))


def votes(face_id, V32, faces, centres):
    """9.2: face_id int [n,H,W] -> votes int64 [F,2]."""
    g, p0, _p1, _p2 = face_cross(V32, faces)
    F = len(g)
    out = np.zeros((F, 2), dtype=np.int64)
    for v, img in enumerate(np.asarray(face_id)):
        ids = img[(img >= 0) & (img < F)].astype(np.int64)
        n = np.bincount(ids, minlength=F)
        c = np.asarray(centres[v], dtype=np.float64)
        with np.errstate(all="ignore"):
            t = (g[:, 0] * (c[0] - p0[:, 0]) + g[:, 1] * (c[1] - p0[:, 1])) + g[:, 2] * (c[2] - p0[:, 2])
        front = t >= 0
        out[front, 0] += n[front]
        out[~front, 1] += n[~front]
    return out


def weights(V32, faces, votes_):
    """9.3 -> (w uint64 [F], P uint64 [F], normals f32 [F,3], usable bool [F])."""
    g, _p0, _p1, _p2 = face_cross(V32, faces)
    vt = np.asarray(votes_, dtype=np.int64)
    with np.errstate(all="ignore"):
        s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        usable = ((vt[:, 0] > 0) | (vt[:, 1] > 0)) & np.isfinite(s) & (s > 0)
        A = np.where(usable, np.sqrt(np.where(usable, s, 1.0)), 0.0)
    w = np.zeros(len(g), dtype=np.uint64)
    nrm = np.zeros((len(g), 3), dtype=F32)
    if usable.any():
        Amax = A.max()
        w[usable] = np.floor((A[usable] / Amax) * TWO32).astype(np.uint64)
        q = g[usable] / A[usable, None]
        flip = (vt[:, 1] > vt[:, 0])[usable]
        nrm[usable] = np.where(flip[:, None], -q, q).astype(F32)
    P = np.cumsum(w, dtype=np.uint64)
    return w, P, nrm, usable


def strata(Wt, K):
    """9.4: tau_k = q k + q div 2, q = Wt div K, as Python integers."""
    q = int(Wt) // int(K)
    return [q * k + q // 2 for k in range(int(K))]


def barycentric(K):
    """9.4 -> (w0, u, v) f64 [K] from the integer R2 sequence."""
    k = np.arange(int(K), dtype=np.uint64)
    r1 = (k * np.uint64(R1)) & np.uint64(0xFFFFFFFF)
    r2 = (k * np.uint64(R2)) & np.uint64(0xFFFFFFFF)
    u = (r1.astype(np.float64) + 0.5) / TWO32
    v = (r2.astype(np.float64) + 0.5) / TWO32
    fold = u + v > 1.0
    u = np.where(fold, 1.0 - u, u)
    v = np.where(fold, 1.0 - v, v)
    return (1.0 - u) - v, u, v


def candidates(V32, faces, colors, votes_, P, normals, K):
    """9.4 -> (points f32 [K,3], normals f32 [K,3], colors f32 [K,3], face int32 [K]). A face whose votes say it is
    wound inwards is read as (p0, p2, p1)."""
    Pint = [int(x) for x in np.asarray(P)]
    tau = strata(Pint[-1], K)
    face = np.searchsorted(np.asarray(P, dtype=np.uint64), np.asarray(tau, dtype=np.uint64), side="right").astype(np.int64)
    for k in (0, K // 2, K - 1):                                   # searchsorted against the definition
        f = int(face[k])
        assert Pint[f] > tau[k] and (f == 0 or Pint[f - 1] <= tau[k])
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face]
    vt = np.asarray(votes_, dtype=np.int64)[face]
    flip = vt[:, 1] > vt[:, 0]
    i0, i1, i2 = Fc[:, 0], np.where(flip, Fc[:, 2], Fc[:, 1]), np.where(flip, Fc[:, 1], Fc[:, 2])
    w0, u, v = barycentric(K)
    Pv = np.asarray(V32, dtype=F32).astype(np.float64)
    C = np.asarray(colors).astype(np.float64)
    pts = ((w0[:, None] * Pv[i0] + u[:, None] * Pv[i1]) + v[:, None] * Pv[i2]).astype(F32)
    a = (w0[:, None] * C[i0] + u[:, None] * C[i1]) + v[:, None] * C[i2]
    col = np.clip(np.rint(a), 0.0, 255.0).astype(F32) / F32(255.0)
    return pts, np.asarray(normals, dtype=F32)[face], col, face.astype(np.int32)


def fps(points, M):
    """9.5 -> (selection int32 [M], radius f32 [M])."""
    P = np.asarray(points, dtype=F32)
    tmp = np.full(len(P), np.inf, dtype=F32)
    sel = np.zeros(M, dtype=np.int32)
    rad = np.full(M, np.inf, dtype=F32)
    cur = 0
    for j in range(1, M):
        dx, dy, dz = P[:, 0] - P[cur, 0], P[:, 1] - P[cur, 1], P[:, 2] - P[cur, 2]
        with np.errstate(over="ignore"):
            d = (dx * dx + dy * dy) + dz * dz
        tmp = np.minimum(tmp, d)
        cur = int(tmp.argmax())                                    # the first occurrence: the lowest index
        sel[j], rad[j] = cur, tmp[cur]
    return sel, rad


def diameter(V32):
    """9.6 -> (D^2, D), brute force in f64 over the f32 vertices."""
    P = np.asarray(V32, dtype=F32).astype(np.float64)
    best = 0.0
    for a in range(0, len(P), 256):
        d = P[a:a + 256, None, :] - P[None, :, :]
        best = max(best, float(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max()))
    return best, float(np.sqrt(best))


def sample(vertices, faces, colors, rotations, intrinsics, distance, z_near, S, M, K, scale=1.0):
    """Section 9 end to end, rendering through the given virtual cameras -> dict of every stage."""
    V32 = f32_vertices(vertices, scale)
    ids = []
    for R, cam in zip(rotations, intrinsics):
        pose = np.eye(4)
        pose[:3, :3], pose[2, 3] = R, distance
        _c, _d, fid, _s = rc.render(vertices, faces, colors, pose, rc.cam_matrix(*[float(x) for x in cam]), (S, S), 0.5,
                                    z_near, scale)
        ids.append(fid)
    vt = votes(np.stack(ids), V32, faces, camera_centres(rotations, distance))
    w, P, nrm, _u = weights(V32, faces, vt)
    pts, cn, col, face = candidates(V32, faces, colors, vt, P, nrm, K)
    sel, rad = fps(pts, M)
    return {"votes": vt, "weights": w, "prefix": P, "face_normals": nrm, "points": pts, "normals": cn, "colors": col,
            "face": face, "selection": sel, "radius": rad, "model_points": pts[sel], "model_normals": cn[sel],
            "model_colors": col[sel]}
