"""Independent numpy restatement of SPEC.md 7.15-7.17 and 9.4.1 (texture-mapped meshes: the mip chain, level selection,
the clamp-to-edge bilinear fetch, the textured resolve and the textured cloud colours), the yardstick of
ossid_texture_mips / ossid_raster_textured / ossid_cloud_candidates_textured. Built on ref_raster's vertex stage and edge
functions and on ref_raster_color's visibility rule; triangles are walked one by one, as ref_raster_color.render does.

No log2 or pow anywhere: a level is found by comparing with exact powers of two.
"""
import numpy as np

import ref_model_cloud as rm
import ref_raster as rr

F32 = np.float32


# ---- 7.15 the mip chain -------------------------------------------------------------------------------------------------
def mip_chain(image):
    """u8 [Ht,Wt,3] -> list of u8 [h_l,w_l,3], level 0 the image, each level the rounded 2 x 2 box of the one before it
    (rows / columns 2y+1, 2x+1 clamped to the last), down to 1 x 1."""
    img = np.asarray(image)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] >= 1 and img.shape[1] >= 1
    levels = [np.ascontiguousarray(img)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        p = levels[-1].astype(np.int64)
        h, w = p.shape[:2]
        y0 = 2 * np.arange((h + 1) >> 1)
        x0 = 2 * np.arange((w + 1) >> 1)
        y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
        q = (p[y0][:, x0] + p[y0][:, x1] + p[y1][:, x0] + p[y1][:, x1] + 2) // 4
        levels.append(q.astype(np.uint8))
    return levels


def mip_buffer(levels):
    """The caller's buffer of ossid_texture_mips: the levels one after the other, 4 bytes per texel (R, G, B, 0) -> u8 [n]."""
    out = []
    for lv in levels:
        t = np.zeros(lv.shape[:2] + (4,), dtype=np.uint8)
        t[..., :3] = lv
        out.append(t.reshape(-1))
    return np.concatenate(out)


def top_level(Ht, Wt):
    l = 0
    while Ht > 1 or Wt > 1:
        Ht, Wt, l = (Ht + 1) >> 1, (Wt + 1) >> 1, l + 1
    return l


# ---- 7.16-7.17 level and fetch ---------------------------------------------------------------------------------------------
def select_level(rho, top):
    """The smallest l with rho <= 2^l, at most top (rho finite, >= 0) -> int64 array."""
    rho = np.asarray(rho, dtype=np.float64)
    lod = np.zeros(rho.shape, dtype=np.int64)
    p = 1.0
    for _ in range(int(top)):
        lod += rho > p
        p *= 2.0
    return lod


def bilinear(level, u, v):
    """Clamp-to-edge bilinear fetch of one level u8 [h,w,3] at (u, v) f64 [...], v upwards -> f64 [...,3], unrounded;
    0 where s or t is not finite."""
    h, w = level.shape[:2]
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = u * float(w) - 0.5
        t = (1.0 - v) * float(h) - 0.5
    ok = np.isfinite(s) & np.isfinite(t)
    s, t = np.where(ok, s, 0.0), np.where(ok, t, 0.0)
    fs, ft = np.floor(s), np.floor(t)
    wx, wy = s - fs, t - ft
    x0 = np.clip(fs, 0, w - 1).astype(np.int64)
    x1 = np.clip(fs + 1.0, 0, w - 1).astype(np.int64)
    y0 = np.clip(ft, 0, h - 1).astype(np.int64)
    y1 = np.clip(ft + 1.0, 0, h - 1).astype(np.int64)
    p = level.astype(np.float64)
    w00, w10, w01, w11 = (1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy
    val = (p[y0, x0] * w00[..., None] + p[y0, x1] * w10[..., None]) + (p[y1, x0] * w01[..., None] + p[y1, x1] * w11[..., None])
    return np.where(ok[..., None], val, 0.0)


def round_u8(a):
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def _uv_at(tri, rz3, uv3, px, py, affine):
    """(u, v, den) of the triangle (x0, y0, x1, y1, x2, y2) after the swap at the samples (px, py)."""
    x0, y0, x1, y1, x2, y2 = tri
    w0, _ = rr._edge(x1, y1, x2, y2, px, py)
    w1, _ = rr._edge(x2, y2, x0, y0, px, py)
    w2, _ = rr._edge(x0, y0, x1, y1, px, py)
    w0, w1, w2 = (w.astype(np.float64) for w in (w0, w1, w2))
    b0, b1, b2 = (w0, w1, w2) if affine else (w0 * rz3[0], w1 * rz3[1], w2 * rz3[2])
    den = (b0 + b1) + b2
    with np.errstate(all="ignore"):
        u = ((b0 * uv3[0][0] + b1 * uv3[1][0]) + b2 * uv3[2][0]) / den
        v = ((b0 * uv3[0][1] + b1 * uv3[1][1]) + b2 * uv3[2][1]) / den
    return u, v, den


def render(vertices, faces, uvs, levels, pose, cam_K, hw, pixel_offset=0.5, z_near=0.05, scale=1.0, affine=False,
           force_lod=None):
    """-> (color u8 [H,W,3], depth f32 [H,W], face_id int32 [H,W], lod int32 [H,W] (-1 = nothing drawn), stats int64 [3]).
    levels = mip_chain(texture). affine=True interpolates the UVs with b_i = w_i (screen-linear: wrong on purpose);
    force_lod fetches every pixel at that level (the test of minification)."""
    H, W = int(hw[0]), int(hw[1])
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    uv = np.asarray(uvs, dtype=F32).astype(np.float64)
    assert uv.shape == (len(vertices), 2)
    Ht, Wt = levels[0].shape[:2]
    top = len(levels) - 1
    assert top == top_level(Ht, Wt)
    sx, sy, rz, ok = rr.vertex_stage(vertices, pose, cam_K, z_near, scale)
    o = int(np.rint(256.0 * float(F32(pixel_offset))))
    depth = np.full((H, W), np.inf, dtype=F32)
    face_id = np.full((H, W), -1, dtype=np.int32)
    lod = np.full((H, W), -1, dtype=np.int32)
    U, Vv = np.zeros((H, W)), np.zeros((H, W))
    image = np.zeros((H, W, 3), dtype=np.uint8)
    stats = np.zeros(3, dtype=np.int64)
    if len(faces) == 0:
        return image, np.zeros((H, W), dtype=F32), face_id, lod, stats
    usable = ok[faces].all(1)
    stats[0] = int((~usable).sum())
    tx, ty = sx[faces], sy[faces]
    area = (tx[:, 1] - tx[:, 0]) * (ty[:, 2] - ty[:, 0]) - (ty[:, 1] - ty[:, 0]) * (tx[:, 2] - tx[:, 0])
    stats[1] = int((usable & (area == 0)).sum())
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
        tri = tuple(int(q) for q in (sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]))
        x0, y0, x1, y1, x2, y2 = tri
        px = (np.arange(int(xa[k]), int(xb[k]) + 1, dtype=np.int64) * 256 + o)[None, :]
        py = (np.arange(int(ya[k]), int(yb[k]) + 1, dtype=np.int64) * 256 + o)[:, None]
        w0, in0 = rr._edge(x1, y1, x2, y2, px, py)
        w1, in1 = rr._edge(x2, y2, x0, y0, px, py)
        w2, in2 = rr._edge(x0, y0, x1, y1, px, py)
        inside = in0 & in1 & in2
        if not inside.any():
            continue
        stats[2] += 1
        b0, b1, b2 = w0.astype(np.float64) * rz[i0], w1.astype(np.float64) * rz[i1], w2.astype(np.float64) * rz[i2]
        with np.errstate(all="ignore"):
            z = (float(A) / ((b0 + b1) + b2)).astype(F32)
        sl = (slice(int(ya[k]), int(yb[k]) + 1), slice(int(xa[k]), int(xb[k]) + 1))
        dwin, fwin = depth[sl], face_id[sl]
        take = inside & ((z < dwin) | ((z == dwin) & (k < fwin)))
        if not take.any():
            continue
        rz3, uv3 = (rz[i0], rz[i1], rz[i2]), (uv[i0], uv[i1], uv[i2])
        u, v, _den = _uv_at(tri, rz3, uv3, px, py, affine)
        ux, vx, denx = _uv_at(tri, rz3, uv3, px + 256, py, affine)
        uy, vy, deny = _uv_at(tri, rz3, uv3, px, py + 256, affine)
        with np.errstate(all="ignore"):
            d = [np.abs((ux - u) * float(Wt)), np.abs((vx - v) * float(Ht)), np.abs((uy - u) * float(Wt)),
                 np.abs((vy - v) * float(Ht))]
        fine = (denx > 0.0) & (deny > 0.0) & np.isfinite(d[0]) & np.isfinite(d[1]) & np.isfinite(d[2]) & np.isfinite(d[3])
        rho = np.where(fine, np.maximum(np.maximum(d[0], d[1]), np.maximum(d[2], d[3])), 0.0)
        level = np.where(fine, select_level(rho, top), top)
        u, v = np.broadcast_to(u, take.shape), np.broadcast_to(v, take.shape)
        U[sl][take], Vv[sl][take], lod[sl][take] = u[take], v[take], level[take]
        dwin[take] = z[take]
        fwin[take] = k
    depth[np.isinf(depth)] = F32(0)
    fetch = lod if force_lod is None else np.where(lod >= 0, int(force_lod), -1)
    for l in range(top + 1):
        m = fetch == l
        if m.any():
            image[m] = round_u8(bilinear(levels[l], U[m], Vv[m]))
    return image, depth, face_id, lod, stats


# ---- 9.4.1 the textured cloud ------------------------------------------------------------------------------------------------
def cloud_colors(faces, uvs, votes_, face, levels, lod):
    """Colours f32 [K,3] of the candidates whose faces are `face` (ref_model_cloud.candidates' fourth output): the UVs
    interpolated affinely with 9.4's barycentrics in the voted orientation, one bilinear fetch at level lod."""
    face = np.asarray(face, dtype=np.int64)
    K = len(face)
    uv = np.asarray(uvs, dtype=F32).astype(np.float64)
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face]
    vt = np.asarray(votes_, dtype=np.int64)[face]
    flip = vt[:, 1] > vt[:, 0]
    i0, i1, i2 = Fc[:, 0], np.where(flip, Fc[:, 2], Fc[:, 1]), np.where(flip, Fc[:, 1], Fc[:, 2])
    w0, u, v = rm.barycentric(K)
    t = (w0[:, None] * uv[i0] + u[:, None] * uv[i1]) + v[:, None] * uv[i2]
    return round_u8(bilinear(levels[int(lod)], t[:, 0], t[:, 1])).astype(F32) / F32(255.0)


def default_cloud_lod(V32, faces, uvs, Ht, Wt, M):
    """9.4.1's host rule: the smallest level whose texel (2^l x the median over faces with positive UV area of
    sqrt(area_3d / area_uv_texels)) is at least half the nominal spacing sqrt(total area / M); at most the top level."""
    P = np.asarray(V32, dtype=F32).astype(np.float64)
    uv = np.asarray(uvs, dtype=F32).astype(np.float64)
    Fc = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    g = np.cross(P[Fc[:, 1]] - P[Fc[:, 0]], P[Fc[:, 2]] - P[Fc[:, 0]])
    a3 = 0.5 * np.sqrt((g * g).sum(1))
    e1, e2 = uv[Fc[:, 1]] - uv[Fc[:, 0]], uv[Fc[:, 2]] - uv[Fc[:, 0]]
    at = 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) * float(Wt) * float(Ht)
    pos = np.isfinite(at) & (at > 0.0) & np.isfinite(a3)
    if not pos.any():
        return 0
    texel = float(np.median(np.sqrt(a3[pos] / at[pos])))
    spacing = float(np.sqrt(a3[np.isfinite(a3)].sum() / float(M)))
    l, top = 0, top_level(Ht, Wt)
    while l < top and texel < 0.5 * spacing:
        texel, l = 2.0 * texel, l + 1
    return l
