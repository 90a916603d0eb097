"""Independent numpy restatement of SPEC.md 7.11-7.14 (colour rendering of a vertex-coloured mesh and the template
stage), the yardstick of ossid_raster_color / ossid_template_reduce in csrc/raster.hip. Built on ref_raster's vertex
stage and edge functions; triangles are walked one by one, as ref_raster.render does.

The visibility rule is written as a comparison, not as a packed key: a sample is taken by the triangle with the smaller
f32 depth and, at equal depth, the lower face index.
"""
import numpy as np

import ref_raster as rr

F32 = np.float32


def cam_matrix(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)


def render(vertices, faces, colors, pose, cam_K, hw, pixel_offset=0.5, z_near=0.05, scale=1.0, affine=False):
    """-> (color u8 [H,W,3], depth f32 [H,W], face_id int32 [H,W] (-1 = nothing drawn), stats int64 [3]).
    affine=True interpolates with b_i = w_i (screen-linear: wrong on purpose, for the test of perspective-correctness)."""
    H, W = int(hw[0]), int(hw[1])
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    colors = np.asarray(colors)
    assert colors.dtype == np.uint8 and colors.shape == (len(vertices), 3)
    col = colors.astype(np.float64)
    sx, sy, rz, ok = rr.vertex_stage(vertices, pose, cam_K, z_near, scale)
    o = int(np.rint(256.0 * float(F32(pixel_offset))))
    depth = np.full((H, W), np.inf, dtype=F32)
    face_id = np.full((H, W), -1, dtype=np.int32)
    image = np.zeros((H, W, 3), dtype=np.uint8)
    stats = np.zeros(3, dtype=np.int64)
    if len(faces) == 0:
        return image, np.zeros((H, W), dtype=F32), face_id, stats
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
        x0, y0, x1, y1, x2, y2 = (int(q) for q in (sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]))
        px = (np.arange(int(xa[k]), int(xb[k]) + 1, dtype=np.int64) * 256 + o)[None, :]
        py = (np.arange(int(ya[k]), int(yb[k]) + 1, dtype=np.int64) * 256 + o)[:, None]
        w0, in0 = rr._edge(x1, y1, x2, y2, px, py)
        w1, in1 = rr._edge(x2, y2, x0, y0, px, py)
        w2, in2 = rr._edge(x0, y0, x1, y1, px, py)
        inside = in0 & in1 & in2
        if not inside.any():
            continue
        stats[2] += 1
        w0, w1, w2 = (w.astype(np.float64) for w in (w0, w1, w2))
        b0, b1, b2 = w0 * rz[i0], w1 * rz[i1], w2 * rz[i2]
        with np.errstate(all="ignore"):
            z = (float(A) / ((b0 + b1) + b2)).astype(F32)
        sl = (slice(int(ya[k]), int(yb[k]) + 1), slice(int(xa[k]), int(xb[k]) + 1))
        dwin, fwin, iwin = depth[sl], face_id[sl], image[sl]
        take = inside & ((z < dwin) | ((z == dwin) & (k < fwin)))
        if not take.any():
            continue
        if affine:
            b0, b1, b2 = w0, w1, w2
        den = (b0 + b1) + b2
        for ch in range(3):
            with np.errstate(all="ignore"):
                a = ((b0 * col[i0, ch] + b1 * col[i1, ch]) + b2 * col[i2, ch]) / den
            iwin[..., ch][take] = np.clip(np.rint(a[take]), 0, 255).astype(np.uint8)
        dwin[take] = z[take]
        fwin[take] = k
    depth[np.isinf(depth)] = F32(0)
    return image, depth, face_id, stats


def box_reduce(color, depth, s):
    """SPEC 7.13: color u8 [S,S,3], depth f32 [S,S], S = s T -> (img f32 [3,T,T], mask f32 [1,T,T])."""
    S = color.shape[0]
    assert color.shape == (S, S, 3) and depth.shape == (S, S) and S % s == 0 and color.dtype == np.uint8
    T = S // s
    cov = depth > 0
    c = np.where(cov[..., None], color.astype(np.int64), 0).reshape(T, s, T, s, 3).sum((1, 3))
    n = cov.reshape(T, s, T, s).sum((1, 3))
    q = (c + (s * s) // 2) // (s * s)
    img = (q.astype(F32) / F32(255.0)).transpose(2, 0, 1)
    mask = (n.astype(F32) / F32(s * s))[None]
    return np.ascontiguousarray(img), mask


def template(vertices, faces, colors, rotation, distance, intrinsics, size, s, z_near=0.05, scale=1.0):
    """One view of SPEC 7.14 through its virtual camera (intrinsics = fx, fy, cx, cy at s * size) -> (img, mask)."""
    pose = np.eye(4)
    pose[:3, :3], pose[2, 3] = rotation, distance
    S = s * size
    color, depth, _f, _s = render(vertices, faces, colors, pose, cam_matrix(*[float(v) for v in intrinsics]), (S, S), 0.5,
                                  z_near, scale)
    return box_reduce(color, depth, s)


def framing(vertices_f32, rotations, distance, cam_K, size, s, pad=1.1):
    """SPEC 7.14 in numpy float64 -> (intrinsics f64 [n,4], template_z f64 [n])."""
    P = np.asarray(vertices_f32, dtype=np.float32).astype(np.float64)
    S = s * size
    out, tz = [], []
    for R in np.asarray(rotations, dtype=np.float64):
        C = P @ R.T
        Z = C[:, 2] + distance
        m = max(np.abs(cam_K[0][0] * C[:, 0] / Z).max(), np.abs(cam_K[1][1] * C[:, 1] / Z).max())
        h = max(pad * m, 5.0)
        out.append([cam_K[0][0] * S / (2 * h), cam_K[1][1] * S / (2 * h), S / 2.0, S / 2.0])
        tz.append(-distance * 2 * h / size)
    return np.array(out), np.array(tz)


def axis_colors(V):
    """The test colouring of the issue: channel c = rint(255 (0.5 + k_c x_c)), k_c = 0.45 / max|x_c| -> (u8 [V,3], k [3])."""
    V = np.asarray(V, dtype=np.float64)
    k = 0.45 / np.abs(V).max(0)
    return np.rint(255.0 * (0.5 + k * V)).astype(np.uint8), k
