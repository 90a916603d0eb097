"""Independent numpy restatement of SPEC.md 13.13 (shadow maps), 13.14 (the shadowed shading pass) and 13.15 (the lights'
views), the yardstick of csrc/scene_shadow.hip, of ossid_scene_light_shadowed and of scenes.shadow_views, built on
ref_scene's camera points and ref_scene_light's conventions.

The edge functions are Python integers (object arrays: exact whatever the magnitude); every float64 expression is written
in the SPEC's parenthesisation and numpy rounds each operation once. The map is a minimum over float32 depths taken by
comparison -- no bit pattern is ordered anywhere -- and turned into bits at the end. The pass is evaluated per instance
over that instance's pixels at once: every step is elementwise, so the vectorisation changes no bit.
"""
import numpy as np

import ref_raster as rr
import ref_scene as rs
import ref_scene_light as rl

F32 = np.float32
MAX_LIGHTS = rl.MAX_LIGHTS
ZFAR = np.uint32(0x7F800000)
FACES_PER_ITEM = 64
Z_NEAR_L = 1e-3


# ---- SPEC 13.15 -----------------------------------------------------------------------------------------------------------------
def _norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def views(radius, n_faces, instance_mesh, transforms, scene_first, table, lights, n_lights, size):
    """radius, n_faces: per mesh of the atlas; table: the atlas index of the table -> (views f32 [S,4,16], enable int32
    [S,4], items int32 [n,3])."""
    Hs, Ws = size
    S = len(scene_first) - 1
    lights = np.asarray(lights, dtype=F32).reshape(S, MAX_LIGHTS, 8).astype(np.float64)
    T = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    out, enable = np.zeros((S, MAX_LIGHTS, 16)), np.zeros((S, MAX_LIGHTS), np.int32)
    for s in range(S):
        objs = [i for i in range(int(scene_first[s]), int(scene_first[s + 1])) if int(instance_mesh[i]) != table]
        if not objs:
            continue
        c = sum(T[i, :3, 3] for i in objs) / float(len(objs))
        r = max(float(_norm(T[i, :3, 3] - c) + radius[int(instance_mesh[i])]) for i in objs)
        if not (r > 0.0 and np.isfinite(r)):
            continue
        big = 1.05 * r
        for l in range(int(n_lights[s])):
            g = lights[s, l, :3]
            if lights[s, l, 3] != 0.0:
                D = float(_norm(c - g))
                if not D > 1.1 * r:
                    continue
                eye, f = g, (c - g) / D
                a = 0.5 * min(Hs, Ws) * np.sqrt(D * D - big * big) / big
            else:
                if not _norm(g) > 0.0:
                    continue
                d = g / _norm(g)
                eye, f = c + big * d, -d
                a = 0.5 * min(Hs, Ws) / big
            k = min(range(3), key=lambda j: (abs(f[j]), j))           # the smallest |e_k . f|, the lowest k on a tie
            up = np.zeros(3)
            up[k] = 1.0
            x = np.cross(up, f)
            x = x / _norm(x)
            y = np.cross(f, x)
            R = np.stack([x, y, f])
            t = -np.array([(R[j, 0] * eye[0] + R[j, 1] * eye[1]) + R[j, 2] * eye[2] for j in range(3)])
            out[s, l] = np.concatenate([R.reshape(9), t, [a, a, Ws / 2.0, Hs / 2.0]])
            enable[s, l] = 1
    out32 = out.astype(F32)
    enable[~np.isfinite(out32).all(2)] = 0
    items = [(MAX_LIGHTS * s + l, i, first)
             for s in range(S) for l in range(MAX_LIGHTS) if enable[s, l]
             for i in range(int(scene_first[s]), int(scene_first[s + 1]))
             for first in range(0, int(n_faces[int(instance_mesh[i])]), FACES_PER_ITEM)]
    return out32, enable, np.asarray(items, dtype=np.int32).reshape(-1, 3)


# ---- the light's projection, shared by 13.13 and 13.14 -----------------------------------------------------------------------
def project(view, point, P, z_near_l):
    """view f32 [16], P three f64 arrays -> (Qz, u, v, usable): Q = R P + t in the written order, the pinhole projection
    of a point light or the orthographic one of a directional light."""
    w = np.asarray(view, dtype=F32).astype(np.float64)
    with np.errstate(all="ignore"):
        qx = ((w[0] * P[0] + w[1] * P[1]) + w[2] * P[2]) + w[9]
        qy = ((w[3] * P[0] + w[4] * P[1]) + w[5] * P[2]) + w[10]
        qz = ((w[6] * P[0] + w[7] * P[1]) + w[8] * P[2]) + w[11]
        if point:
            u, v = (qx / qz) * w[12] + w[14], (qy / qz) * w[13] + w[15]
        else:
            u, v = qx * w[12] + w[14], qy * w[13] + w[15]
        ok = (qz > np.float64(F32(z_near_l))) & np.isfinite(qx) & np.isfinite(qy) & np.isfinite(qz) & np.isfinite(u) & np.isfinite(v)
    return qz, u, v, ok


# ---- SPEC 13.13 -----------------------------------------------------------------------------------------------------------------
def _edge(ax, ay, bx, by, px, py):
    """Edge function of a -> b at the samples (object arrays of Python integers) and the inside test with the ownership
    rule -> (E as object array, inside bool)."""
    dx, dy = bx - ax, by - ay
    E = dx * (py - ay) - dy * (px - ax)
    if dy > 0 or (dy == 0 and dx < 0):
        return E, (E >= 0).astype(bool)
    return E, (E > 0).astype(bool)


def shadow_maps(meshes, instance_mesh, transforms, scene_first, lights, light_views, items, size, z_near_l=Z_NEAR_L, boxes=None):
    """meshes: list of (V, F, C) by atlas index -> uint32 [S,4,Hs,Ws]. A row of `items` that leads outside an array is
    skipped, as is a face with an index outside [0, nv) or an unusable vertex. boxes: a list that receives, per triangle
    that covers a sample, (mesh, samples in its clipped box): a box of more than 64 goes to the whole wave (7.10)."""
    Hs, Ws = size
    S, I = len(scene_first) - 1, len(instance_mesh)
    lights = np.asarray(lights, dtype=F32).reshape(S, MAX_LIGHTS, 8)
    light_views = np.asarray(light_views, dtype=F32).reshape(S, MAX_LIGHTS, 16)
    depth = np.full((S * MAX_LIGHTS, Hs, Ws), np.inf, dtype=F32)
    for ls, i, first in np.asarray(items, dtype=np.int64).reshape(-1, 3):
        ls, i, first = int(ls), int(i), int(first)
        if not 0 <= ls < S * MAX_LIGHTS:
            continue
        s, l = divmod(ls, MAX_LIGHTS)
        if not (0 <= i < I and int(scene_first[s]) <= i < int(scene_first[s + 1])):
            continue
        m = int(instance_mesh[i])
        if not 0 <= m < len(meshes):
            continue
        V, F, _C = meshes[m]
        F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
        nv, nf = len(V), len(F)
        if not 0 <= first < nf:
            continue
        point = bool(lights[s, l, 3] != 0)
        C = rs.camera_points(V, transforms[i]).astype(np.float64)
        qz, u, v, ok = project(light_views[s, l], point, [C[:, 0], C[:, 1], C[:, 2]], z_near_l)
        with np.errstate(all="ignore"):
            ok &= (np.abs(u) < 2.0 ** 20) & (np.abs(v) < 2.0 ** 20)
            sx = np.rint(np.where(ok, u, 0.0) * 256.0).astype(np.int64)
            sy = np.rint(np.where(ok, v, 0.0) * 256.0).astype(np.int64)
            rz = np.where(ok, (1.0 / np.where(ok, qz, 1.0)) if point else qz, 0.0)
        for fc in range(first, min(first + FACES_PER_ITEM, nf)):
            i0, i1, i2 = (int(k) for k in F[fc])
            if not (0 <= i0 < nv and 0 <= i1 < nv and 0 <= i2 < nv) or not (ok[i0] and ok[i1] and ok[i2]):
                continue
            x0, y0, x1, y1, x2, y2 = (int(q) for q in (sx[i0], sy[i0], sx[i1], sy[i1], sx[i2], sy[i2]))
            A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
            if A == 0:
                continue
            if A < 0:
                i1, i2, A = i2, i1, -A
                x1, y1, x2, y2 = x2, y2, x1, y1
            # map pixel x is sampled at 256 x + 128
            xa, xb = max(0, -((-(min(x0, x1, x2) - 128)) // 256)), min(Ws - 1, (max(x0, x1, x2) - 128) // 256)
            ya, yb = max(0, -((-(min(y0, y1, y2) - 128)) // 256)), min(Hs - 1, (max(y0, y1, y2) - 128) // 256)
            if xa > xb or ya > yb:
                continue
            px = np.array([256 * x + 128 for x in range(xa, xb + 1)], dtype=object)[None, :]
            py = np.array([256 * y + 128 for y in range(ya, yb + 1)], dtype=object)[:, None]
            w0, in0 = _edge(x1, y1, x2, y2, px, py)
            w1, in1 = _edge(x2, y2, x0, y0, px, py)
            w2, in2 = _edge(x0, y0, x1, y1, px, py)
            inside = in0 & in1 & in2
            if not inside.any():
                continue
            if boxes is not None:
                boxes.append((m, (xb - xa + 1) * (yb - ya + 1)))
            w0, w1, w2 = (w.astype(np.float64) for w in (w0, w1, w2))
            acc = (w0 * rz[i0] + w1 * rz[i1]) + w2 * rz[i2]
            z = (float(A) / acc[inside] if point else acc[inside] / float(A)).astype(F32)
            win = depth[ls, ya:yb + 1, xa:xb + 1]
            win[inside] = np.minimum(win[inside], z)
    return np.ascontiguousarray(depth).view(np.uint32).reshape(S, MAX_LIGHTS, Hs, Ws)


# ---- SPEC 13.14 -----------------------------------------------------------------------------------------------------------------
def visibility(shadow_map, view, point, beta, size, P, ndl, z_near_l=Z_NEAR_L):
    """One enabled light at the surface points P (three f64 arrays) with N.L = ndl > 0 -> (vis f64, k int64)."""
    Hs, Ws = size
    qz, u, v, ok = project(view, point, P, z_near_l)
    w = np.asarray(view, dtype=F32).astype(np.float64)
    b0, b1 = (np.float64(F32(b)) for b in beta)
    with np.errstate(all="ignore"):
        texel = qz / w[12] if point else np.full(len(ndl), 1.0 / w[12])
        s2 = 1.0 - ndl * ndl
        tn = np.sqrt(np.where(s2 > 0.0, s2, 0.0)) / ndl
        bias = texel * (b0 + b1 * np.where(tn < 8.0, tn, 8.0))
        thr = qz - bias
        ix = np.clip(np.floor(np.where(ok, u, 0.0)), -2.0, Ws + 1.0).astype(np.int64)
        iy = np.clip(np.floor(np.where(ok, v, 0.0)), -2.0, Hs + 1.0).astype(np.int64)
        k = np.zeros(len(ndl), np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                x, y = ix + dx, iy + dy
                inside = (x >= 0) & (x < Ws) & (y >= 0) & (y < Hs)
                zb = shadow_map[np.clip(y, 0, Hs - 1), np.clip(x, 0, Ws - 1)]
                zf = zb.view(F32).astype(np.float64)
                k += inside & (zb != ZFAR) & (zf < thr)
    k = np.where(ok, k, 0)
    return (9 - k).astype(np.float64) / 9.0, k


def light(meshes, normals, instance_mesh, transforms, scene_first, cams, hw, albedo, instance, face, lights, n_lights,
          ambient, material, shadow_map, light_views, enable, size, params, pixel_offset=0.0, z_near=0.05, z_near_l=Z_NEAR_L):
    """ref_scene_light.light's steps 1-8 with 13.14's visibility on each light's two terms. shadow_map uint32
    [S,4,Hs,Ws], light_views f32 [S,4,16], enable [S,4], params f32 [S,2] -> dict: lit, normal, blocked u8 [S,H,W],
    shaded bool."""
    H, W = hw
    S, I = len(cams), len(instance_mesh)
    albedo, instance, face = np.asarray(albedo), np.asarray(instance), np.asarray(face)
    lights = np.asarray(lights, dtype=F32).reshape(S, MAX_LIGHTS, 8)
    ambient, material = np.asarray(ambient, dtype=F32).reshape(S, 3), np.asarray(material, dtype=F32).reshape(-1, 2)
    shadow_map = np.asarray(shadow_map).view(np.uint32).reshape(S, MAX_LIGHTS, size[0], size[1])
    light_views = np.asarray(light_views, dtype=F32).reshape(S, MAX_LIGHTS, 16)
    enable, params = np.asarray(enable).reshape(S, MAX_LIGHTS), np.asarray(params, dtype=F32).reshape(S, 2)
    lit = albedo.copy()
    normal = np.zeros((S, H, W, 3), F32)
    blocked = np.zeros((S, H, W), np.uint8)
    shaded = np.zeros((S, H, W), bool)
    o = int(np.rint(256.0 * float(F32(pixel_offset))))
    dot = rl._dot
    for s in range(S):
        K = rs.rc.cam_matrix(*[float(F32(v)) for v in cams[s]])
        for i in range(max(int(scene_first[s]), 0), min(int(scene_first[s + 1]), I)):
            m = int(instance_mesh[i])
            if not 0 <= m < len(meshes):
                continue
            V, F, _C = meshes[m]
            F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
            nv, nf = len(V), len(F)
            sel = (instance[s] == i) & (face[s] >= 0) & (face[s] < nf)
            if not sel.any():
                continue
            ys, xs = np.nonzero(sel)
            fi = F[face[s][sel]]
            good = ((fi >= 0) & (fi < nv)).all(1)
            ys, xs, fi = ys[good], xs[good], fi[good]
            sx, sy, rz, ok = rr.vertex_stage(V, transforms[i], K, z_near)
            i0, i1, i2 = fi[:, 0], fi[:, 1], fi[:, 2]
            A = (sx[i1] - sx[i0]) * (sy[i2] - sy[i0]) - (sy[i1] - sy[i0]) * (sx[i2] - sx[i0])
            good = ok[i0] & ok[i1] & ok[i2] & (A != 0)
            ys, xs, i0, i1, i2, A = ys[good], xs[good], i0[good], i1[good], i2[good], A[good]
            if len(ys) == 0:
                continue
            j0, j1, j2 = i0, np.where(A < 0, i2, i1), np.where(A < 0, i1, i2)
            px, py = 256 * xs.astype(np.int64) + o, 256 * ys.astype(np.int64) + o

            def edge(a, b):
                return (sx[b] - sx[a]) * (py - sy[a]) - (sy[b] - sy[a]) * (px - sx[a])
            w0, w1, w2 = edge(j1, j2), edge(j2, j0), edge(j0, j1)
            with np.errstate(all="ignore"):
                b0, b1, b2 = w0.astype(np.float64) * rz[j0], w1.astype(np.float64) * rz[j1], w2.astype(np.float64) * rz[j2]
                den = (b0 + b1) + b2
                Cp = rs.camera_points(V, transforms[i]).astype(np.float64)
                P = [((b0 * Cp[j0, c] + b1 * Cp[j1, c]) + b2 * Cp[j2, c]) / den for c in range(3)]
                T = np.asarray(transforms[i], dtype=np.float64).astype(F32)
                n32 = np.asarray(normals[m], dtype=F32).reshape(nv, 3)
                nr = np.stack([(T[r, 0] * n32[:, 0] + T[r, 1] * n32[:, 1]) + T[r, 2] * n32[:, 2] for r in range(3)], 1)
                nr = nr.astype(np.float64)
                N = [(b0 * nr[j0, c] + b1 * nr[j1, c]) + b2 * nr[j2, c] for c in range(3)]
                NN = dot(N[0], N[1], N[2], N[0], N[1], N[2])
                fb = ~(NN > 0.0) | ~np.isfinite(NN)
                a, b = Cp[i1] - Cp[i0], Cp[i2] - Cp[i0]
                fn = [a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]]
                N = [np.where(fb, fn[c], N[c]) for c in range(3)]
                NN = np.where(fb, dot(fn[0], fn[1], fn[2], fn[0], fn[1], fn[2]), NN)
                ln = np.sqrt(NN)
                Nh = [np.where(NN > 0.0, N[c] / ln, 0.0) for c in range(3)]
                pl = np.sqrt(dot(P[0], P[1], P[2], P[0], P[1], P[2]))
                Vh = [-P[c] / pl for c in range(3)]
                flip = dot(Nh[0], Nh[1], Nh[2], Vh[0], Vh[1], Vh[2]) < 0.0
                Nh = [np.where(flip, -Nh[c], Nh[c]) for c in range(3)]
                E = [np.full(len(ys), np.float64(ambient[s, c])) for c in range(3)]
                Sp = [np.zeros(len(ys)) for _ in range(3)]
                ktot = np.zeros(len(ys), np.int64)
                e = rl.exponent(material[i, 1])
                for l in range(min(max(int(n_lights[s]), 0), MAX_LIGHTS)):
                    row = lights[s, l]
                    D = [np.full(len(ys), np.float64(row[c])) for c in range(3)]
                    if row[3] != 0:
                        D = [D[c] - P[c] for c in range(3)]
                    dd = dot(D[0], D[1], D[2], D[0], D[1], D[2])
                    on = (dd > 0.0) & np.isfinite(dd)
                    dl = np.sqrt(dd)
                    Lh = [D[c] / dl for c in range(3)]
                    ndl = dot(Nh[0], Nh[1], Nh[2], Lh[0], Lh[1], Lh[2])
                    on &= ndl > 0.0
                    vis = np.ones(len(ys))
                    if enable[s, l] != 0:
                        vis, k = visibility(shadow_map[s, l], light_views[s, l], bool(row[3] != 0), params[s], size, P,
                                            np.where(on, ndl, 1.0), z_near_l)
                        vis, k = np.where(on, vis, 1.0), np.where(on, k, 0)
                        ktot += k
                    Ic = [np.float64(row[4 + c]) for c in range(3)]
                    E = [np.where(on, E[c] + Ic[c] * (ndl * vis), E[c]) for c in range(3)]
                    Hh = [Lh[c] + Vh[c] for c in range(3)]
                    hh = dot(Hh[0], Hh[1], Hh[2], Hh[0], Hh[1], Hh[2])
                    on &= hh > 0.0
                    hl = np.sqrt(hh)
                    ndh = dot(Nh[0], Nh[1], Nh[2], Hh[0] / hl, Hh[1] / hl, Hh[2] / hl)
                    on &= ndh > 0.0
                    p = ndh
                    for _ in range(e):
                        p = p * p
                    Sp = [np.where(on, Sp[c] + Ic[c] * (p * vis), Sp[c]) for c in range(3)]
                ks = np.float64(material[i, 0])
                for c in range(3):
                    v = albedo[s, ys, xs, c].astype(np.float64) * E[c] + 255.0 * (ks * Sp[c])
                    r = np.rint(v)
                    lit[s, ys, xs, c] = np.where(r >= 255.0, 255.0, np.where(r > 0.0, r, 0.0)).astype(np.uint8)
                    normal[s, ys, xs, c] = Nh[c].astype(F32)
            blocked[s, ys, xs] = ktot.astype(np.uint8)
            shaded[s, ys, xs] = True
    return {"lit": lit, "normal": normal, "blocked": blocked, "shaded": shaded}
