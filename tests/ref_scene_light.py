"""Independent numpy restatement of SPEC.md 13.10 (smooth vertex normals by fixed-point sums) and 13.11 (the deferred
shading pass), the yardstick of csrc/scene_light.hip, built on ref_raster's vertex stage and ref_scene's camera points.

The normals' sums are Python integers (exact, any order); every float64 expression is written in the SPEC's
parenthesisation and numpy rounds each operation once; roundings to integers are np.rint (half to even). The pass is
evaluated per instance over that instance's pixels at once: every step is elementwise, so the vectorisation changes no
bit.

Also the light table of the issue for ref_scene.fixture() (fixture_lights()).
"""
import functools
from fractions import Fraction

import numpy as np

import ref_raster as rr
import ref_scene as rs

F32 = np.float32
MAX_LIGHTS = 4


# ---- SPEC 13.10 -----------------------------------------------------------------------------------------------------------------
def shift_for(vertices):
    """The host's rule: e = the largest f64 extent of the bounding box of the finite f32 vertices, x = 2.0 * e * e in f64;
    the largest integer s with x * 2^s <= 2^40, by exact rationals; 0 when e = 0 or nothing is finite."""
    V = np.asarray(vertices, dtype=np.float64).astype(F32).astype(np.float64).reshape(-1, 3)
    V = V[np.isfinite(V).all(1)]
    if len(V) == 0:
        return 0
    e = float((V.max(0) - V.min(0)).max())
    if e == 0.0:
        return 0
    x, lim, s = Fraction(2.0 * e * e), Fraction(2) ** 40, 0
    while x * Fraction(2) ** (s + 1) <= lim:
        s += 1
    while x * Fraction(2) ** s > lim:
        s -= 1
    return s


def vertex_normals(vertices, faces, shift, want_sums=False):
    """-> f32 [V,3] (and, with want_sums, the integer sums as a list of V lists of 3 Python ints)."""
    P = np.asarray(vertices, dtype=np.float64).astype(F32).astype(np.float64).reshape(-1, 3)
    nv = len(P)
    acc = [[0, 0, 0] for _ in range(nv)]
    for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3):
        i0, i1, i2 = (int(i) for i in f)
        if not (0 <= i0 < nv and 0 <= i1 < nv and 0 <= i2 < nv):
            continue
        with np.errstate(all="ignore"):
            a, b = P[i1] - P[i0], P[i2] - P[i0]
            n = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        if not np.isfinite(n).all():
            continue
        q = [int(np.rint(np.ldexp(n[c], int(shift)))) for c in range(3)]
        for i in (i0, i1, i2):
            for c in range(3):
                acc[i][c] += q[c]
    out = np.zeros((nv, 3), F32)
    for v in range(nv):
        sx, sy, sz = (np.float64(float(a)) for a in acc[v])          # int -> f64 rounds half to even, as the device's cast
        nn = (sx * sx + sy * sy) + sz * sz
        if nn > 0.0:
            ln = np.sqrt(nn)
            out[v] = (F32(sx / ln), F32(sy / ln), F32(sz / ln))
    return (out, acc) if want_sums else out


def mesh_normals(meshes):
    """The atlas's normals, mesh by mesh, each at its own shift."""
    return [vertex_normals(V, F, shift_for(V)) for V, F, _C in meshes]


# ---- SPEC 13.11 -----------------------------------------------------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def exponent(ef):
    ef = F32(ef)
    return 0 if not ef > 0 else (10 if ef >= 10 else int(ef))


def light(meshes, normals, instance_mesh, transforms, scene_first, cams, hw, albedo, instance, face, lights, n_lights,
          ambient, material, pixel_offset=0.0, z_near=0.05):
    """meshes: list of (V, F, C) by atlas index; normals: list of f32 [nv,3] beside them; albedo u8 [S,H,W,3], instance and
    face int32 [S,H,W]; lights f32 [S,4,8], n_lights [S], ambient f32 [S,3], material f32 [I,2]
    -> dict: lit u8 [S,H,W,3], normal f32 [S,H,W,3], shaded bool [S,H,W] (the pixels that passed every check), fallback
    bool [S,H,W] (those that took the face's normal)."""
    H, W = hw
    S, I = len(cams), len(instance_mesh)
    albedo, instance, face = np.asarray(albedo), np.asarray(instance), np.asarray(face)
    lights = np.asarray(lights, dtype=F32).reshape(S, MAX_LIGHTS, 8)
    ambient, material = np.asarray(ambient, dtype=F32).reshape(S, 3), np.asarray(material, dtype=F32).reshape(-1, 2)
    lit = albedo.copy()
    normal = np.zeros((S, H, W, 3), F32)
    shaded, fallback = np.zeros((S, H, W), bool), np.zeros((S, H, W), bool)
    o = int(np.rint(256.0 * float(F32(pixel_offset))))
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
            # 1. the winner's setup with the A < 0 swap, its weights and their sum
            j0, j1, j2 = i0, np.where(A < 0, i2, i1), np.where(A < 0, i1, i2)
            px, py = 256 * xs.astype(np.int64) + o, 256 * ys.astype(np.int64) + o

            def edge(a, b):
                return (sx[b] - sx[a]) * (py - sy[a]) - (sy[b] - sy[a]) * (px - sx[a])
            w0, w1, w2 = edge(j1, j2), edge(j2, j0), edge(j0, j1)
            with np.errstate(all="ignore"):
                b0, b1, b2 = w0.astype(np.float64) * rz[j0], w1.astype(np.float64) * rz[j1], w2.astype(np.float64) * rz[j2]
                den = (b0 + b1) + b2
                # 2. the surface point from the f32 camera points
                C32 = rs.camera_points(V, transforms[i])
                Cp = C32.astype(np.float64)
                P = [((b0 * Cp[j0, c] + b1 * Cp[j1, c]) + b2 * Cp[j2, c]) / den for c in range(3)]
                # 3. the f32-rotated vertex normals, interpolated without the division
                T = np.asarray(transforms[i], dtype=np.float64).astype(F32)
                n32 = np.asarray(normals[m], dtype=F32).reshape(nv, 3)
                nr = np.stack([(T[r, 0] * n32[:, 0] + T[r, 1] * n32[:, 1]) + T[r, 2] * n32[:, 2] for r in range(3)], 1)
                assert nr.dtype == F32
                nr = nr.astype(np.float64)
                N = [(b0 * nr[j0, c] + b1 * nr[j1, c]) + b2 * nr[j2, c] for c in range(3)]
                # 4. the face's normal where that has no finite positive length
                NN = _dot(N[0], N[1], N[2], N[0], N[1], N[2])
                fb = ~(NN > 0.0) | ~np.isfinite(NN)
                a, b = Cp[i1] - Cp[i0], Cp[i2] - Cp[i0]
                fn = [a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]]
                N = [np.where(fb, fn[c], N[c]) for c in range(3)]
                NN = np.where(fb, _dot(fn[0], fn[1], fn[2], fn[0], fn[1], fn[2]), NN)
                ln = np.sqrt(NN)
                Nh = [np.where(NN > 0.0, N[c] / ln, 0.0) for c in range(3)]
                # 5. the view direction; two-sided
                pl = np.sqrt(_dot(P[0], P[1], P[2], P[0], P[1], P[2]))
                Vh = [-P[c] / pl for c in range(3)]
                flip = _dot(Nh[0], Nh[1], Nh[2], Vh[0], Vh[1], Vh[2]) < 0.0
                Nh = [np.where(flip, -Nh[c], Nh[c]) for c in range(3)]
                # 6. the lights, in order
                E = [np.full(len(ys), np.float64(ambient[s, c])) for c in range(3)]
                Sp = [np.zeros(len(ys)) for _ in range(3)]
                e = exponent(material[i, 1])
                for l in range(min(max(int(n_lights[s]), 0), MAX_LIGHTS)):
                    row = lights[s, l]
                    D = [np.full(len(ys), np.float64(row[c])) for c in range(3)]
                    if row[3] != 0:
                        D = [D[c] - P[c] for c in range(3)]
                    dd = _dot(D[0], D[1], D[2], D[0], D[1], D[2])
                    on = (dd > 0.0) & np.isfinite(dd)
                    dl = np.sqrt(dd)
                    Lh = [D[c] / dl for c in range(3)]
                    ndl = _dot(Nh[0], Nh[1], Nh[2], Lh[0], Lh[1], Lh[2])
                    on &= ndl > 0.0
                    Ic = [np.float64(row[4 + c]) for c in range(3)]
                    E = [np.where(on, E[c] + Ic[c] * ndl, E[c]) for c in range(3)]
                    Hh = [Lh[c] + Vh[c] for c in range(3)]
                    hh = _dot(Hh[0], Hh[1], Hh[2], Hh[0], Hh[1], Hh[2])
                    on &= hh > 0.0
                    hl = np.sqrt(hh)
                    ndh = _dot(Nh[0], Nh[1], Nh[2], Hh[0] / hl, Hh[1] / hl, Hh[2] / hl)
                    on &= ndh > 0.0
                    p = ndh
                    for _ in range(e):
                        p = p * p
                    Sp = [np.where(on, Sp[c] + Ic[c] * p, Sp[c]) for c in range(3)]
                # 7., 8.
                ks = np.float64(material[i, 0])
                for c in range(3):
                    v = albedo[s, ys, xs, c].astype(np.float64) * E[c] + 255.0 * (ks * Sp[c])
                    r = np.rint(v)
                    lit[s, ys, xs, c] = np.where(r >= 255.0, 255.0, np.where(r > 0.0, r, 0.0)).astype(np.uint8)
                    normal[s, ys, xs, c] = Nh[c].astype(F32)
            shaded[s, ys, xs] = True
            fallback[s, ys, xs] = fb
    return {"lit": lit, "normal": normal, "shaded": shaded, "fallback": fallback}


# ---- the fixture's lights -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_lights():
    """The hand-written table for ref_scene.fixture(): scene 0 has four lights, directional and point mixed, with e = 0 on
    instance 1 and e = 10 on instance 3; scene 1 is the empty scene; scene 2 has n_lights = 0 and a tinted ambient.
    -> (lights f32 [3,4,8], n_lights int32 [3], ambient f32 [3,3], material f32 [9,2]); callers must not write into them."""
    lights = np.zeros((3, MAX_LIGHTS, 8), F32)
    lights[0, 0] = (-0.3, -0.5, -1.0, 0, 0.45, 0.40, 0.35, 0)          # directional, from above left of the camera
    lights[0, 1] = (0.4, -0.2, 0.1, 1, 0.30, 0.32, 0.36, 0)            # a point light right of the camera
    lights[0, 2] = (0.0, 0.6, 0.7, 1, 0.20, 0.15, 0.10, 0)             # a point light below, inside the scene's depth range
    lights[0, 3] = (1.0, 0.0, -0.2, 0, 0.10, 0.12, 0.14, 7)            # directional, grazing from the right
    lights[1, 0] = (0.0, 0.0, -1.0, 0, 0.5, 0.5, 0.5, 0)               # lights nothing: the scene is empty
    lights[2, 0] = (0.0, 0.0, -1.0, 0, 9.0, 9.0, 9.0, 0)               # beyond n_lights = 0: not read
    n_lights = np.array([4, 1, 0], np.int32)
    ambient = np.array([[0.30, 0.32, 0.35], [0.5, 0.5, 0.5], [0.8, 0.9, 1.1]], F32)
    material = np.array([[0.0, 4], [0.25, 0], [0.25, 0], [0.3, 10], [0.2, 5], [0.1, 3], [0.3, 6], [0.15, 5.7], [0.3, 12]], F32)
    return lights, n_lights, ambient, material


def fixture_meshes():
    """The fixture's meshes in atlas order (obj_id 1, 2, 3) and the instances' atlas indices."""
    fx = rs.fixture()
    order = sorted(fx["meshes"])
    return [fx["meshes"][o] for o in order], np.array([order.index(o) for o in fx["instance_obj"]], np.int32)


@functools.lru_cache(maxsize=None)
def fixture_normals():
    return mesh_normals(fixture_meshes()[0])


@functools.lru_cache(maxsize=None)
def reference():
    """The pass over ref_scene.reference() under fixture_lights(), computed once; callers must not write into it."""
    fx, ref = rs.fixture(), rs.reference()
    meshes, imesh = fixture_meshes()
    lights, n_lights, ambient, material = fixture_lights()
    return light(meshes, fixture_normals(), imesh, fx["transforms"], fx["scene_first"], fx["cams"], rs.HW, ref["color"],
                 ref["instance"], ref["face"], lights, n_lights, ambient, material, 0.0, rs.NEAR)
