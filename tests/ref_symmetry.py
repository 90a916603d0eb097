"""SPEC.md section 17.3 restated in numpy with brute-force neighbours: what csrc/symmetry.hip's ossid_sym_score computes
through its cell grid, bit for bit. Also the analytic objects whose symmetry groups the tests derive by hand.

Plain helper module (no tests): test_symmetry.py passes score_transforms to find_symmetries(score=...),
test_symmetry_gpu.py compares the kernels with it."""
import numpy as np

Q_ONE = 4294967296.0            # 17.3: an accepted d2 is counted as trunc(d2 / worst * 2^32)


def transform_f32(T, Q):
    """17.3 steps 1-3: f32 points [Mq,3] under f64 transforms [C,4,4] -> f32 [C,Mq,3]; per row
    ((r0 x + r1 y) + r2 z) + t in f64, each operation rounded once, then one rounding to f32."""
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    x, y, z = (np.asarray(Q, dtype=np.float32).astype(np.float64)[:, a][None] for a in range(3))
    with np.errstate(all="ignore"):
        rows = [((T[:, i, 0, None] * x + T[:, i, 1, None] * y) + T[:, i, 2, None] * z) + T[:, i, 3, None] for i in range(3)]
        return np.stack(rows, axis=-1).astype(np.float32)


def nearest(points, targets, worst):
    """17.3 step 4 by brute force: f32 points [...,3] against f32 targets [Nt,3] -> (d2 f32, index int64) of the
    lexicographic minimum of (d2, index) among the targets with d2 <= worst; (worst, -1) where there is none.
    d2 = (dx dx + dy dy) + dz dz in f32, dx = point - target."""
    P, Tg = np.asarray(points, dtype=np.float32), np.asarray(targets, dtype=np.float32)
    with np.errstate(all="ignore"):
        dx, dy, dz = (P[..., None, a] - Tg[:, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        ok = d2 <= np.float32(worst)                      # NaN never counts
    key = np.where(ok, d2, np.float32(np.inf))
    idx = key.argmin(-1)                                  # the first of equal minima: the lowest index
    hit = ok.any(-1)
    best = np.take_along_axis(d2, idx[..., None], -1)[..., 0]
    return np.where(hit, best, np.float32(worst)).astype(np.float32), np.where(hit, idx, -1)


def score_transforms(targets, queries, transforms, tol, max_elems=1 << 23):
    """ossid_sym_score: -> (miss int32 [C], worst_d2 f32 [C], sum_q int64 [C])."""
    Tg, Q = np.asarray(targets, dtype=np.float32).reshape(-1, 3), np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    T = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4)
    worst = np.float32(tol) * np.float32(tol)
    C = len(T)
    miss, worst_d2, sum_q = np.zeros(C, np.int32), np.zeros(C, np.float32), np.zeros(C, np.int64)
    step = max(1, int(max_elems // (len(Tg) * len(Q))))
    for a in range(0, C, step):
        P = transform_f32(T[a:a + step], Q)
        with np.errstate(all="ignore"):                   # `nearest` without the index, which no output carries
            dx, dy, dz = (P[..., None, k] - Tg[:, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            d2 = np.where(d2 <= worst, d2, np.float32(np.inf)).min(-1)
            hit = np.isfinite(d2)                         # worst is finite: an accepted d2 is
            q = np.where(hit, np.floor(d2.astype(np.float64) / np.float64(worst) * Q_ONE), 0.0)
        miss[a:a + step] = (~hit).sum(1)
        worst_d2[a:a + step] = np.where(hit, d2, np.float32(0.0)).max(1)
        sum_q[a:a + step] = q.astype(np.int64).sum(1)
    return miss, worst_d2, sum_q


# ---- analytic objects: even deterministic surface samples (no random numbers) ---------------------------------------------
def _rect(o, u, v, nu, nv):
    """nu x nv cell-centred samples of the parallelogram o + s u + t v, s t in (0, 1)."""
    s, t = (np.arange(nu) + 0.5) / nu, (np.arange(nv) + 0.5) / nv
    return (np.asarray(o, float) + s[:, None, None] * np.asarray(u, float) + t[None, :, None] * np.asarray(v, float)).reshape(-1, 3)


def box_points(a, b, c, spacing):
    """The surface of the box [-a/2, a/2] x [-b/2, b/2] x [-c/2, c/2], samples about `spacing` apart."""
    n = lambda e: max(1, int(round(e / spacing)))
    out = []
    for s in (-0.5, 0.5):
        out.append(_rect((-a / 2, -b / 2, s * c), (a, 0, 0), (0, b, 0), n(a), n(b)))
        out.append(_rect((-a / 2, s * b, -c / 2), (a, 0, 0), (0, 0, c), n(a), n(c)))
        out.append(_rect((s * a, -b / 2, -c / 2), (0, b, 0), (0, 0, c), n(b), n(c)))
    return np.concatenate(out)


def prism_points(n_sides, radius, height, spacing):
    """A right prism over the regular n-gon of circumradius `radius` in the xy plane, axis z, centred at the origin: the
    side rectangles and the two caps (each cap as n triangles from the axis, sampled on a barycentric lattice)."""
    ang = 2.0 * np.pi * np.arange(n_sides + 1) / n_sides
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], 1)
    out = []
    for i in range(n_sides):
        p, q = ring[i], ring[i + 1]
        edge = float(np.linalg.norm(q - p))
        out.append(_rect((p[0], p[1], -height / 2), (q[0] - p[0], q[1] - p[1], 0), (0, 0, height),
                         max(1, int(round(edge / spacing))), max(1, int(round(height / spacing)))))
        m = max(1, int(round(radius / spacing)))
        for z in (-height / 2, height / 2):
            for i1 in range(m):
                for i2 in range(m - i1):
                    for w1, w2 in (((i1 + 1 / 3) / m, (i2 + 1 / 3) / m), ((i1 + 2 / 3) / m, (i2 + 2 / 3) / m)):
                        if w1 + w2 < 1.0:
                            out.append(np.array([[w1 * p[0] + w2 * q[0], w1 * p[1] + w2 * q[1], z]]))
    return np.concatenate(out)


def lathe_points(profile, spacing):
    """The surface of revolution about z of the polyline profile [(r, z), ...]: rings about `spacing` apart along the
    profile, each ring with samples about `spacing` apart and a phase that differs from ring to ring."""
    prof = np.asarray(profile, dtype=np.float64)
    out, k = [], 0
    for (r0, z0), (r1, z1) in zip(prof[:-1], prof[1:]):
        n = max(1, int(round(np.hypot(r1 - r0, z1 - z0) / spacing)))
        for i in range(n):
            f = (i + 0.5) / n
            r, z = r0 + f * (r1 - r0), z0 + f * (z1 - z0)
            m = max(1, int(round(2.0 * np.pi * r / spacing)))
            th = 2.0 * np.pi * (np.arange(m) + 0.618033988749895 * k) / m
            out.append(np.stack([r * np.cos(th), r * np.sin(th), np.full(m, z)], 1))
            k += 1
    return np.concatenate(out)


LATHE_PROFILE = [(0.0, -0.5), (0.5, -0.5), (0.5, -0.1), (0.2, 0.1), (0.2, 0.5), (0.0, 0.5)]      # a bottle: no up-down mirror
CYLINDER_PROFILE = [(0.0, -0.5), (0.4, -0.5), (0.4, 0.5), (0.0, 0.5)]


def thin(points, n):
    """n of the points, evenly strided: the queries of a point-set input."""
    P = np.asarray(points)
    return P[(np.arange(n) * len(P)) // n]


def diameter(points):
    """The largest distance between two points, f64 (brute force by chunks)."""
    P = np.asarray(points, dtype=np.float64)
    best = 0.0
    for a in range(0, len(P), 512):
        d = P[a:a + 512, None, :] - P[None]
        best = max(best, float((d * d).sum(-1).max()))
    return float(np.sqrt(best))
