"""An object's symmetry transformations from its own surface (csrc/symmetry.hip, SPEC.md section 17): what BOP's
models_info.json lists under `symmetries_discrete` / `symmetries_continuous` and what bop_eval.symmetry_transformations,
scoring.select_instances and OnlineStream(symmetries=...) consume. The definition is this build's own: BOP published its
lists without the procedure that made them, so parity with those lists is unpinned.

Candidate rotations about the surface sample's centroid (one axis per +- pair of the icosphere directions MeshAtlas.resting
uses, angles 2 pi / k) are scored on the GPU -- every query point is transformed and looked up among the targets -- and the
selection among the scored candidates is host numpy, stated step by step in SPEC 17.5. score_transforms is bit-equal to
the numpy restatement tests/ref_symmetry.py, which find_symmetries(score=...) can run in its place."""
from math import gcd

import numpy as np
import torch

from . import _lib
from . import render as _render

N_QUERIES, OVERSAMPLE = 2048, 16                 # a Mesh's queries, and targets per query: 32768 targets (17.1)
FAN_RINGS, FAN_AZIMUTHS = (0.5, 0.25), 6         # 17.5 step 3: rings at these fractions of the grid spacing
FURTHER_ANGLES = (1.0, 2.0, 3.0)                 # 17.5 step 4, radians; and 2 pi / (max_order + 1), 2 pi / (max_order + 3)
MAX_CONTINUOUS = 3                               # 17.5 step 7


# ---- candidates (17.4) ------------------------------------------------------------------------------------------------------
def grid_spacing(level):
    """The nominal angle between neighbouring icosphere directions: the icosahedron's edge, atan(2), halved per level."""
    return float(np.arctan(2.0)) / float(2 ** int(level))


def candidate_axes(level=4):
    """One of each +- pair of render._icosphere_vertices(level), in their order -> f64 [(10 * 4^level + 2) / 2, 3]: the
    direction whose last component of magnitude above 1e-9 (z, then y, then x) is positive."""
    level = int(level)
    if not 0 <= level <= 5:
        raise ValueError("candidate_axes: level must lie in [0, 5], got %r" % (level,))
    d = _render._icosphere_vertices(level)
    big = np.abs(d) > 1e-9
    lead = np.where(big[:, 2], d[:, 2], np.where(big[:, 1], d[:, 1], d[:, 0]))
    return np.ascontiguousarray(d[lead > 0.0])


def rotation_about(axis, angle, centre):
    """The rotation by `angle` about the line through `centre` along `axis` -> f64 [4,4]: Rodrigues' formula as 8.6 writes
    it, R = I + sin K + (1 - cos) K K, t = centre - R centre."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt(a @ a)
    c = np.asarray(centre, dtype=np.float64)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    T[:3, 3] = c - T[:3, :3] @ c
    return T


def _orders(max_order):
    if int(max_order) != max_order or not 2 <= int(max_order) <= 64:
        raise ValueError("max_order must be an integer in [2, 64], got %r" % (max_order,))
    return list(range(2, int(max_order) + 1))


def candidate_rotations(centre, level=4, max_order=8):
    """The candidates of 17.4 -> f64 [A * (max_order - 1), 4, 4], A = (10 * 4^level + 2) / 2 axes (candidate_axes), axis
    major, the orders k = 2 .. max_order minor: the proper rotation by 2 pi / k about the axis through `centre`."""
    orders = _orders(max_order)
    return np.stack([rotation_about(a, 2.0 * np.pi / k, centre) for a in candidate_axes(level) for k in orders])


# ---- the scorer (17.2-17.3) ---------------------------------------------------------------------------------------------------
def _points(x, what, cap, finite):
    if torch.is_tensor(x):
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError("%s must be [n,3], got %s" % (what, tuple(x.shape)))
        t = x
    else:
        a = np.asarray(x)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("%s must be [n,3], got %s" % (what, a.shape))
        a = np.ascontiguousarray(a, dtype=np.float64).astype(np.float32)
        if finite and not np.isfinite(a).all():
            raise ValueError("%s must be finite" % what)
        t = torch.from_numpy(a)
    if not 1 <= int(t.shape[0]) <= cap:
        raise ValueError("%s: 1 to %d points, got %d" % (what, cap, int(t.shape[0])))
    return t


def _check_tol(tol):
    t = np.float32(tol)
    with np.errstate(all="ignore"):
        sq = t * t
    if not (np.isfinite(t) and t > 0 and np.isfinite(sq) and sq > 0):
        raise ValueError("tol and its f32 square must be finite and positive, got %r" % (tol,))
    return float(t)


def score_transforms(targets, queries, transforms, tol):
    """SPEC 17.2-17.3: targets [Nt,3] (finite, Nt <= 32768), queries [Mq,3] (Mq <= 4096), numpy or tensors, cast to f32;
    transforms f64 [C,4,4] (any C >= 1; calls of at most SYM_MAX_TRANSFORMS), tol a length ->
    (miss int32 [C], worst_d2 f32 [C], sum_q int64 [C]) on the device: per transform the queries without a target at
    d2 <= tol^2, the largest accepted d2, and the sum of trunc(d2 / tol^2 * 2^32) over the accepted queries. One grid
    build, one launch per SYM_MAX_TRANSFORMS transforms, nothing read back; ValueError before the device is touched."""
    Tg = _points(targets, "targets", _lib.SYM_MAX_TARGETS, True)
    Q = _points(queries, "queries", _lib.SYM_MAX_QUERIES, False)
    if torch.is_tensor(transforms):
        T = transforms
    else:
        T = torch.from_numpy(np.ascontiguousarray(np.asarray(transforms, dtype=np.float64)))
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4) or T.shape[0] < 1:
        raise ValueError("transforms must be [C,4,4] with C >= 1, got %s" % (tuple(T.shape),))
    tol = _check_tol(tol)
    dev = next((t.device for t in (Tg, Q, T) if t.is_cuda), None) or _lib._dev()
    Tg, Q = (t.to(dev, torch.float32).contiguous() for t in (Tg, Q))
    T = T.to(dev, torch.float64).contiguous()
    Nt, Mq, C = int(Tg.shape[0]), int(Q.shape[0]), int(T.shape[0])
    need = int(_lib.fn("ossid_sym_grid_nbytes")(Nt))
    grid = torch.empty(need, dtype=torch.uint8, device=dev)
    miss = torch.empty(C, dtype=torch.int32, device=dev)
    worst = torch.empty(C, dtype=torch.float32, device=dev)
    sum_q = torch.empty(C, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_sym_grid")(Tg.data_ptr(), Nt, tol, grid.data_ptr(), need, _lib.stream()), "ossid_sym_grid")
        for a in range(0, C, _lib.SYM_MAX_TRANSFORMS):
            n = min(C - a, _lib.SYM_MAX_TRANSFORMS)
            rc = _lib.fn("ossid_sym_score")(grid.data_ptr(), need, Nt, Q.data_ptr(), Mq, T[a:a + n].data_ptr(), n, tol,
                                            miss[a:a + n].data_ptr(), worst[a:a + n].data_ptr(), sum_q[a:a + n].data_ptr(),
                                            _lib.stream())
            _lib.check(rc, "ossid_sym_score")
    return miss, worst, sum_q


# ---- the selection (17.5) -----------------------------------------------------------------------------------------------------
def _host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _fan(axis, spacing):
    """17.5 step 3: the axis and FAN_AZIMUTHS directions on each ring at FAN_RINGS x spacing around it -> f64 [1 + 12, 3].
    The ring's frame: u = normalise(e x axis), e the coordinate axis of the smallest |component| (the first at ties),
    v = axis x u."""
    a = np.asarray(axis, dtype=np.float64)
    e = np.zeros(3)
    e[int(np.argmin(np.abs(a)))] = 1.0
    u = np.cross(e, a)
    u = u / np.sqrt(u @ u)
    v = np.cross(a, u)
    out = [a]
    for f in FAN_RINGS:
        rho = f * spacing
        for j in range(FAN_AZIMUTHS):
            al = 2.0 * np.pi * j / FAN_AZIMUTHS
            d = np.cos(rho) * a + np.sin(rho) * (np.cos(al) * u + np.sin(al) * v)
            out.append(d / np.sqrt(d @ d))
    return np.stack(out)


def _angle_between_axes(a, b):
    """The angle between two undirected lines, [0, pi / 2]."""
    return float(np.arccos(min(1.0, abs(float(np.dot(a, b))))))


def _sources(mesh_or_points, diameter):
    """-> (targets, queries, diameter)."""
    from . import model_cloud as _mc
    if isinstance(mesh_or_points, _render.Mesh):
        cloud, info = _mc.sample_model_cloud(mesh_or_points, n_points=N_QUERIES, oversample=OVERSAMPLE, return_info=True)
        d = _mc.mesh_diameter(mesh_or_points) if diameter is None else float(diameter)
        return info["candidates"]["points"], cloud.model_points, d
    if isinstance(mesh_or_points, (tuple, list)) and len(mesh_or_points) == 2:
        targets, queries = mesh_or_points
    else:
        targets = mesh_or_points
        n = int(targets.shape[0])
        m = min(n, N_QUERIES)
        idx = (np.arange(m) * n) // m                    # an evenly strided subset: no launch
        queries = targets[torch.from_numpy(idx).to(targets.device)] if torch.is_tensor(targets) else np.asarray(targets)[idx]
    d = _mc.mesh_diameter(targets) if diameter is None else float(diameter)
    return targets, queries, d


def find_symmetries(mesh_or_points, tol_rel=0.05, max_miss=0, level=4, max_order=8, score=None, diameter=None,
                    return_info=False):
    """SPEC section 17 -> {"symmetries_discrete": [16 row-major numbers per symmetry], "symmetries_continuous":
    [{"axis": [3], "offset": [3]}]}, models_info.json's form, in the unit of the input.

    mesh_or_points: a render.Mesh with vertex colours or a texture (targets = the 32768 candidates of its model cloud,
    queries = the cloud's 2048 points, SPEC 9.4-9.5; diameter = mesh_diameter), or points [N,3] (targets; queries = an
    evenly strided 2048 of them), or a (targets, queries) pair; `diameter` overrides model_cloud.mesh_diameter of the
    mesh or the targets. tol = tol_rel x diameter; a candidate is accepted iff at most max_miss queries find no target
    within tol. score: a callable with score_transforms' signature (the tests pass the numpy restatement).
    Limits (17.6): an order above max_order is missed; colour is not looked at; a rotation centre far from the sample's
    centroid is not found. With return_info also a dict: tol, centre, diameter, n_candidates, clusters."""
    score = score_transforms if score is None else score
    orders = _orders(max_order)
    if not (np.isfinite(tol_rel) and tol_rel > 0.0):
        raise ValueError("tol_rel must be finite and positive, got %r" % (tol_rel,))
    if int(max_miss) != max_miss or max_miss < 0:
        raise ValueError("max_miss must be an integer >= 0, got %r" % (max_miss,))
    axes = candidate_axes(level)
    targets, queries, diam = _sources(mesh_or_points, diameter)
    if not (np.isfinite(diam) and diam > 0.0):
        raise ValueError("find_symmetries: the diameter must be finite and positive, got %r" % (diam,))
    tol = float(tol_rel) * diam
    Th = _host(targets).astype(np.float32)
    if not np.isfinite(Th).all():
        raise ValueError("find_symmetries: the targets must be finite")
    centre = Th.astype(np.float64).mean(0)
    spacing = grid_spacing(level)
    n_scored = [0]

    def run(transforms):
        """-> (accepted bool [n], cost int64 [n]): cost = sum_q + miss * 2^32, a miss counting as a hit at d2 = tol^2"""
        T = np.ascontiguousarray(np.stack(transforms))
        n_scored[0] += len(T)
        miss, _worst, sum_q = (_host(x) for x in score(targets, queries, T, tol))
        return miss <= int(max_miss), sum_q.astype(np.int64) + miss.astype(np.int64) * (1 << 32)

    # 1. every candidate
    A, K = len(axes), len(orders)
    acc, sums = run([rotation_about(a, 2.0 * np.pi / k, centre) for a in axes for k in orders])
    acc, sums = acc.reshape(A, K), sums.reshape(A, K)
    # 2. per order, greedy non-minimum suppression among the accepted axes within phi_k
    survivors = []                                        # (axis, k, cost)
    for ki, k in enumerate(orders):
        phi = min(2.0 * float(tol_rel) / np.sin(np.pi / k) + spacing, 0.5 * np.pi)
        live = [int(i) for i in np.lexsort((np.arange(A), sums[:, ki])) if acc[i, ki]]
        while live:
            best = live[0]
            survivors.append((axes[best], k, int(sums[best, ki])))
            live = [i for i in live if _angle_between_axes(axes[i], axes[best]) > phi]
    # 3. one refinement: the fan around each survivor, its direction of lowest (cost, fan index); a survivor whose refined
    # direction is not accepted is dropped
    if survivors:
        fans = [_fan(a, spacing) for a, _k, _s in survivors]
        facc, fsum = run([rotation_about(d, 2.0 * np.pi / k, centre) for f, (_a, k, _s) in zip(fans, survivors) for d in f])
        per = 1 + len(FAN_RINGS) * FAN_AZIMUTHS
        refined = []
        for i, (_a, k, _s) in enumerate(survivors):
            sm = fsum[i * per:(i + 1) * per]
            j = int(np.lexsort((np.arange(per), sm))[0])
            if facc[i * per + j]:
                refined.append((fans[i][j], k, int(sm[j])))
        survivors = refined
    # clusters: survivors of different orders about one axis (within 2 x spacing of the cluster's first member), taken
    # from the highest order down, by cost inside an order
    clusters = []                                         # {"members": {k: (axis, cost)}, "axis": first member's}
    for a, k, s in sorted(survivors, key=lambda m: (-m[1], m[2])):
        for c in clusters:
            if _angle_between_axes(a, c["axis"]) <= 2.0 * spacing:
                if k not in c["members"]:
                    c["members"][k] = (a, s)
                break
        else:
            clusters.append({"axis": a, "members": {k: (a, s)}})
    # 4. an axis accepted at every order is continuous iff it also passes the further angles (about its order-2 member)
    further = list(FURTHER_ANGLES) + [2.0 * np.pi / (orders[-1] + 1), 2.0 * np.pi / (orders[-1] + 3)]
    full = [c for c in clusters if all(k in c["members"] for k in orders)]
    for c in clusters:
        c["continuous"] = False
    if full:
        cacc, _s = run([rotation_about(c["members"][2][0], th, centre) for c in full for th in further])
        for i, c in enumerate(full):
            c["continuous"] = bool(cacc[i * len(further):(i + 1) * len(further)].all())
    cont = [c for c in clusters if c["continuous"]]
    discrete, continuous = [], []
    if len(cont) >= 2:
        # 7. a sphere: at most three of its axes, the lowest order-2 cost first -- a subset of its symmetries
        cont = sorted(cont, key=lambda c: c["members"][2][1])[:MAX_CONTINUOUS]
        continuous = [c["members"][2][0] for c in cont]
        emit = []
    elif len(cont) == 1:
        # 5.-6. nothing discrete about the continuous axis; of the two-fold axes perpendicular to it the lowest cost
        continuous = [cont[0]["members"][2][0]]
        perp = [c for c in clusters if not c["continuous"] and 2 in c["members"] and
                abs(float(np.dot(c["members"][2][0], continuous[0]))) <= np.sin(2.0 * spacing)]
        emit = [(m[0], 1, 2) for m in sorted((c["members"][2] for c in perp), key=lambda m: m[1])[:1]]
    else:
        # 8. per cluster the powers j / k of its accepted orders, once per reduced fraction p / q, about the member of
        # order q (of the smallest accepted multiple of q when q itself has no member)
        emit = []
        for c in clusters:
            ks = sorted(c["members"])
            fracs = sorted({(j // gcd(j, k), k // gcd(j, k)) for k in ks for j in range(1, k)}, key=lambda f: (f[1], f[0]))
            for p, q in fracs:
                emit.append((c["members"][min(k for k in ks if k % q == 0)][0], p, q))
    # 9. the emitted list is scored once more: what is not accepted is not emitted
    if emit:
        Ts = [rotation_about(a, 2.0 * np.pi * p / q, centre) for a, p, q in emit]
        eacc, _s = run(Ts)
        discrete = [[float(v) for v in T.reshape(-1)] for T, ok in zip(Ts, eacc) if ok]
    out = {"symmetries_discrete": discrete,
           "symmetries_continuous": [{"axis": [float(v) for v in a], "offset": [float(v) for v in centre]} for a in continuous]}
    if not return_info:
        return out
    return out, {"tol": tol, "centre": centre, "diameter": diam, "n_candidates": A * K, "n_scored": n_scored[0],
                 "clusters": clusters}


def scaled(symmetries, factor):
    """The dict of find_symmetries in another unit: the translations of `symmetries_discrete` and the `offset`s of
    `symmetries_continuous` times `factor` (1000 takes metres to models_info.json's millimetres)."""
    f = float(factor)
    disc = []
    for m in symmetries.get("symmetries_discrete", ()):
        m = [float(v) for v in m]
        for i in (3, 7, 11):
            m[i] *= f
        disc.append(m)
    cont = [{"axis": [float(v) for v in s["axis"]], "offset": [float(v) * f for v in s["offset"]]}
            for s in symmetries.get("symmetries_continuous", ())]
    return {"symmetries_discrete": disc, "symmetries_continuous": cont}


def has_symmetry(symmetries):
    return bool(symmetries.get("symmetries_discrete")) or bool(symmetries.get("symmetries_continuous"))
