"""Independent numpy restatement of SPEC.md section 6 (point-pair-feature pose hypotheses), the yardstick of csrc/ppf.hip.

float32 wherever SPEC 6 says f32 (sampling, features, bins), float64 with the stated sequential order where it says f64
(scene covariances, poses, clustering). The test object and scene are those of tests/ref_icp.py (ellipsoid with a bump
rendered into synth.make_frame's background).
"""
import math

import numpy as np

import ref_icp as ri

F32 = np.float32
NA, NALPHA, CHUNK = 15, 30, 1024
NORMAL_RADIUS_REL = 2.0                 # SPEC 6.3 default
CLUSTER_COS = math.cos(math.pi / 15.0)        # cos 12 degrees, libm as the host side computes it


# ---- 6.1 / 6.2: validity, diameter, sampling ------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def prepare_model(points, normals):
    """-> (P f32 [V,3], N f32 [V,3] normalised, valid bool [V]): finite points, non-zero finite normals."""
    P = np.asarray(points, dtype=np.float64).astype(F32)
    N = np.asarray(normals, dtype=np.float64).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = _dot(N, N)
        ok = np.isfinite(P).all(1) & np.isfinite(l2) & (l2 > 0)
        ln = np.sqrt(np.where(ok, l2, F32(1)))
        Nn = (N / ln[:, None]).astype(F32)
    return P, Nn, ok


def scene_valid(P):
    P = np.asarray(P, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(P).all(1) & (P[:, 2] > 0)


def bounds(P, ok):
    """-> (lo f32 [3], D f32): componentwise minimum of the valid points and the f32 diagonal of their box."""
    lo, hi = P[ok].min(0), P[ok].max(0)
    e = (hi - lo).astype(F32)
    return lo, F32(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def sample(P, ok, h):
    """SPEC 6.2: voxel floor((p - lo) / h) in f32, the lowest input index per voxel, kept indices ascending."""
    idx = np.nonzero(ok)[0]
    if len(idx) == 0:
        return idx
    lo = P[idx].min(0)
    v = np.floor((P[idx] - lo) / F32(h)).astype(F32)
    _, first = np.unique(v, axis=0, return_index=True)
    return np.sort(idx[first])


def depth2cloud(depth, mask, cam_K):
    """Pixels with mask && depth > 0 in row-major order, back-projected with depth2xyz's expression (SPEC 5.2)."""
    depth = np.asarray(depth, dtype=F32)
    sel = np.asarray(mask).astype(bool) & (depth > 0)
    y, x = np.nonzero(sel)
    z = depth[y, x]
    fx, fy, cx, cy = (F32(v) for v in (cam_K[0][0], cam_K[1][1], cam_K[0][2], cam_K[1][2]))
    X = (x.astype(F32) - cx) * z / fx
    Y = (y.astype(F32) - cy) * z / fy
    return np.stack([X, Y, z], 1).astype(F32)


# ---- 6.4: tables, basis, feature --------------------------------------------------------------------------------------
def tables(h, D):
    """Host tables (f64 -> f32) for a model with sampling step h and diameter D."""
    h64, D64 = float(F32(h)), float(F32(D))
    nd = int(np.floor(D64 / h64)) + 1
    k = np.arange(1, nd, dtype=np.float64)
    ang = [j * math.pi / NA for j in range(1, NA)]
    al = [a * 2.0 * math.pi / NALPHA for a in range(NALPHA)]
    cos_a = np.array([math.cos(x) for x in ang]).astype(F32)
    return {"nd": nd, "dist2": ((k * h64) * (k * h64)).astype(F32), "d2max": F32(D64 * D64), "cos_a": cos_a,
            "sec_c": cos_a, "sec_s": np.array([math.sin(x) for x in ang]).astype(F32),
            "rot_c": np.array([math.cos(x) for x in al]), "rot_s": np.array([math.sin(x) for x in al])}


def basis(n):
    """Duff et al. 2017 branch-free orthonormal basis (e1, e2) of unit normals n f32 [k,3], in f32."""
    n = np.asarray(n, dtype=F32)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    sign = np.copysign(F32(1), nz).astype(F32)
    a = F32(-1) / (sign + nz)
    b = (nx * ny) * a
    e1 = np.stack([F32(1) + ((sign * nx) * nx) * a, sign * b, -(sign * nx)], 1).astype(F32)
    e2 = np.stack([b, sign + (ny * ny) * a, -ny], 1).astype(F32)
    return e1, e2


def sector(u, v, tab):
    """Rotation bin of (u, v) = (d.e1, d.e2): 30 sectors of 12 degrees by sign tests against the host directions."""
    lower = (v < 0) | ((v == 0) & (u < 0))
    u2, v2 = np.where(lower, -u, u).astype(F32), np.where(lower, -v, v).astype(F32)
    b = np.zeros(np.shape(u), dtype=np.int64)
    for c, s in zip(tab["sec_c"], tab["sec_s"]):
        b += ((c * v2) - (s * u2)) >= 0
    return b + 15 * lower


def feature(pr, nr, e1r, e2r, pi, ni, tab):
    """SPEC 6.4 for pairs (reference r, partner i), broadcast -> (ok, key, rotation bin)."""
    d = (pi - pr).astype(F32)
    dist2 = _dot(d, d)
    ok = (dist2 > 0) & (dist2 <= tab["d2max"])
    ln = np.sqrt(np.where(ok, dist2, F32(1))).astype(F32)
    c1 = _dot(nr, d) / ln
    c2 = _dot(ni, d) / ln
    c3 = _dot(nr, ni)
    db = np.zeros(np.shape(dist2), dtype=np.int64)
    for t in tab["dist2"]:
        db += dist2 >= t
    a = [np.zeros(np.shape(dist2), dtype=np.int64) for _ in range(3)]
    for t in tab["cos_a"]:
        for j, c in enumerate((c1, c2, c3)):
            a[j] += c <= t
    key = ((db * NA + a[0]) * NA + a[1]) * NA + a[2]
    return ok, key, sector(_dot(e1r, d), _dot(e2r, d), tab)


# ---- 6.5: the model table -----------------------------------------------------------------------------------------------
class Model:
    """points/normals in the caller's units -> sampled model, tables and the key-sorted entries m_r * 32 + bin_m."""

    def __init__(self, points, normals, rel=0.03):
        P, N, ok = prepare_model(points, normals)
        self.lo, self.D = bounds(P, ok)
        self.h = F32(F32(rel) * self.D)
        self.idx = sample(P, ok, self.h)
        self.P, self.N = P[self.idx], N[self.idx]
        self.e1, self.e2 = basis(self.N)
        self.tab = tables(self.h, self.D)
        Ms = len(self.idx)
        keys, ents = [], []
        for r in range(Ms):
            okp, key, bn = feature(self.P[r], self.N[r], self.e1[r], self.e2[r], self.P, self.N, self.tab)
            okp[r] = False
            keys.append(key[okp])
            ents.append((r * 32 + bn[okp]).astype(np.uint32))
        keys, ents = np.concatenate(keys), np.concatenate(ents)
        order = np.argsort(keys, kind="stable")
        self.keys, self.entries = keys[order], ents[order]
        self.nkeys = self.tab["nd"] * NA ** 3

    @classmethod
    def from_sampled(cls, P, N, h, D):
        """The model of already-sampled points P f32 [Ms,3], unit normals N f32 [Ms,3] and free h, D (what the C ABI
        takes). The keyed pairs are found first by 6.4's own distance test, then `feature` runs on those pairs alone, in
        (r, i) order: the same entries in the same order as __init__'s loop over all pairs."""
        self = cls.__new__(cls)
        self.P, self.N = np.ascontiguousarray(P, dtype=F32).reshape(-1, 3), np.ascontiguousarray(N, dtype=F32).reshape(-1, 3)
        self.h, self.D = F32(h), F32(D)
        Ms = len(self.P)
        self.idx, self.lo = np.arange(Ms), None
        self.e1, self.e2 = basis(self.N)
        self.tab = tables(self.h, self.D)
        rr, ii = [], []
        for r0 in range(0, Ms, 256):
            d = (self.P[None, :, :] - self.P[r0:r0 + 256, None, :]).astype(F32)
            s2 = _dot(d, d)
            r, i = np.nonzero((s2 > 0) & (s2 <= self.tab["d2max"]))
            keep = (r + r0) != i
            rr.append(r[keep] + r0)
            ii.append(i[keep])
        r, i = np.concatenate(rr), np.concatenate(ii)
        okp, key, bn = feature(self.P[r], self.N[r], self.e1[r], self.e2[r], self.P[i], self.N[i], self.tab)
        assert okp.all()
        order = np.argsort(key, kind="stable")
        self.keys, self.entries = key[order], (r * 32 + bn).astype(np.uint32)[order]
        self.nkeys = self.tab["nd"] * NA ** 3
        return self

    def key_entries(self, key):
        a, b = np.searchsorted(self.keys, [key, key + 1])
        return np.sort(self.entries[a:b])


# ---- 6.3: scene normals -----------------------------------------------------------------------------------------------
def smallest_eigvec(C):
    w, V = np.linalg.eigh(C)
    v = V[:, 0]
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def scene_normals(S, h, rel=NORMAL_RADIUS_REL):
    """-> (normals f32 [n,3], ok bool [n]) of the sampled scene S f32 [n,3]."""
    return scene_normals_radius(S, F32(F32(rel) * F32(h)))


def scene_normals_radius(S, radius):
    """scene_normals with the f32 radius r given (what the C ABI takes)."""
    r = float(F32(radius))
    r2 = F32(r * r)
    n = len(S)
    out, ok = np.zeros((n, 3), dtype=F32), np.zeros(n, dtype=bool)
    for i in range(n):
        d = (S - S[i]).astype(F32)
        nb = np.nonzero(_dot(d, d) <= r2)[0]
        if len(nb) < 3:
            continue
        Q = S[nb].astype(np.float64)
        mu = np.cumsum(Q, 0)[-1] / len(nb)
        X = Q - mu
        C = np.cumsum(X[:, :, None] * X[:, None, :], 0)[-1]
        v = smallest_eigvec(C).astype(F32)
        if _dot(v, S[i]) > 0:
            v = -v
        out[i], ok[i] = v, True
    return out, ok


# ---- 6.5 / 6.6: voting, poses, clustering -----------------------------------------------------------------------------
def pose(model, m_r, alpha, s, ns):
    """f64 pose p -> s + B_s Rx(-alpha 12deg) B_m^T (p - m) from f32 inputs, written-out sums."""
    e1s, e2s = basis(ns[None])
    Bs = np.stack([ns, e1s[0], e2s[0]], 1).astype(np.float64)          # columns n, e1, e2
    Bm = np.stack([model.N[m_r], model.e1[m_r], model.e2[m_r]], 1).astype(np.float64)
    c, sn = model.tab["rot_c"][alpha], model.tab["rot_s"][alpha]
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, c, sn], [0.0, -sn, c]])
    M1 = np.empty((3, 3))
    for i in range(3):
        for j in range(3):                                             # Rx . Bm^T
            M1[i, j] = (Rx[i, 0] * Bm[j, 0] + Rx[i, 1] * Bm[j, 1]) + Rx[i, 2] * Bm[j, 2]
    T = np.eye(4)
    for i in range(3):
        for j in range(3):
            T[i, j] = (Bs[i, 0] * M1[0, j] + Bs[i, 1] * M1[1, j]) + Bs[i, 2] * M1[2, j]
    m = model.P[m_r].astype(np.float64)
    for i in range(3):
        T[i, 3] = float(s[i]) - ((T[i, 0] * m[0] + T[i, 1] * m[1]) + T[i, 2] * m[2])
    return T


def vote_acc(model, S, Sn, Sok, r, basis_s=None):
    """The accumulator acc[m_r * 30 + alpha] of reference r (int64 [Ms * 30]), or None when r is dropped or no pair of
    its has a key with entries. Also returns the range lengths of its keyed partners (for the cases' premises)."""
    e1, e2 = basis(Sn) if basis_s is None else basis_s
    if not Sok[r]:
        return None, np.zeros(0, dtype=np.int64)
    okp, key, bs = feature(S[r], Sn[r], e1[r], e2[r], S, Sn, model.tab)
    okp &= np.asarray(Sok, dtype=bool)
    okp[r] = False
    key, bs = key[okp], bs[okp]
    a = np.searchsorted(model.keys, key)
    b = np.searchsorted(model.keys, key + 1)
    ln = b - a
    if ln.sum() == 0:
        return None, ln
    rep = np.repeat(np.arange(len(key)), ln)
    pos = np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln) + np.repeat(a, ln)
    e = model.entries[pos].astype(np.int64)
    alpha = ((e & 31) - bs[rep]) % NALPHA
    return np.bincount((e >> 5) * NALPHA + alpha, minlength=len(model.idx) * NALPHA), ln


def vote(model, S, Sn, Sok, ref_step):
    """-> list over reference indices 0, k, 2k, ... of (ref, m_r, alpha, count) (count 0: no candidate)."""
    bs = basis(Sn)
    out = []
    for r in range(0, len(S), ref_step):
        acc, _ln = vote_acc(model, S, Sn, Sok, r, bs)
        if acc is None:
            out.append((r, 0, 0, 0))
            continue
        best = int(acc.argmax())
        out.append((r, best // NALPHA, best % NALPHA, int(acc[best])))
    return out


def cluster(model, cands, S, Sn, dist_rel=0.1, num_result=100):
    """SPEC 6.6 -> (poses f64 [n,4,4], scores f64 [n])."""
    cs = [c for c in cands if c[3] > 0]
    cs.sort(key=lambda c: (-c[3], c[0]))
    thr = float(F32(dist_rel)) * float(model.D)
    thr2 = thr * thr
    seeds, sums = [], []
    for r, m_r, al, cnt in cs:
        T = pose(model, m_r, al, S[r], Sn[r])
        for j, Ts in enumerate(seeds):
            dt = T[:3, 3] - Ts[:3, 3]
            if ((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]) > thr2:
                continue
            tr = 0.0
            for a in range(3):
                for b in range(3):
                    tr += T[a, b] * Ts[a, b]
            if (tr - 1.0) / 2.0 >= CLUSTER_COS:
                sums[j] += cnt
                break
        else:
            seeds.append(T)
            sums.append(cnt)
    order = sorted(range(len(seeds)), key=lambda j: (-sums[j], j))[:num_result]
    poses = np.array([seeds[j] for j in order]).reshape(-1, 4, 4)
    return poses, np.array([sums[j] / len(model.idx) for j in order], dtype=np.float64)


def cluster_arrays(votes, poses, thr, Ms, num_result=100):
    """SPEC 6.6 over given candidates: votes int [nref] (0: no candidate), poses f64 [nref,4,4], thr = f32(dist_rel) * D as
    f64 -> (poses f64 [k,4,4], scores f64 [k], ncand, nseed). The plain greedy loop in f64, each candidate tested against
    the seeds so far (one numpy expression over the seeds, the sums in 6.6's written order)."""
    votes = np.asarray(votes, dtype=np.int64)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    cs = sorted((j for j in range(len(votes)) if votes[j] > 0), key=lambda j: (-votes[j], j))
    thr2 = float(thr) * float(thr)
    seedT = np.zeros((max(len(cs), 1), 4, 4))
    seeds, sums = [], []
    for j in cs:
        T, ns = poses[j], len(seeds)
        hit = -1
        if ns:
            Ts = seedT[:ns]
            dt = T[None, :3, 3] - Ts[:, :3, 3]
            near = ((dt[:, 0] * dt[:, 0] + dt[:, 1] * dt[:, 1]) + dt[:, 2] * dt[:, 2]) <= thr2
            tr = np.zeros(ns)
            for a in range(3):
                for b in range(3):
                    tr = tr + T[a, b] * Ts[:, a, b]
            ok = near & ((tr - 1.0) / 2.0 >= CLUSTER_COS)
            if ok.any():
                hit = int(np.argmax(ok))
        if hit >= 0:
            sums[hit] += int(votes[j])
        else:
            seedT[ns] = T
            seeds.append(j)
            sums.append(int(votes[j]))
    order = sorted(range(len(seeds)), key=lambda s_: (-sums[s_], s_))[:num_result]
    out = np.array([poses[seeds[s_]] for s_ in order]).reshape(-1, 4, 4)
    return out, np.array([sums[s_] / Ms for s_ in order], dtype=np.float64), len(cs), len(seeds)


# ---- 6.4 a second time: geometry in float64, no sign tests --------------------------------------------------------------
def basis64(n):
    """Duff et al.'s basis of the f32 normals, evaluated in float64."""
    n = np.asarray(n, dtype=np.float64)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    sign = np.copysign(1.0, nz)
    a = -1.0 / (sign + nz)
    b = nx * ny * a
    return (np.stack([1.0 + sign * nx * nx * a, sign * b, -sign * nx], -1), np.stack([b, sign + ny * ny * a, -ny], -1))


def feature_geometric(pr, nr, pi, ni, h, D, ang_margin=1e-5, dist_margin=1e-6):
    """SPEC 6.4 stated by its geometry, in float64 from the f32 inputs: the three angles by arccos, the rotation angle by
    arctan2 in the reference normal's basis, bins by floor(angle / 12 degrees) and floor(l / h).
    -> (ok, key, rotation bin, safe): `safe` is False where a quantity lies within ang_margin rad of an angle bin edge or
    within dist_margin * D of a distance edge (0, k h, D): there float32 may decide either way."""
    pr, nr, pi, ni = (np.asarray(x, dtype=np.float64) for x in (pr, nr, pi, ni))
    h, D = float(F32(h)), float(F32(D))
    d = pi - pr
    l = np.sqrt((d * d).sum(-1))
    ok = (l > 0) & (l <= D)
    ls = np.where(l > 0, l, 1.0)
    step = math.pi / NA
    nd = int(np.floor(D / h)) + 1
    db = np.minimum(np.floor(l / h), nd - 1).astype(np.int64)
    edge = np.minimum(np.abs(l / h - np.round(l / h)) * h, np.abs(l - D))
    safe = edge > dist_margin * D
    bins = []
    for c in ((nr * d).sum(-1) / ls, (ni * d).sum(-1) / ls, (nr * ni).sum(-1)):
        ang = np.arccos(np.clip(c, -1.0, 1.0))
        bins.append(np.minimum(np.floor(ang / step), NA - 1).astype(np.int64))
        safe &= np.abs(ang / step - np.round(ang / step)) * step > ang_margin
    e1, e2 = basis64(nr)
    u, v = (e1 * d).sum(-1), (e2 * d).sum(-1)
    rot = np.mod(np.arctan2(v, u), 2.0 * math.pi)
    rb = np.minimum(np.floor(rot / step), NALPHA - 1).astype(np.int64)
    safe &= np.abs(rot / step - np.round(rot / step)) * step > ang_margin
    safe &= np.hypot(u, v) > ang_margin * ls                  # partner on the normal's axis: no rotation angle
    key = ((db * NA + bins[0]) * NA + bins[1]) * NA + bins[2]
    return ok, key, rb, safe


def find(model, cloud, rel=0.05, ref_rate=0.2, num_result=100, normals=None, trace=None):
    """SPEC 6 end to end on a scene cloud f32 [n,3] -> (poses, scores). `normals` = (Sn, Sok) replaces 6.3;
    `trace`, a dict, receives the intermediate stages."""
    C = np.asarray(cloud, dtype=F32)
    h = F32(F32(rel) * model.D)
    idx = sample(C, scene_valid(C), h)
    S = C[idx]
    Sn, Sok = normals if normals is not None else scene_normals(S, h)
    step = ref_step(ref_rate)
    cands = vote(model, S, Sn, Sok, step)
    poses, scores = cluster(model, cands, S, Sn, num_result=num_result)
    if trace is not None:
        trace.update(idx=idx, S=S, normals=Sn, normals_ok=Sok, cands=cands, h=h)
    return poses, scores


def ref_step(rate):
    return max(1, int(np.floor(1.0 / float(rate) + 0.5)))


# ---- the test object and scene ----------------------------------------------------------------------------------------
def object_model(n=40000, seed=7):
    """Dense surface of ref_icp's ellipsoid with a bump, f64 points and unit normals (object frame, metres)."""
    return ri._surface(n, np.random.default_rng(seed))


POSES = (([0.3, 1.0, 0.2], 25.0, [0.12, 0.06, 0.75]), ([1.0, -0.4, 0.3], 70.0, [-0.10, 0.02, 0.80]),
         ([-0.2, 0.5, 1.0], 140.0, [0.02, -0.09, 0.70]))


def gt_pose(k):
    axis, deg, t = POSES[k]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ri.rot(axis, deg), t
    return T


def box_mask(depth_bg, depth, ratio=1.2):
    """The object's projected box (the pixels the render changed) expanded like online_learning.py:384-405."""
    ys, xs = np.nonzero(depth != depth_bg)
    H, W = depth.shape
    x1, y1, x2, y2 = xs.min(), ys.min(), xs.max() + 1, ys.max() + 1
    cx, cy, hw, hh = (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) / 2 * ratio, (y2 - y1) / 2 * ratio
    x1, y1, x2, y2 = max(0, cx - hw), max(0, cy - hh), min(W - 1, cx + hw), min(H - 1, cy + hh)
    m = np.zeros((H, W), dtype=bool)
    m[int(y1):int(y2), int(x1):int(x2)] = True
    return m


def scene(k, seed=42):
    """-> depth f32 [480,640], cam_K, mask bool [480,640], T_gt for object pose k."""
    from ossid_code_amd import synth
    _img, bg = synth.make_frame(seed)
    T = gt_pose(k)
    depth = ri.render_into(bg, T, synth.CAM_K)
    return depth, synth.CAM_K.copy(), box_mask(bg, depth), T


def best_gap(poses, T_gt, D):
    """-> (translation / D, rotation degrees) of the hypothesis nearest the truth (translation gap + rotation gap in D
    units weighted as the cluster test does)."""
    best = None
    for T in poses:
        dt, dr = ri.pose_gap(T, T_gt)
        v = (dt / float(D), dr)
        if best is None or (v[0] / 0.1 + v[1] / 12.0) < (best[0] / 0.1 + best[1] / 12.0):
            best = v
    return best
