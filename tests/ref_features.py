"""Independent numpy restatement of SPEC.md section 11 (keypoint-feature pose hypotheses), the yardstick of
csrc/features.hip, and the textured test object.

Integers wherever SPEC 11 says integers (grey, scale space, detection, histograms, descriptor sums, matching), float32 in
the written order where it says f32 (sample coordinates, gradient blend, soft binning), float64 for the frames and the
poses. Clustering is SPEC 6.6's, taken from ref_ppf (11.8: it is not restated a second time).
"""
import math

import numpy as np

import ref_ppf
import ref_raster as rr

F32 = np.float32
MAX_KEYPOINTS = 4096
MAX_MODEL_FEATURES = 65536
MIN_SIDE = 8                        # 11.1: an octave exists only if both its sides are >= this
CONTRAST = 192
EDGE_R = 10
RHO = (6, 9)                        # 11.3 window radius for s = 1, 2
SIGMA = (math.sqrt(2.0), 2.0)       # sigma of L_1, L_2 in octave pixels
FRAME_R = (4, 6)                    # 11.5 normal baseline for s = 1, 2 (octave pixels)


# ---- host tables --------------------------------------------------------------------------------------------------------
def _quadrant_table(n_per_quadrant, offset):
    """cos / sin of (k + offset) * 90 / n degrees for k = 0 .. 4 n - 1, f32, the first quadrant computed (cos only, in f64)
    and the rest built by symmetry: sin(a) = cos(90 - a), then (c, s) -> (-s, c) per quadrant."""
    n = n_per_quadrant
    step = 90.0 / n
    if offset == 0.0:       # angles k step: cos for k = 0 .. n, sin_k = cos_{n-k}
        q = [F32(math.cos(k * step * math.pi / 180.0)) for k in range(n + 1)]
        q[0], q[n] = F32(1), F32(0)
        c = [q[k] for k in range(n)]
        s = [q[n - k] for k in range(n)]
    else:                   # angles (k + .5) step: sin_k = cos_{n-1-k}
        q = [F32(math.cos((k + 0.5) * step * math.pi / 180.0)) for k in range(n)]
        c = list(q)
        s = [q[n - 1 - k] for k in range(n)]
    for k in range(n, 4 * n):
        c.append(-s[k - n])
        s.append(c[k - n])
    return np.array(c, dtype=F32), np.array(s, dtype=F32)


SEC_C, SEC_S = _quadrant_table(9, 0.0)          # 36 sector boundaries (k 10 degrees); tests use k = 1 .. 17
ORI_C, ORI_S = _quadrant_table(9, 0.5)          # cos / sin of (b + .5) 10 degrees
R8 = F32(math.sqrt(0.5))
DIR8 = np.array([(1, 0), (R8, R8), (0, 1), (-R8, R8), (-1, 0), (-R8, -R8), (0, -1), (R8, -R8)], dtype=F32)


def ori_weights(s):
    rho, sg = RHO[s - 1], 1.5 * SIGMA[s - 1]
    return np.array([[int(np.rint(1024.0 * math.exp(-(float(dx * dx) + float(dy * dy)) / (2.0 * sg * sg))))
                      for dx in range(-rho, rho + 1)] for dy in range(-rho, rho + 1)], dtype=np.int64)


DESC_GW = np.array([[math.exp(-((i - 7.5) ** 2 + (j - 7.5) ** 2) / 128.0) for j in range(16)] for i in range(16)]).astype(F32)


# ---- 11.1 -----------------------------------------------------------------------------------------------------------------
def grey(img):
    p = np.asarray(img).astype(np.int64)
    return ((77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8).astype(np.int64)


def blur_pass(L):
    k = np.array([1, 4, 6, 4, 1], dtype=np.int64)
    P = np.pad(L, 2, mode="reflect")
    H, W = L.shape
    acc = np.zeros((H, W), dtype=np.int64)
    for i in range(5):
        for j in range(5):
            acc += k[i] * k[j] * P[i:i + H, j:j + W]
    return (acc + 128) >> 8


def octave_sizes(H, W, octaves=3):
    out = [(H, W)]
    while len(out) < octaves:
        h, w = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if h < MIN_SIDE or w < MIN_SIDE:
            break
        out.append((h, w))
    return out


def pyramid(img, octaves=3):
    """-> list per octave of int64 [5, Ho, Wo]."""
    g = grey(img) << 6
    sizes = octave_sizes(g.shape[0], g.shape[1], octaves)
    pyr = []
    for o in range(len(sizes)):
        L0 = blur_pass(g) if o == 0 else pyr[-1][2][::2, ::2]
        lv = [L0]
        for n in (1, 2, 4, 8):
            L = lv[-1]
            for _ in range(n):
                L = blur_pass(L)
            lv.append(L)
        pyr.append(np.stack(lv))
    return pyr


# ---- 11.2 -----------------------------------------------------------------------------------------------------------------
def detect(pyr, depth, mask, contrast=CONTRAST):
    """-> int64 [n, 4] rows (o, s, y, x), ascending."""
    sel = np.asarray(mask).astype(bool) & (np.asarray(depth, dtype=F32) > 0)
    out = []
    for o, Ls in enumerate(pyr):
        D = Ls[1:] - Ls[:-1]
        H, W = D.shape[1:]
        for s in (1, 2):
            c = D[s, 1:-1, 1:-1]
            gt = np.ones(c.shape, dtype=bool)
            lt = np.ones(c.shape, dtype=bool)
            for ds in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if ds == 0 and dy == 0 and dx == 0:
                            continue
                        nb = D[s + ds, 1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
                        gt &= c > nb
                        lt &= c < nb
            Ds = D[s]
            dxx = Ds[1:-1, 2:] + Ds[1:-1, :-2] - 2 * c
            dyy = Ds[2:, 1:-1] + Ds[:-2, 1:-1] - 2 * c
            dxy4 = Ds[2:, 2:] + Ds[:-2, :-2] - Ds[2:, :-2] - Ds[:-2, 2:]
            tr = dxx + dyy
            det4 = 4 * dxx * dyy - dxy4 * dxy4
            keep = (gt | lt) & (np.abs(c) >= contrast) & (det4 > 0) & (4 * EDGE_R * tr * tr < (EDGE_R + 1) ** 2 * det4)
            keep &= sel[np.ix_(np.arange(1, H - 1) << o, np.arange(1, W - 1) << o)]
            ys, xs = np.nonzero(keep)
            out.extend((o, s, int(y) + 1, int(x) + 1) for y, x in zip(ys, xs))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


# ---- 11.3 / 11.4 ----------------------------------------------------------------------------------------------------------
def sector(u, v, cs, sn, half):
    """6.4's sign-test rule with 2 * half sectors on f32 arrays (cs / sn: the boundary directions k = 1 .. half - 1)."""
    lower = (v < 0) | ((v == 0) & (u < 0))
    u2, v2 = np.where(lower, -u, u).astype(F32), np.where(lower, -v, v).astype(F32)
    b = np.zeros(np.shape(u), dtype=np.int64)
    for c, s in zip(cs, sn):
        b += ((c * v2) - (s * u2)) >= 0
    return b + half * lower


def gradients(L):
    """Integer central differences, zero on the border (never read there)."""
    gx = np.zeros_like(L)
    gy = np.zeros_like(L)
    gx[:, 1:-1] = L[:, 2:] - L[:, :-2]
    gy[1:-1, :] = L[2:, :] - L[:-2, :]
    return gx, gy


def orientation(gx, gy, s, y, x):
    """-> bin 0 .. 35, or -1 when the window leaves the image."""
    rho = RHO[s - 1]
    H, W = gx.shape
    if x - rho - 1 < 0 or y - rho - 1 < 0 or x + rho + 1 > W - 1 or y + rho + 1 > H - 1:
        return -1
    wx = gx[y - rho:y + rho + 1, x - rho:x + rho + 1]
    wy = gy[y - rho:y + rho + 1, x - rho:x + rho + 1]
    m = np.sqrt((wx * wx + wy * wy).astype(F32)).astype(np.int64)
    add = (m * ori_weights(s)) >> 10
    b = sector(wx.astype(F32), wy.astype(F32), SEC_C[1:18], SEC_S[1:18], 18)
    h = np.zeros(36, dtype=np.int64)             # a zero gradient has m = 0 and adds nothing
    np.add.at(h, b.ravel(), add.ravel())
    hs = np.roll(h, 1) + 2 * h + np.roll(h, -1)
    return int(np.argmax(hs))


def descriptor(L, gx, gy, s, y, x, b):
    """-> i8 [128] or None (dropped)."""
    H, W = L.shape
    c, sn = ORI_C[b], ORI_S[b]
    hsp = F32(0.75 * SIGMA[s - 1])
    jj = (np.arange(16, dtype=F32) - F32(7.5))
    u = (jj * hsp)[None, :] + np.zeros((16, 1), dtype=F32)
    v = (jj * hsp)[:, None] + np.zeros((1, 16), dtype=F32)
    px = (F32(x) + ((c * u) - (sn * v))).astype(F32)
    py = (F32(y) + ((sn * u) + (c * v))).astype(F32)
    x0f, y0f = np.floor(px), np.floor(py)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    if (x0 - 1 < 0).any() or (y0 - 1 < 0).any() or (x0 + 2 > W - 1).any() or (y0 + 2 > H - 1).any():
        return None
    ax, ay = (px - x0f).astype(F32), (py - y0f).astype(F32)
    one = F32(1)

    def blend(g):
        g00, g01 = g[y0, x0].astype(F32), g[y0, x0 + 1].astype(F32)
        g10, g11 = g[y0 + 1, x0].astype(F32), g[y0 + 1, x0 + 1].astype(F32)
        return ((g00 * (one - ax) + g01 * ax) * (one - ay)) + ((g10 * (one - ax) + g11 * ax) * ay)
    bx, by = blend(gx), blend(gy)
    gu = ((c * bx) + (sn * by)).astype(F32)
    gv = ((c * by) - (sn * bx)).astype(F32)
    k = sector(gu, gv, DIR8[1:4, 0], DIR8[1:4, 1], 4)
    d0, d1 = DIR8[k], DIR8[(k + 1) % 8]
    a = (((gu * d1[..., 1]) - (gv * d1[..., 0])) / R8).astype(F32)
    bb = (((d0[..., 0] * gv) - (d0[..., 1] * gu)) / R8).astype(F32)
    acc = np.zeros(128, dtype=np.int64)
    ii = np.arange(16)
    cc = (ii - 1.5) / 4.0
    c0 = np.floor(cc).astype(np.int64)
    f = (cc - c0).astype(F32)                       # exact dyadic
    for i in range(16):
        for j in range(16):
            for cy, wy in ((c0[i], one - f[i]), (c0[i] + 1, f[i])):
                if not 0 <= cy < 4:
                    continue
                for cx, wx in ((c0[j], one - f[j]), (c0[j] + 1, f[j])):
                    if not 0 <= cx < 4:
                        continue
                    for coef, kk in ((a[i, j], k[i, j]), (bb[i, j], (k[i, j] + 1) % 8)):
                        val = F32(F32(F32(coef * wy) * wx) * DESC_GW[i, j])
                        acc[(cy * 4 + cx) * 8 + kk] += int(np.rint(val))
    S = int((acc * acc).sum())
    cap = int(math.floor(0.2 * math.sqrt(float(S))))
    vc = np.minimum(acc, cap)
    S2 = int((vc * vc).sum())
    if S2 == 0:
        return None
    q = np.minimum(127, np.rint(256.0 * vc.astype(np.float64) / math.sqrt(float(S2))).astype(np.int64))
    return q.astype(np.int8)


# ---- 11.5 -----------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def frame(depth, cam_K, o, s, y, x, b):
    """-> f64 [4,4] or None (dropped)."""
    depth = np.asarray(depth, dtype=F32)
    H, W = depth.shape
    fx, fy, cx, cy = (F32(v) for v in (cam_K[0][0], cam_K[1][1], cam_K[0][2], cam_K[1][2]))
    xf, yf = x << o, y << o
    r = FRAME_R[s - 1] << o

    def backproject(px, py):
        z = depth[py, px]
        return np.array([(F32(px) - cx) * z / fx, (F32(py) - cy) * z / fy, z], dtype=F32)
    if xf - r < 0 or yf - r < 0 or xf + r > W - 1 or yf + r > H - 1:
        return None
    Z = depth[yf, xf]
    nb = []
    for px, py in ((xf + r, yf), (xf - r, yf), (xf, yf + r), (xf, yf - r)):
        zn = depth[py, px]
        if not zn > 0 or not np.abs(F32(zn - Z)) <= F32(F32(0.05) * Z):
            return None
        nb.append(backproject(px, py).astype(np.float64))
    P = backproject(xf, yf).astype(np.float64)
    n = _cross(nb[0] - nb[1], nb[2] - nb[3])
    l2 = _dot3(n, n)
    if not l2 > 0.0:
        return None
    n = n / math.sqrt(l2)
    if _dot3(n, P) > 0.0:
        n = -n
    c, sn = float(ORI_C[b]), float(ORI_S[b])
    ray = np.array([((float(xf) + c) - float(cx)) / float(fx), ((float(yf) + sn) - float(cy)) / float(fy), 1.0])
    den = _dot3(n, ray)
    if abs(den) < 1e-6:
        return None
    nP = _dot3(n, P)
    Pp = (ray * nP) / den
    e1 = Pp - P
    e1 = e1 - n * _dot3(n, e1)
    l2 = _dot3(e1, e1)
    if not l2 > 0.0:
        return None
    e1 = e1 / math.sqrt(l2)
    e2 = _cross(n, e1)
    F = np.eye(4)
    F[:3, 0], F[:3, 1], F[:3, 2], F[:3, 3] = e1, e2, n, P
    return F


def featurize(img, depth, mask, cam_K, contrast=CONTRAST, max_keypoints=MAX_KEYPOINTS, octaves=3, trace=None):
    """11.1-11.5 -> (kps int64 [n,4], bins int64 [n], desc i8 [n,128], frames f64 [n,4,4], ok bool [n])."""
    pyr = pyramid(img, octaves)
    kps = detect(pyr, depth, mask, contrast)
    if trace is not None:
        trace.update(pyramid=pyr, keypoints=kps)
    if len(kps) > max_keypoints:
        raise ValueError("featurize: %d keypoints, more than max_keypoints = %d; raise contrast" % (len(kps), max_keypoints))
    n = len(kps)
    bins = np.full(n, -1, dtype=np.int64)
    desc = np.zeros((n, 128), dtype=np.int8)
    frames = np.zeros((n, 4, 4))
    ok = np.zeros(n, dtype=bool)
    grads = {}
    for i, (o, s, y, x) in enumerate(kps.tolist()):
        if (o, s) not in grads:
            grads[(o, s)] = gradients(pyr[o][s])
        gx, gy = grads[(o, s)]
        b = orientation(gx, gy, s, y, x)
        bins[i] = b
        if b < 0:
            continue
        d = descriptor(pyr[o][s], gx, gy, s, y, x, b)
        if d is None:
            continue
        F = frame(depth, cam_K, o, s, y, x, b)
        if F is None:
            continue
        desc[i], frames[i], ok[i] = d, F, True
    return kps, bins, desc, frames, ok


def smoothed_histogram(gx, gy, s, y, x):
    """11.3's smoothed 36-bin histogram of a keypoint whose window lies in the image; orientation() is its first arg-max."""
    rho = RHO[s - 1]
    wx = gx[y - rho:y + rho + 1, x - rho:x + rho + 1]
    wy = gy[y - rho:y + rho + 1, x - rho:x + rho + 1]
    m = np.sqrt((wx * wx + wy * wy).astype(F32)).astype(np.int64)
    add = (m * ori_weights(s)) >> 10
    b = sector(wx.astype(F32), wy.astype(F32), SEC_C[1:18], SEC_S[1:18], 18)
    h = np.zeros(36, dtype=np.int64)
    np.add.at(h, b.ravel(), add.ravel())
    return np.roll(h, 1) + 2 * h + np.roll(h, -1)


def describe_rows(pyr, depth, cam_K, kps):
    """11.3-11.5 on given keypoint rows (o, s, y, x), the per-row part of featurize: pyr a list per octave of [5,Ho,Wo]
    -> (bins int64 [n], desc i8 [n,128], frames f64 [n,4,4], ok bool [n])."""
    kps = np.asarray(kps, dtype=np.int64).reshape(-1, 4)
    n = len(kps)
    bins = np.full(n, -1, dtype=np.int64)
    desc = np.zeros((n, 128), dtype=np.int8)
    frames = np.zeros((n, 4, 4))
    ok = np.zeros(n, dtype=bool)
    grads = {}
    for i, (o, s, y, x) in enumerate(kps.tolist()):
        if (o, s) not in grads:
            grads[(o, s)] = gradients(np.asarray(pyr[o][s], dtype=np.int64))
        gx, gy = grads[(o, s)]
        b = orientation(gx, gy, s, y, x)
        bins[i] = b
        if b < 0:
            continue
        d = descriptor(pyr[o][s], gx, gy, s, y, x, b)
        if d is None:
            continue
        F = frame(depth, cam_K, o, s, y, x, b)
        if F is None:
            continue
        desc[i], frames[i], ok[i] = d, F, True
    return bins, desc, frames, ok


def match_matrix(desc_s, ok_s, desc_m):
    """match() in matrix form: d2 = |a|^2 + |b|^2 - 2 A B^T in int64, the first minimum per row -> (best, d2, w)."""
    A = np.asarray(desc_s).astype(np.int64)
    B = np.asarray(desc_m).astype(np.int64)
    n = len(A)
    best, d2b = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    okv = np.asarray(ok_s).astype(bool)
    if len(B) and okv.any():
        nb = (B * B).sum(1)
        rows = np.flatnonzero(okv)
        for a in range(0, len(rows), 256):                      # by blocks of scene rows: bounded memory at 65536 model rows
            r = rows[a:a + 256]
            d2 = (A[r] * A[r]).sum(1)[:, None] + nb[None, :] - 2 * (A[r] @ B.T)
            j = np.argmin(d2, axis=1)
            best[r], d2b[r] = j, d2[np.arange(len(r)), j]
    w = np.where(best >= 0, np.maximum(0, 1024 - (d2b >> 6)), 0)
    return best, d2b, w


# ---- 11.6 -----------------------------------------------------------------------------------------------------------------
def rigid_inverse(T):
    """[R | t] -> [R^T | -(R^T t)] in the written order."""
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    for j in range(3):
        out[j, 3] = -((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2])
    return out


def rigid_mul(A, B):
    """A . B for [R | t] matrices, each element (a0 b0 + a1 b1) + a2 b2, translation + A's."""
    out = np.eye(4)
    for a in range(3):
        for b in range(3):
            out[a, b] = (A[a, 0] * B[0, b] + A[a, 1] * B[1, b]) + A[a, 2] * B[2, b]
        out[a, 3] = ((A[a, 0] * B[0, 3] + A[a, 1] * B[1, 3]) + A[a, 2] * B[2, 3]) + A[a, 3]
    return out


def model_features(view_images, view_depths, view_cams, view_poses, contrast=CONTRAST):
    """view_*: per view the rendered colour u8 [S,S,3], depth f32 [S,S], intrinsics (fx, fy, cx, cy) f32 and the pose
    T_v f64 [4,4] -> (desc i8 [Nm,128], frames f64 [Nm,4,4]) in the object's frame."""
    descs, frames = [], []
    for img, dep, cam, T in zip(view_images, view_depths, view_cams, view_poses):
        K = [[cam[0], 0, cam[2]], [0, cam[1], cam[3]], [0, 0, 1]]
        _k, _b, d, F, ok = featurize(img, dep, np.asarray(dep) > 0, K, contrast)
        Ti = rigid_inverse(np.asarray(T, dtype=np.float64))
        for i in np.nonzero(ok)[0]:
            descs.append(d[i])
            frames.append(rigid_mul(Ti, F[i]))
    if len(descs) > MAX_MODEL_FEATURES:
        raise ValueError("model features: %d, more than %d; raise contrast or lower level" % (len(descs), MAX_MODEL_FEATURES))
    return np.array(descs, dtype=np.int8).reshape(-1, 128), np.array(frames).reshape(-1, 4, 4)


# ---- 11.7 / 11.8 ----------------------------------------------------------------------------------------------------------
def match(desc_s, ok_s, desc_m):
    """-> (best j int64 [Ns] (-1 = skipped), d2 int64 [Ns], w int64 [Ns])."""
    A = np.asarray(desc_s).astype(np.int64)
    B = np.asarray(desc_m).astype(np.int64)
    n = len(A)
    best, d2b = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int64)
    if len(B):
        for i in range(n):
            if not ok_s[i]:
                continue
            d2 = ((A[i][None, :] - B) ** 2).sum(1)
            best[i] = int(np.argmin(d2))
            d2b[i] = d2[best[i]]
    w = np.where(best >= 0, np.maximum(0, 1024 - (d2b >> 6)), 0)
    return best, d2b, w


def candidate_poses(frames_s, frames_m, best, w):
    T = np.zeros((len(best), 4, 4))
    for i in range(len(best)):
        if w[i] > 0:
            T[i] = rigid_mul(frames_s[i], rigid_inverse(frames_m[best[i]]))
    return T


def cluster(T, w, D, dist_rel=0.1, num_result=100):
    """SPEC 6.6 through ref_ppf.cluster: votes w, reference index = scene feature index, score = sum w / 1024."""
    class _M:
        pass
    m = _M()
    m.D, m.idx = F32(D), range(1024)
    cands = [(i, i, 0, int(w[i])) for i in range(len(w))]
    saved = ref_ppf.pose
    ref_ppf.pose = lambda model, m_r, al, s, ns: T[m_r]
    try:
        return ref_ppf.cluster(m, cands, [None] * len(w), [None] * len(w), dist_rel, num_result)
    finally:
        ref_ppf.pose = saved


def find_hypotheses(img, depth, mask, cam_K, desc_m, frames_m, D, contrast=CONTRAST, num_result=100, trace=None):
    kps, bins, desc, frames, ok = featurize(img, depth, mask, cam_K, contrast)
    best, d2, w = match(desc, ok, desc_m)
    T = candidate_poses(frames, frames_m, best, w)
    poses, scores = cluster(T, w, D, num_result=num_result)
    if trace is not None:
        trace.update(keypoints=kps, bins=bins, desc=desc, frames=frames, ok=ok, best=best, d2=d2, w=w, cand=T)
    return poses, scores


# ---- the test object ------------------------------------------------------------------------------------------------------
def textured_mesh(level, blobs=400, seed=11, sig=(0.002, 0.006)):
    """ref_raster.bump_mesh(level) with seeded vertex colours: `blobs` Gaussian blobs on the surface, sigma 4-12 mm,
    per-channel amplitudes, on mid grey -> (V f64, F int32, colours u8 [V,3])."""
    V, F = rr.bump_mesh(level)
    rng = np.random.default_rng(seed)
    centres = V[rng.integers(0, len(V), blobs)]
    sig = rng.uniform(sig[0], sig[1], blobs)
    amp = rng.uniform(-110.0, 110.0, (blobs, 3))
    col = np.full((len(V), 3), 128.0)
    for c, s, a in zip(centres, sig, amp):
        d2 = ((V - c) ** 2).sum(1)
        col += np.exp(-d2 / (2.0 * s * s))[:, None] * a
    return V, F, np.clip(np.rint(col), 0, 255).astype(np.uint8)


def mesh_diameter(V):
    """SPEC 6.1's D of the f32 vertices."""
    P = np.asarray(V, dtype=np.float64).astype(F32)
    e = (P.max(0) - P.min(0)).astype(F32)
    return F32(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def view_poses(rotations, distance):
    T = np.tile(np.eye(4), (len(rotations), 1, 1))
    T[:, :3, :3], T[:, 2, 3] = rotations, distance
    return T


def useful(T, T_gt, D):
    """6.6's "same pose" basin: within 0.1 D and 12 degrees."""
    import ref_icp as ri
    dt, dr = ri.pose_gap(T, T_gt)
    return dt <= 0.1 * float(D) and dr <= 12.0
