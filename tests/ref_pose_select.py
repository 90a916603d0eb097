"""Numpy restatement of SPEC.md section 16 (distinct-pose selection): greedy non-maximum suppression over scored poses under
8.7's squared MSSD distance. f64, the written order of operations, elementwise products only (never `@`), so the kernel
(csrc/pose_select.hip) can be held to it integer for integer. Slow on purpose: one pick at a time, one symmetry at a time."""
import numpy as np

F32 = np.float32
MAX_POSES, MAX_INSTANCES, MAX_SYMMETRIES, MAX_POINTS = 65536, 64, 4096, 1 << 22


def _compose(Pg, S):
    """8.7: G = [R_gt . S_R | R_gt . S_t + t_gt], each element (a0 b0 + a1 b1) + a2 b2, the translation + t last."""
    G = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            G[r, c] = (Pg[r, 0] * S[0, c] + Pg[r, 1] * S[1, c]) + Pg[r, 2] * S[2, c]
        G[r, 3] = ((Pg[r, 0] * S[0, 3] + Pg[r, 1] * S[1, 3]) + Pg[r, 2] * S[2, 3]) + Pg[r, 3]
    return G


def _transform(T, P):
    """T [..., 3|4, 4], P f64 [M,3] -> X, Y, Z of shape [..., M]: ((r0 x + r1 y) + r2 z) + t."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return [((T[..., r, 0, None] * x + T[..., r, 1, None] * y) + T[..., r, 2, None] * z) + T[..., r, 3, None] for r in range(3)]


def distances(poses, p, points, symmetries):
    """D(n, p) f64 [N] for every candidate n against the pick p: min over symmetries of max over points of q_v."""
    P = np.asarray(points).astype(F32).astype(np.float64)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    syms = np.asarray(symmetries, dtype=np.float64).reshape(-1, 4, 4)
    with np.errstate(all="ignore"):
        Xe, Ye, Ze = _transform(poses, P)                              # [N, M]
        D = np.full(len(poses), np.inf)
        for S in syms:
            Xg, Yg, Zg = _transform(_compose(poses[p], S), P)          # [M]
            dx, dy, dz = Xe - Xg, Ye - Yg, Ze - Zg
            q = (dx * dx + dy * dy) + dz * dz
            q = np.where(np.isnan(q), np.inf, q)
            D = np.minimum(D, q.max(axis=1))
    return D


def select(poses, scores, points, K, sep, symmetries=None, min_score=-np.inf):
    """-> (selected int32 [K], count int32 [1], owner int32 [N])."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    scores = np.asarray(scores).astype(F32).reshape(-1)
    N = len(poses)
    syms = np.eye(4)[None] if symmetries is None else np.asarray(symmetries, dtype=np.float64).reshape(-1, 4, 4)
    M = len(np.asarray(points))
    if not (1 <= N <= MAX_POSES and len(scores) == N and 1 <= K <= MAX_INSTANCES and 1 <= len(syms) <= MAX_SYMMETRIES
            and 1 <= M <= MAX_POINTS and np.isfinite(sep) and sep >= 0 and not np.isnan(min_score)):
        raise ValueError("outside section 16's caps")
    thr = np.float64(sep) * np.float64(sep)
    with np.errstate(invalid="ignore"):
        eligible = scores >= F32(min_score)                           # false for NaN
    selected = np.full(K, -1, dtype=np.int32)
    owner = np.full(N, -1, dtype=np.int32)
    count = 0
    for r in range(K):
        free = np.flatnonzero(eligible & (owner < 0))
        if len(free) == 0:
            break
        p = int(free[np.argmax(scores[free])])                         # the first maximum: the lowest index; +0 == -0
        selected[r] = p
        count += 1
        near = distances(poses, p, points, syms) <= thr
        owner[near & (owner < 0)] = r
        owner[p] = r
    return selected, np.array([count], dtype=np.int32), owner
