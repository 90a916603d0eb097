"""Independent numpy restatement of SPEC.md 6.9 (dense pose refinement of PPF hypotheses), the yardstick of
csrc/ppf_refine.hip, on top of tests/ref_ppf.py.

float32 where SPEC 6.9 says f32 (sampling, the inverse transform of the scene points, d2 and the threshold test), float64
for the moments, the Cholesky solve and the pose update. Correspondences are a brute-force nearest neighbour over the
refinement model points, chunked over the scene points, ties to the lowest model index.
"""
import math

import numpy as np

import ref_ppf as rp

F32 = rp.F32
REFINE_SAMPLING_REL = 0.02          # SPEC 6.9 defaults
REFINE_STEPS = 5


def refine_step_h(rel, D):
    return F32(F32(rel) * F32(D))


def thresholds(D, h_r, steps=REFINE_STEPS):
    """thr_k = f32(max(0.1 * 2^-k * D, 2 * h_r)) in f64 from the f32 D and h_r."""
    return [F32(max(0.1 * 2.0 ** -k * float(F32(D)), 2.0 * float(F32(h_r)))) for k in range(steps)]


class RefineModel:
    """The refinement surface of a model: its valid vertices sampled at h_r = f32(rel) * D, file normals normalised."""

    def __init__(self, points, normals, rel=REFINE_SAMPLING_REL):
        P, N, ok = rp.prepare_model(points, normals)
        _lo, self.D = rp.bounds(P, ok)
        self.h = refine_step_h(rel, self.D)
        self.idx = rp.sample(P, ok, self.h)
        self.P, self.N = P[self.idx], N[self.idx]


def scene_points(cloud, D, rel=REFINE_SAMPLING_REL):
    """The refinement scene: the valid points of an f32 cloud sampled with the model's h_r -> (indices, points)."""
    C = np.asarray(cloud, dtype=F32)
    idx = rp.sample(C, rp.scene_valid(C), refine_step_h(rel, D))
    return idx, C[idx]


def inverse_f32(T):
    """(R^T, -R^T t) of an f64 pose, each element a written-out f64 sum, cast to f32."""
    R, t = np.asarray(T, dtype=np.float64)[:3, :3], np.asarray(T, dtype=np.float64)[:3, 3]
    Ri = R.T.copy()
    ti = np.array([-((Ri[j, 0] * t[0] + Ri[j, 1] * t[1]) + Ri[j, 2] * t[2]) for j in range(3)])
    return Ri.astype(F32), ti.astype(F32)


def to_model_frame(T, S):
    """Scene points f32 [n,3] into the model frame by the f32 inverse of T, SPEC 3.2's parenthesisation."""
    Ri, ti = inverse_f32(T)
    S = np.asarray(S, dtype=F32)
    cols = [((Ri[j, 0] * S[:, 0] + Ri[j, 1] * S[:, 1]) + Ri[j, 2] * S[:, 2]) + ti[j] for j in range(3)]
    return np.stack(cols, 1).astype(F32)


def nearest(X, M, chunk=1024):
    """Brute force: for each row of X the lowest-index nearest row of M under the f32 d2 -> (index, d2 f32)."""
    idx = np.empty(len(X), dtype=np.int64)
    best = np.empty(len(X), dtype=F32)
    for a in range(0, len(X), chunk):
        d = (X[a:a + chunk, None, :] - M[None, :, :]).astype(F32)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        j = np.argmin(d2, axis=1)                       # first minimum: ties to the lowest index
        idx[a:a + chunk] = j
        best[a:a + chunk] = d2[np.arange(len(j)), j]
    return idx, best


def correspondences(T, S, M, thr):
    """SPEC 6.9 at pose T: -> (scene indices, model indices, d2) of the accepted pairs, scene order."""
    X = to_model_frame(T, S)
    j, d2 = nearest(X, M)
    ok = d2 <= F32(float(thr) * float(thr))
    return np.nonzero(ok)[0], j[ok], d2[ok], X


def moments(X, M, N):
    """Point-to-plane normal equations of pairs (x, m, n) f32 [k,3] -> A f64 [6,6], g f64 [6]."""
    x, m, n = (np.asarray(a, dtype=np.float64) for a in (X, M, N))
    c = np.stack([x[:, 1] * n[:, 2] - x[:, 2] * n[:, 1], x[:, 2] * n[:, 0] - x[:, 0] * n[:, 2],
                  x[:, 0] * n[:, 1] - x[:, 1] * n[:, 0]], 1)
    d = x - m
    r = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    J = np.concatenate([c, n], 1)
    return J.T @ J, J.T @ r


def cholesky_solve(A, g):
    """A delta = -g by Cholesky in f64; None when a pivot is <= 1e-12 * trace(A) / 6."""
    tol = 1e-12 * float(np.trace(A)) / 6.0
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j] - sum(L[j, k] * L[j, k] for k in range(j))
        if not s > tol:
            return None
        L[j, j] = math.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - sum(L[i, k] * y[k] for k in range(i))) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - sum(L[k, i] * x[k] for k in range(i + 1, 6))) / L[i, i]
    return x


def rodrigues(w):
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + W
    K = W / th
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def update(T, delta):
    """T <- T . [dR^T | -dR^T tau] with dR = Rodrigues(omega), delta = (omega, tau)."""
    dR = rodrigues(delta[:3])
    out = np.eye(4)
    out[:3, :3] = np.asarray(T)[:3, :3] @ dR.T
    out[:3, 3] = np.asarray(T)[:3, 3] - out[:3, :3] @ delta[3:]
    return out


def refine_one(T, S, model, steps=REFINE_STEPS, trace=None):
    """SPEC 6.9 on one pose -> (pose f64 [4,4], pairs at the final pose within thr_{steps-1}, steps done)."""
    thr = thresholds(model.D, model.h, steps)
    T = np.asarray(T, dtype=np.float64).copy()
    done = 0
    for k in range(steps):
        si, mi, _d2, X = correspondences(T, S, model.P, thr[k])
        if trace is not None:
            trace.append((T.copy(), si, mi))
        if len(si) < 6:
            break
        A, g = moments(X[si], model.P[mi], model.N[mi])
        delta = cholesky_solve(A, g)
        if delta is None:
            break
        T = update(T, delta)
        done += 1
    si, _mi, _d2, _X = correspondences(T, S, model.P, thr[steps - 1])
    return T, len(si), done


def refine(poses, S, model, steps=REFINE_STEPS):
    """Every hypothesis, then sorted by refined score descending, ties by input rank -> (poses, scores, pairs, steps,
    order) where order[i] is the input rank of output row i."""
    rows = [refine_one(T, S, model, steps) for T in poses]
    order = sorted(range(len(rows)), key=lambda i: (-rows[i][1], i))
    P = np.array([rows[i][0] for i in order]).reshape(-1, 4, 4)
    pairs = np.array([rows[i][1] for i in order], dtype=np.int64)
    return P, pairs / float(len(model.idx)), pairs, np.array([rows[i][2] for i in order], dtype=np.int64), order
