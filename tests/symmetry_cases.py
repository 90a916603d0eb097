"""Edge cases of SPEC.md section 17's scorer (ossid_sym_grid / ossid_sym_score) and the workspace contract (tests/guarded.py)
of its grid buffer, whose size query is ossid_sym_grid_nbytes. Plain helper module: nothing here touches the GPU at import.

A case is (targets f32 [Nt,3], queries f32 [Mq,3], transforms f64 [C,4,4], tol); the sets are seeded, the scorer itself
draws nothing."""
import numpy as np

from guarded import Contract

SHAPES = [(37, 257, 5)]              # (Nt, Mq, C): ragged everywhere -- 37 * 16 bytes of sorted points, 4 waves and one lane


def _rot(axis, angle, t=(0.0, 0.0, 0.0)):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt(a @ a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def blob(Nt, Mq, C, seed=0, tol=0.08):
    """Targets on a unit sphere's surface, queries among and beside them, small and large rotations: hits and misses mixed."""
    rng = np.random.default_rng(seed)
    P = rng.normal(size=(Nt, 3))
    P = (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(np.float32)
    Q = (P[rng.integers(0, Nt, size=Mq)] + rng.normal(scale=0.03, size=(Mq, 3))).astype(np.float32)
    T = np.stack([_rot(rng.normal(size=3), rng.uniform(0.0, 0.2) if c % 2 else rng.uniform(0.0, 3.0), rng.normal(scale=0.01, size=3))
                  for c in range(C)])
    return P, Q, T, tol


def need(lib, s):
    return {"ossid_sym_grid_nbytes": int(lib.fn("ossid_sym_grid_nbytes")(s[0]))}


def pred(lib, s):
    Nt, Mq, C = s
    assert Nt % 4 and Mq % 64 and Mq > 256 and C > 1
    assert need(lib, s)["ossid_sym_grid_nbytes"] % 512


def build(lib, s):
    import torch

    import ref_symmetry as rs
    Nt, Mq, C = s
    P, Q, T, tol = blob(Nt, Mq, C)
    Pd, Qd, Td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (P, Q, T))
    nbytes = need(lib, s)["ossid_sym_grid_nbytes"]

    def run(ws, out):
        g = ws["grid"]
        return lib.fn("ossid_sym_grid")(Pd.data_ptr(), Nt, tol, g.ptr, g.nbytes, None) or \
            lib.fn("ossid_sym_score")(g.ptr, g.nbytes, Nt, Qd.data_ptr(), Mq, Td.data_ptr(), C, tol, out["miss"].ptr,
                                      out["worst_d2"].ptr, out["sum_q"].ptr, None)

    def anchor(out):
        miss, worst, sum_q = rs.score_transforms(P, Q, T, tol)
        assert 0 < miss.sum() < C * Mq
        assert np.array_equal(out["miss"].view(torch.int32).cpu().numpy(), miss)
        assert np.array_equal(out["worst_d2"].view(torch.float32).cpu().numpy().view(np.uint32), worst.view(np.uint32))
        assert np.array_equal(out["sum_q"].view(torch.int64).cpu().numpy(), sum_q)

    # the score entry's own view of the buffer: the grid is built through the full span behind the one the contract hands
    # over (`whole`: the queried bytes at the 256-byte aligned payload), so a short or misaligned span reaches ossid_sym_score
    def run_score(ws, out):
        g = ws["grid"]
        base = g.ptr - g.ptr % 256                              # a span off by 4 lies in the same aligned payload
        rc = lib.fn("ossid_sym_grid")(Pd.data_ptr(), Nt, tol, base, nbytes, None)
        assert rc == 0, rc
        return lib.fn("ossid_sym_score")(g.ptr, g.nbytes, Nt, Qd.data_ptr(), Mq, Td.data_ptr(), C, tol, out["miss"].ptr,
                                         out["worst_d2"].ptr, out["sum_q"].ptr, None)

    outs = {"miss": 4 * C, "worst_d2": 4 * C, "sum_q": 8 * C}
    return [Contract("sym_grid+sym_score %s" % (s,), {"grid": nbytes}, outs, run, anchor, short=("grid",), misalign=("grid",)),
            Contract("sym_score alone %s" % (s,), {"grid": nbytes}, outs, run_score, anchor, short=("grid",), misalign=("grid",))]
