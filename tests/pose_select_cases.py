"""SPEC.md section 16's hand-checkable cases, shared by tests/test_pose_select.py (the restatement against the answers written
out here) and tests/test_pose_select_gpu.py (the kernel against the restatement and the same answers). Every case is
(poses, scores, K, sep, symmetries or None, min_score, selected, owner); the points are POINTS."""
import numpy as np

POINTS = np.random.default_rng(16).uniform(-0.1, 0.1, (37, 3)).astype(np.float32)
NINF = float("-inf")


def at(x, y=0.0, z=1.0, R=None):
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = [x, y, z]
    return T


RZ180 = np.diag([-1.0, -1.0, 1.0, 1.0])          # entries exactly 0, +-1
BELOW = float(np.nextafter(0.25, 0.0))
_pair = np.stack([at(0.0), at(0.25)])
_chain = np.stack([at(0.0), at(0.25), at(0.5)])
_flip = np.stack([at(0.1, 0.2, 1.0), at(0.1, 0.2, 1.0, R=np.diag([-1.0, -1.0, 1.0]))])
_line = np.stack([at(float(i)) for i in range(4)])
_near = np.stack([at(0.0), at(0.05), at(1.0), at(1.05)])

CASES = {
    # q = 0.0625 = sep * sep exactly for every point (a pure translation), and <= suppresses
    "threshold_equal": (_pair, [2, 1], 2, 0.25, None, NINF, [0, -1], [0, 0]),
    "threshold_below": (_pair, [2, 1], 2, BELOW, None, NINF, [0, 1], [0, 1]),
    # suppression is not transitive: pose 2 is 0.5 from pose 0 and survives it; picked second, pose 1 takes both neighbours
    "chain_from_the_end": (_chain, [3, 2, 1], 3, 0.25, None, NINF, [0, 2, -1], [0, 0, 1]),
    "chain_from_the_middle": (_chain, [2, 3, 1], 3, 0.25, None, NINF, [1, -1, -1], [0, 0, 0]),
    "symmetry_unknown": (_flip, [2, 1], 2, 0.01, None, NINF, [0, 1], [0, 1]),
    "symmetry_known": (_flip, [2, 1], 2, 0.01, np.stack([np.eye(4), RZ180]), NINF, [0, -1], [0, 0]),
    # NaN is never eligible; equal scores go to the lower index; -inf is eligible without a bound
    "scores": (_line, [np.nan, 1, 1, NINF], 4, 0.1, None, NINF, [1, 2, 3, -1], [-1, 0, 1, 2]),
    "scores_all_nan": (_line, [np.nan] * 4, 4, 0.1, None, NINF, [-1, -1, -1, -1], [-1, -1, -1, -1]),
    "scores_signed_zero": (_line, [-0.0, 0.0, -1.0, 0.0], 2, 0.1, None, NINF, [0, 1], [0, 1, -1, -1]),
    # below min_score: never picked (3), but owned when within sep of a pick (1)
    "min_score": (_near, [5, 1, 4, 1], 4, 0.1, None, 2.0, [0, 2, -1, -1], [0, 0, 1, 1]),
    "min_score_far": (_line, [5, 1, 4, 2], 4, 0.1, None, 2.0, [0, 2, 3, -1], [0, -1, 1, 2]),
}
