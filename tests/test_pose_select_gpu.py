"""SPEC.md section 16 on the device: ossid_pose_select through the C ABI against the restatement tests/ref_pose_select.py --
selected, count and owner are integers and must be EQUAL -- on the hand-checked cases, at the kernel's tile edges, on a
randomised three-cluster frame, with a NaN pose, twice over prefilled outputs, and its refusals; then
scoring.select_instances, which hands the same arrays on."""
import numpy as np
import pytest
import torch

import pose_select_cases as pc
import ref_pose_select as rp
from ossid_code_amd import scoring

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = np.frombuffer(bytes([0xA5] * 4), dtype=np.int32)[0]
NINF = float("-inf")


def _abi(hiplib, poses, scores, points, K, sep, syms=None, min_score=NINF, expect=0):
    """-> (selected [K], count [1], owner [N], keys [K]) with every output prefilled with 0xA5 bytes and GUARD words behind
    each checked; on a refusal (expect = -22) nothing at all may have been written."""
    dev = torch.device("cuda", 0)
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    N, M = len(poses), len(points)
    syms = np.eye(4)[None] if syms is None else np.ascontiguousarray(syms, dtype=np.float64)
    T = torch.from_numpy(poses).to(dev)
    sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)).to(dev)
    P = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
    Sm = torch.from_numpy(syms).to(dev)
    nk = max(K, 1)
    sel = torch.full(((nk + GUARD) * 4,), 0xA5, dtype=torch.uint8, device=dev)
    cnt = torch.full(((1 + GUARD) * 4,), 0xA5, dtype=torch.uint8, device=dev)
    own = torch.full(((N + GUARD) * 4,), 0xA5, dtype=torch.uint8, device=dev)
    keys = torch.full(((nk + GUARD) * 8,), 0xA5, dtype=torch.uint8, device=dev)
    rc = hiplib.fn("ossid_pose_select")(T.data_ptr(), sc.data_ptr(), N, P.data_ptr(), M, Sm.data_ptr(), len(syms), K, float(sep),
                                        float(min_score), sel.data_ptr(), cnt.data_ptr(), own.data_ptr(), keys.data_ptr(),
                                        hiplib.stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    s, c, o = (t.cpu().numpy().view(np.int32) for t in (sel, cnt, own))
    k = keys.cpu().numpy().view(np.uint64)
    if expect:
        assert (s == FILL).all() and (c == FILL).all() and (o == FILL).all() and (k == 0xA5A5A5A5A5A5A5A5).all()
        return None
    assert (s[K:] == FILL).all() and (c[1:] == FILL).all() and (o[N:] == FILL).all() and (k[K:] == 0xA5A5A5A5A5A5A5A5).all()
    return s[:K].copy(), c[:1].copy(), o[:N].copy(), k[:K].copy()


def _equal(got, want):
    return all(g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got[:3], want))


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_hand_checked_cases(hiplib, case):
    poses, scores, K, sep, syms, min_score, want_sel, want_owner = pc.CASES[case]
    got = _abi(hiplib, poses, scores, pc.POINTS, K, sep, syms, min_score)
    print(case, got[0].tolist(), got[1].tolist(), got[2].tolist())
    assert got[0].tolist() == want_sel and got[2].tolist() == want_owner and got[1].tolist() == [sum(v >= 0 for v in want_sel)]
    assert _equal(got, rp.select(poses, scores, pc.POINTS, K, sep, syms, min_score))


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.sqrt((a * a).sum())
    th = np.deg2rad(deg)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def _rz_syms(S):
    out = np.tile(np.eye(4), (S, 1, 1))
    for i in range(S):
        out[i, :3, :3] = _rot((0, 0, 1), i * 360.0 / S)
    return out


def _frame(seed, N, M, S, clusters, sep, sigma=0.004, tie_scores=True):
    """N candidates around `clusters` centres on a grid 3 sep apart (so picks of different clusters never suppress each
    other), each a small random rotation off its centre's, turned by a random element of the S-fold symmetry about z (near
    its cluster only through the symmetry), jittered by sigma; scores from a short list, so equal scores are common."""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-0.1, 0.1, (M, 3)).astype(np.float32)
    syms = _rz_syms(S)
    side = int(np.ceil(np.sqrt(clusters)))
    centres = np.array([[3.0 * sep * (c % side), 3.0 * sep * (c // side), 1.0] for c in range(clusters)])
    base = [_rot(rng.normal(size=3), rng.uniform(0, 180)) for _ in range(clusters)]
    member = np.concatenate([np.arange(clusters), rng.integers(0, clusters, max(0, N - clusters))])[:N]
    poses = np.tile(np.eye(4), (N, 1, 1))
    for n, c in enumerate(member):
        R = base[c] @ _rot(rng.normal(size=3), rng.normal(0.0, 1.0)) @ syms[rng.integers(0, S), :3, :3]
        poses[n, :3, :3] = R
        poses[n, :3, 3] = centres[c] + rng.normal(0.0, sigma, 3)
    scores = rng.choice(np.array([0.5, 1.0, 2.0, 3.0, -1.0], np.float32), N) if tie_scores else rng.random(N).astype(np.float32)
    return poses, scores, points, syms, member


# (N, M, S, K, clusters): the suppress kernel takes 16 candidates a workgroup (4 waves x 4) and 4 symmetries a chunk, its
# lanes stride the points by the wave's 64; the pick kernel takes 1024 candidates a workgroup (256 lanes x 4).
EDGES = {
    "N1_M1_S1_K1": (1, 1, 1, 1, 1),                   # one of everything: a single lane has a point
    "N15": (15, 37, 1, 4, 3),                         # one below the suppress tile: the last wave has three candidates
    "N17": (17, 37, 1, 4, 3),                         # one above: a second workgroup holding one candidate
    "N1023": (1023, 5, 1, 3, 6),                      # one below the pick workgroup's span
    "N1025": (1025, 5, 1, 3, 6),                      # one above: a second pick workgroup with one candidate
    "M63": (40, 63, 2, 3, 3),                         # one below the wave: one step, the last lane idle
    "M65": (40, 65, 2, 3, 3),                         # one above: a second step with one lane
    "M257": (40, 257, 1, 3, 3),                       # no multiple of the wave or of the workgroup's 256
    "S3": (40, 37, 3, 3, 3),                          # one below a symmetry chunk: one slot never compared
    "S5": (40, 37, 5, 3, 3),                          # one above: a second chunk with one live transform
    "S9_K1": (33, 70, 9, 1, 4),                       # K = 1: one round, three chunks
    "K64_full": (150, 9, 1, 64, 70),                  # 70 mutually distant clusters: every one of the 64 rounds picks
    "K64_padded": (90, 9, 2, 64, 5),                  # more rounds than clusters: count = 5, the rest -1
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_tile_edges_equal_the_restatement(hiplib, case):
    N, M, S, K, clusters = EDGES[case]
    sep = 0.04
    poses, scores, points, syms, member = _frame(len(case) * 131 + N, N, M, S, clusters, sep)
    if case[0] == "N":
        scores[-1] = 9.0                              # the first pick is the last candidate: the one past the boundary
    want = rp.select(poses, scores, points, K, sep, syms)
    assert case[0] != "N" or want[0][0] == N - 1
    got = _abi(hiplib, poses, scores, points, K, sep, syms)
    print(case, "picks", got[1].tolist(), got[0].tolist()[:8], "owned", int((got[2] >= 0).sum()), "of", N)
    assert _equal(got, want)
    if case == "K64_full":
        assert got[1][0] == 64 and (got[0] >= 0).all() and len(set(member[got[0]])) == 64
    if case == "K64_padded":
        assert got[1][0] == 5 and (got[0][5:] == -1).all() and (got[2] >= 0).all()
    # the scratch is an output too: round r's key names its pick, 0 a round without one
    for r in range(K):
        assert (int(got[3][r]) == 0) == (got[0][r] < 0)
        if got[0][r] >= 0:
            assert 0xffffffff - (int(got[3][r]) & 0xffffffff) == got[0][r]


def test_three_clusters_one_pick_each(hiplib):
    sep = 0.04
    poses, scores, points, syms, member = _frame(2024, 200, 37, 1, 3, sep, tie_scores=False)
    want = rp.select(poses, scores, points, 5, sep, syms)
    assert want[1].tolist() == [3] and (want[2] >= 0).all() and sorted(member[want[0][:3]]) == [0, 1, 2]
    rank = {int(c): r for r, c in enumerate(member[want[0][:3]])}
    assert want[2].tolist() == [rank[int(c)] for c in member]                  # every candidate belongs to its cluster's pick
    got = _abi(hiplib, poses, scores, points, 5, sep, syms)
    print(got[0].tolist(), got[1].tolist(), np.bincount(got[2]).tolist())
    assert _equal(got, want)
    # the Python entry hands the same arrays on: tensors or numpy, a [N,1] score column, no synchronisation of its own
    out = scoring.select_instances(poses, scores[:, None], points, 5, sep)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in out)
    assert _equal([t.cpu().numpy() for t in out], want)
    dev = torch.device("cuda", 0)
    out = scoring.select_instances(torch.from_numpy(poses).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(points),
                                   5, sep, symmetries=torch.from_numpy(syms), min_score=NINF)
    assert _equal([t.cpu().numpy() for t in out], want)
    # a bound on the score: the weakest pick's cluster is owned by nobody
    bound = float(np.sort(scores[want[0][:3]])[0]) + 1e-3
    want_b = rp.select(poses, scores, points, 5, sep, syms, bound)
    got_b = scoring.select_instances(poses, scores, points, 5, sep, min_score=bound)
    assert want_b[1].tolist() == [2] and _equal([t.cpu().numpy() for t in got_b], want_b)


def test_same_call_twice_is_byte_identical(hiplib):
    poses, scores, points, syms, _ = _frame(77, 300, 100, 6, 7, 0.04)
    a = _abi(hiplib, poses, scores, points, 9, 0.04, syms, min_score=0.75)
    b = _abi(hiplib, poses, scores, points, 9, 0.04, syms, min_score=0.75)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert _equal(a, rp.select(poses, scores, points, 9, 0.04, syms, 0.75)) and a[1][0] == 7


def test_nan_pose_is_picked_and_owns_only_itself(hiplib):
    poses = np.stack([pc.at(0.0), pc.at(0.01), pc.at(0.02), pc.at(0.5)])
    poses[1, 1, 2] = np.nan
    for scores, want_sel, want_owner in (([1, 3, 2, 0], [1, 2, 3, -1], [1, 0, 1, 2]), ([3, 1, 2, 0], [0, 1, 3, -1], [0, 1, 0, 2])):
        got = _abi(hiplib, poses, scores, pc.POINTS, 4, 0.1)
        assert got[0].tolist() == want_sel and got[2].tolist() == want_owner and got[1].tolist() == [3]
        assert _equal(got, rp.select(poses, scores, pc.POINTS, 4, 0.1))


def test_refusals_return_einval_and_write_nothing(hiplib):
    poses, scores, points, syms, _ = _frame(5, 20, 10, 2, 2, 0.04)
    ok = _abi(hiplib, poses, scores, points, 2, 0.04, syms)
    assert ok[1][0] == 2
    for kw in (dict(K=0), dict(K=65), dict(sep=-1e-9), dict(sep=float("inf")), dict(sep=float("nan")), dict(min_score=float("nan"))):
        args = dict(K=2, sep=0.04, min_score=NINF)
        args.update(kw)
        assert _abi(hiplib, poses, scores, points, args["K"], args["sep"], syms, args["min_score"], expect=-22) is None
    # sizes and pointers: the raw call, outputs prefilled
    dev = torch.device("cuda", 0)
    buf = torch.zeros(1 << 14, dtype=torch.float64, device=dev)
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=dev)
    p, q = buf.data_ptr(), out.data_ptr()
    args = (("poses", p), ("scores", p + 32768), ("N", 4), ("points", p + 65536), ("M", 8), ("syms", p + 98304), ("S", 1), ("K", 2),
            ("sep", 0.1), ("min_score", NINF), ("selected", q), ("count", q + 1024), ("owner", q + 2048), ("keys", q + 3072),
            ("s", hiplib.stream()))
    fn = hiplib.fn("ossid_pose_select")
    for kw in ({"N": 0}, {"N": -1}, {"N": 65537}, {"M": 0}, {"M": (1 << 22) + 1}, {"S": 0}, {"S": 4097}, {"K": -3}, {"poses": None},
               {"scores": None}, {"points": None}, {"syms": None}, {"selected": None}, {"count": None}, {"owner": None},
               {"keys": None}):
        assert fn(*[kw.get(k, d) for k, d in args]) == -22, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all()
    assert fn(*[d for _, d in args]) == 0
    torch.cuda.synchronize()
    res = out.cpu().numpy().view(np.int32)
    # four all-zero poses of score 0: candidate 0 is picked and owns all four, round 1 finds nobody
    assert res[:2].tolist() == [0, -1] and res[256] == 1 and res[512:516].tolist() == [0, 0, 0, 0]
