"""SPEC.md section 17 on the device: ossid_sym_grid / ossid_sym_score through the C ABI against the restatement
tests/ref_symmetry.py (brute-force neighbours) -- miss and sum_q are integers and worst_d2 is compared on its bits, so all
three must be EQUAL -- at the smallest shapes that can still go wrong, behind guard words, with every refusal; then
symmetry.find_symmetries at its defaults on meshes whose groups are derived by hand."""
import numpy as np
import pytest
import torch

import ref_icp
import ref_symmetry as rs
import symmetry_cases as sc
from guarded import EINVAL, OUT_FILL, Guarded, ready, run_contract, sync
from ossid_code_amd import bop_eval, render, symmetry

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _abi(hiplib, P, Q, T, tol, expect=0, grid_bytes=None, null=None, Nt=None, Mq=None, C=None):
    """One ossid_sym_grid and one ossid_sym_score over guarded buffers -> (miss, worst_d2, sum_q) numpy. On a refusal
    (expect = -22, of either entry) nothing at all may have been written."""
    ready()
    P, Q = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, 3)
    T = np.ascontiguousarray(T, dtype=np.float64).reshape(-1, 4, 4)
    Nt, Mq, C = len(P) if Nt is None else Nt, len(Q) if Mq is None else Mq, len(T) if C is None else C
    Pd, Qd, Td = (torch.from_numpy(a).cuda() for a in (P, Q, T))
    need = int(hiplib.fn("ossid_sym_grid_nbytes")(len(P)))
    assert need > 0
    grid = Guarded(need, 0x7F)
    nb = need if grid_bytes is None else grid_bytes
    out = {"miss": Guarded(4 * len(T), OUT_FILL), "worst_d2": Guarded(4 * len(T), OUT_FILL), "sum_q": Guarded(8 * len(T), OUT_FILL)}
    ptr = {"targets": Pd.data_ptr(), "grid": grid.ptr, "queries": Qd.data_ptr(), "transforms": Td.data_ptr(),
           **{k: g.ptr for k, g in out.items()}}
    if null is not None:
        ptr[null] = None
    rc = hiplib.fn("ossid_sym_grid")(ptr["targets"], Nt, tol, ptr["grid"], nb, hiplib.stream())
    if rc != 0:
        sync()
        assert bool((grid.payload == 0x7F).all()), "ossid_sym_grid refused, yet the grid buffer was written"
    else:
        rc = hiplib.fn("ossid_sym_score")(ptr["grid"], nb, Nt, ptr["queries"], Mq, ptr["transforms"], C, tol, ptr["miss"],
                                          ptr["worst_d2"], ptr["sum_q"], hiplib.stream())
    sync()
    assert rc == expect, rc
    assert grid.intact() and all(g.intact() for g in out.values())
    if expect != 0:
        assert all(bool((g.payload == OUT_FILL).all()) for g in out.values()), "refused, yet an output was written"
        return None
    return (out["miss"].view(torch.int32).cpu().numpy(), out["worst_d2"].view(torch.float32).cpu().numpy(),
            out["sum_q"].view(torch.int64).cpu().numpy())


def _equal(got, want):
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (got[1], want[1])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])


def _check(hiplib, P, Q, T, tol):
    want = rs.score_transforms(P, Q, T, tol)
    _equal(_abi(hiplib, P, Q, T, tol), want)
    return want


@pytest.mark.parametrize("Nt,Mq,C", [(500, 1, 3), (500, 63, 3), (500, 64, 3), (500, 257, 3), (1, 130, 4), (300, 70, 1),
                                     (4099, 300, 7)])
def test_kernels_equal_the_restatement(hiplib, Nt, Mq, C):
    P, Q, T, tol = sc.blob(Nt, Mq, C, seed=Nt + Mq)
    if Nt == 1:
        Q[::3] = P[0] + np.float32(0.01)                        # some hits on the only target
    miss, worst, sum_q = _check(hiplib, P, Q, T, tol)
    print("Nt %d Mq %d C %d: miss %s worst_d2 %s" % (Nt, Mq, C, miss.tolist(), worst.tolist()))
    assert 0 < miss.sum() < C * Mq or Mq == 1                   # hits and misses both occur


def test_wrapper_crosses_its_chunk(hiplib):
    """score_transforms launches ossid_sym_score once per SYM_MAX_TRANSFORMS transforms."""
    cap = hiplib.SYM_MAX_TRANSFORMS
    P, Q, T, tol = sc.blob(8, 3, 5, seed=1)
    rng = np.random.default_rng(2)
    big = np.tile(np.eye(4), (cap + 1, 1, 1))
    big[:, :3, 3] = rng.normal(scale=0.05, size=(cap + 1, 3))
    got = symmetry.score_transforms(P, Q, big, tol)
    assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32, torch.float32, torch.int64]
    want = rs.score_transforms(P, Q, big, tol)
    _equal([t.cpu().numpy() for t in got], want)
    assert 0 < want[0][cap:].sum() + want[0][:cap].sum() < 3 * (cap + 1)
    _abi(hiplib, P, Q, big, tol, expect=EINVAL)                 # the entry itself refuses more than its cap


def test_coordinates_near_flt_max(hiplib):
    """A box whose extent overflows f32 sizes to the one-cell grid (17.2: lo = 0, the probe is the brute force); a box near
    FLT_MAX with a finite extent grows its cells until they fit. Only a coincident point is within tol there."""
    perm = np.eye(4)[[1, 2, 0, 3]]                              # x -> y -> z -> x: exact
    for P in ([[-3e38, 0, 0], [3e38, 0, 0], [0, 3e38, -3e38], [FLT_MAX, FLT_MAX, FLT_MAX], [-FLT_MAX, 1.0, 2.0]],
              [[1e38, 1e38, 1e38], [3e38, 2e38, 1e38], [2e38, 3e38, 1.5e38], [1e38, 3e38, 3e38]]):
        P = np.asarray(P, dtype=np.float32)
        Q = np.concatenate([P, P[:, [2, 0, 1]], P * np.float32(0.5), [[0.0, 0.0, 0.0]]]).astype(np.float32)
        miss, worst, sum_q = _check(hiplib, P, Q, np.stack([np.eye(4), perm, perm @ perm]), 1.0)
        assert miss[0] <= len(Q) - len(P) and (worst == 0).all() and (sum_q == 0).all()


def test_the_tolerance_is_inclusive_and_ties_do_not_count_twice(hiplib):
    half, up = np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1.0))
    origin, I = np.zeros((1, 3), np.float32), np.eye(4)[None]
    on = _check(hiplib, origin, [[half, 0, 0]], I, 0.5)
    assert on[0][0] == 0 and on[1][0] == np.float32(0.25) and on[2][0] == 1 << 32          # d2 == tol^2: accepted, q = 2^32
    off = _check(hiplib, origin, [[up, 0, 0]], I, 0.5)
    assert off[0][0] == 1 and off[1][0] == 0 and off[2][0] == 0                             # the next float up: rejected
    # two targets equidistant from the query (and a duplicate of each): one hit, counted once
    P = np.array([[-1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 5, 0]], np.float32)
    tie = _check(hiplib, P, origin, I, 1.5)
    d2, idx = rs.nearest(origin, P, np.float32(1.5) * np.float32(1.5))
    assert idx[0] == 0 and d2[0] == 1.0                                                      # the lower index wins
    assert tie[0][0] == 0 and tie[1][0] == 1.0 and tie[2][0] == int(np.floor(1.0 / np.float64(np.float32(2.25)) * 2.0 ** 32))


def test_nan_misses_and_identical_targets(hiplib):
    P, Q, T, tol = sc.blob(200, 90, 4, seed=5)
    Q[7, 1] = np.nan
    Q[80] = np.nan
    T[1, 0, 2] = np.nan                                         # every query of transform 1 misses
    T[2, 3, :] = np.nan                                         # row 3 is not read
    T[3, 1, 3] = np.inf
    miss, _worst, _sum = _check(hiplib, P, Q, T, tol)
    assert miss[1] == 90 and miss[3] == 90 and 2 <= miss[0] < 90 and 2 <= miss[2] < 90
    same = np.tile(np.float32([0.25, -0.5, 0.125]), (300, 1))
    Q = (same[:70] + np.random.default_rng(0).normal(scale=0.05, size=(70, 3))).astype(np.float32)
    miss, _worst, _sum = _check(hiplib, same, Q, np.eye(4)[None], 0.08)
    assert 0 < miss[0] < 70


def test_guard_words_around_the_workspace(hiplib):
    for shape in sc.SHAPES:
        for contract in sc.build(hiplib, shape):
            sizes = run_contract(contract)
            print("CONTRACT %s %s" % (contract.name, sizes))


def test_refusals_launch_nothing(hiplib):
    P, Q, T, tol = sc.blob(40, 10, 3)
    assert hiplib.fn("ossid_sym_grid_nbytes")(0) == 0 and hiplib.fn("ossid_sym_grid_nbytes")(hiplib.SYM_MAX_TARGETS + 1) == 0
    assert hiplib.fn("ossid_sym_grid_nbytes")(-1) == 0 and hiplib.fn("ossid_sym_grid_nbytes")(hiplib.SYM_MAX_TARGETS) > 0
    for kw in ({"Nt": 0}, {"Nt": hiplib.SYM_MAX_TARGETS + 1}, {"Mq": 0}, {"Mq": hiplib.SYM_MAX_QUERIES + 1}, {"C": 0},
               {"C": hiplib.SYM_MAX_TRANSFORMS + 1}, {"null": "targets"}, {"null": "grid"}, {"null": "queries"},
               {"null": "transforms"}, {"null": "miss"}, {"null": "worst_d2"}, {"null": "sum_q"},
               {"grid_bytes": int(hiplib.fn("ossid_sym_grid_nbytes")(40)) - 1}, {"grid_bytes": 0}):
        _abi(hiplib, P, Q, T, tol, expect=EINVAL, **kw)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):      # tol, or its f32 square, not finite and positive
        _abi(hiplib, P, Q, T, bad, expect=EINVAL)
    with pytest.raises(ValueError):
        symmetry.score_transforms(P, Q, T, 0.0)


def test_score_refuses_on_its_own(hiplib):
    """ossid_sym_score's refusals that ossid_sym_grid shares, reached with a grid that was built: the entry alone is called
    with each bad Nt, tol, grid pointer and grid size; it returns OSSID_EINVAL and writes no output."""
    ready()
    P, Q, T, tol = sc.blob(40, 10, 3)
    Pd, Qd, Td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (P, Q, T))
    need = int(hiplib.fn("ossid_sym_grid_nbytes")(40))
    grid = Guarded(need + 16, 0x7F)                             # 16 spare bytes: the pointer off by 4 still has `need` behind it
    assert hiplib.fn("ossid_sym_grid")(Pd.data_ptr(), 40, tol, grid.ptr, need, hiplib.stream()) == 0
    sync()
    built = grid.payload.clone()

    def score(expect, Nt=40, tol=tol, ptr=grid.ptr, nbytes=need):
        out = {"miss": Guarded(12, OUT_FILL), "worst_d2": Guarded(12, OUT_FILL), "sum_q": Guarded(24, OUT_FILL)}
        rc = hiplib.fn("ossid_sym_score")(ptr, nbytes, Nt, Qd.data_ptr(), 10, Td.data_ptr(), 3, tol, out["miss"].ptr,
                                          out["worst_d2"].ptr, out["sum_q"].ptr, hiplib.stream())
        sync()
        assert rc == expect, (rc, Nt, tol, nbytes)
        assert all(g.intact() for g in out.values()) and grid.intact() and torch.equal(grid.payload, built)
        if expect != 0:
            assert all(bool((g.payload == OUT_FILL).all()) for g in out.values()), "refused, yet an output was written"
        return out
    good = score(0)
    _equal((good["miss"].view(torch.int32).cpu().numpy(), good["worst_d2"].view(torch.float32).cpu().numpy(),
            good["sum_q"].view(torch.int64).cpu().numpy()), rs.score_transforms(P, Q, T, tol))
    for kw in ({"Nt": 0}, {"Nt": -1}, {"Nt": hiplib.SYM_MAX_TARGETS + 1}, {"ptr": None}, {"nbytes": need - 1}, {"nbytes": 0},
               {"ptr": grid.ptr + 4}, {"ptr": grid.ptr + 8}):
        score(EINVAL, **kw)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e30):
        score(EINVAL, tol=bad)
    # a grid built for another Nt or another tol is not followed: every query misses, nothing outside the buffer is read
    for kw in ({"Nt": 39}, {"tol": 2.0 * tol}, {"tol": 0.5 * tol}):
        out = score(0, **kw)
        assert out["miss"].view(torch.int32).cpu().tolist() == [10, 10, 10]
        assert not out["worst_d2"].view(torch.float32).cpu().any() and not out["sum_q"].view(torch.int64).cpu().any()


def test_a_grid_of_garbage_is_not_followed(hiplib):
    """Buffers the grid entry never wrote -- 0x00, 0x7F, 0xFF -- are scored without a fault: every query misses."""
    ready()
    P, Q, T, tol = sc.blob(40, 10, 3)
    Qd, Td = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (Q, T))
    need = int(hiplib.fn("ossid_sym_grid_nbytes")(40))
    for fill in (0x00, 0x7F, 0xFF):
        grid = Guarded(need, fill)
        out = {"miss": Guarded(12, OUT_FILL), "worst_d2": Guarded(12, OUT_FILL), "sum_q": Guarded(24, OUT_FILL)}
        rc = hiplib.fn("ossid_sym_score")(grid.ptr, need, 40, Qd.data_ptr(), 10, Td.data_ptr(), 3, tol, out["miss"].ptr,
                                          out["worst_d2"].ptr, out["sum_q"].ptr, hiplib.stream())
        sync()
        assert rc == 0 and grid.intact() and all(g.intact() for g in out.values())
        assert out["miss"].view(torch.int32).cpu().tolist() == [10, 10, 10]


# ---- find_symmetries at its defaults -------------------------------------------------------------------------------------------
def _mesh(V, F):
    V = np.asarray(V, dtype=np.float64)
    return render.Mesh(V, np.asarray(F, dtype=np.int32), colors=np.full((len(V), 3), 160, np.uint8))


def _prism_mesh(ring, height):
    """A right prism over the polygon `ring` [n,2] (counter-clockwise), z in [-height / 2, height / 2]."""
    n = len(ring)
    V = [[x, y, -height / 2] for x, y in ring] + [[x, y, height / 2] for x, y in ring] + [[0, 0, -height / 2], [0, 0, height / 2]]
    F = []
    for i in range(n):
        j = (i + 1) % n
        F += [[i, j, n + j], [i, n + j, n + i], [2 * n, j, i], [2 * n + 1, n + i, n + j]]
    return _mesh(V, F)


def _lathe_mesh(profile, segments=96):
    prof = np.asarray(profile, dtype=np.float64)
    th = 2.0 * np.pi * np.arange(segments) / segments
    V = np.concatenate([np.stack([r * np.cos(th), r * np.sin(th), np.full(segments, z)], 1) for r, z in prof])
    F = []
    for k in range(len(prof) - 1):
        for i in range(segments):
            a, b, c, d = k * segments + i, k * segments + (i + 1) % segments, (k + 1) * segments + i, (k + 1) * segments + (i + 1) % segments
            F += [[a, b, d], [a, d, c]]
    return _mesh(V, F)                                          # the rings at r = 0 give faces without area: they weigh nothing


def _icosphere(level):
    """(unit vertices [10 * 4^level + 2, 3], faces): the icosahedron, each face split in four `level` times."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    V = [np.array(v, dtype=np.float64) / np.sqrt(1.0 + g * g) for v in
         ((-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
          (-g, 0, -1), (-g, 0, 1))]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nxt = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = V[i] + V[j]
                V.append(p / np.sqrt(p @ p))
                mid[key] = len(V) - 1
            return mid[key]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = nxt
    return np.stack(V), np.array(F, dtype=np.int32)


def _bumped_ellipsoid_mesh(level=5):
    """tests/ref_icp.py's ellipsoid with its bump as a radial mesh: every icosphere direction at the farther of its exits
    from the ellipsoid and from the bump's sphere."""
    d, F = _icosphere(level)
    te = 1.0 / np.sqrt(((d / ref_icp.AXES) ** 2).sum(1))
    b = d @ ref_icp.BUMP_C
    disc = b * b - (ref_icp.BUMP_C @ ref_icp.BUMP_C - ref_icp.BUMP_R ** 2)
    tb = np.where(disc > 0.0, b + np.sqrt(np.maximum(disc, 0.0)), 0.0)
    return _mesh(d * np.maximum(te, tb)[:, None], F)


S2 = np.sqrt(0.5)
MESHES = {
    "box": (lambda: _prism_mesh(np.array([[0.5, 0.3], [-0.5, 0.3], [-0.5, -0.3], [0.5, -0.3]]), 0.3), 3, 0),
    "square_prism": (lambda: _prism_mesh(0.5 * np.array([[1, 0], [0, 1], [-1, 0], [0, -1]]), 0.4), 7, 0),
    "lathe": (lambda: _lathe_mesh(rs.LATHE_PROFILE), 0, 1),
    # borderline by construction (SPEC 17.6): 0.048 - 0.050 d symmetric under tilted half-turns; the issue's asymmetric object
    "ellipsoid_with_bump": (lambda: _bumped_ellipsoid_mesh(), 0, 0),
    # asymmetric with a margin: a tetrahedron whose six edges all differ (0.73, 0.75, 0.78, 0.90, 1.00, 1.06)
    "scalene_tetrahedron": (lambda: _mesh([[0, 0, 0], [1, 0, 0], [0.2, 0.7, 0], [0.4, 0.3, 0.6]],
                                          [[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]), 0, 0),
}


@pytest.mark.parametrize("name", list(MESHES))
def test_find_symmetries_at_its_defaults(hiplib, name):
    make, n_disc, n_cont = MESHES[name]
    ready()
    mesh = make()
    out, info = symmetry.find_symmetries(mesh, return_info=True)
    sync()
    print("%s: d %.4g tol %.4g scored %d -> %d discrete, %d continuous; clusters %s"
          % (name, info["diameter"], info["tol"], info["n_scored"], len(out["symmetries_discrete"]), len(out["symmetries_continuous"]),
             [(np.round(c["axis"], 3).tolist(), sorted(c["members"]), c["continuous"]) for c in info["clusters"]]))
    assert len(out["symmetries_discrete"]) == n_disc and len(out["symmetries_continuous"]) == n_cont
    if not symmetry.has_symmetry(out):
        return
    # a pose times a symmetry is the same pose to MSSD (SPEC 8.7) once the evaluation is given what was found
    S = bop_eval.symmetry_transformations(out)
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = ref_icp.rot([0.3, -1.0, 0.5], 40.0), [0.05, -0.1, 3.0]
    moved = [np.asarray(m).reshape(4, 4) for m in out["symmetries_discrete"]] + \
        [symmetry.rotation_about(c["axis"], 1.234, c["offset"]) for c in out["symmetries_continuous"]]
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    est = np.stack([pose @ M for M in moved])
    mssd, _mspd = bop_eval.mssd_mspd(mesh, S, est, np.tile(pose, (len(est), 1, 1)), K)
    plain, _ = bop_eval.mssd_mspd(mesh, np.eye(4)[None], est, np.tile(pose, (len(est), 1, 1)), K)
    print("   MSSD with the symmetries %s, without %s (tol %.4g)" % (mssd.tolist(), plain.tolist(), info["tol"]))
    assert (mssd <= info["tol"]).all() and (plain > info["tol"]).all()


def test_stream_finds_symmetries_on_first_use(hiplib):
    """OnlineStream(symmetries="auto", meshes=...): an object's transformations are found once from its mesh, in 8.6's form,
    and it is scored with ADI; an object without a mesh, or without a symmetry, has none and keeps `symmetric`."""
    from ossid_code_amd.stream import OnlineStream
    ready()
    box = MESHES["box"][0]()
    stream = OnlineStream(None, None, None, meshes={1: box, 3: MESHES["ellipsoid_with_bump"][0]()}, symmetries="auto")
    S = stream._symmetries(1)
    sync()
    assert S.shape == (4, 4, 4) and np.array_equal(S[0], np.eye(4)) and stream._symmetries(1) is S
    assert stream._symmetric({"obj_id": 1}) is True
    assert stream._symmetries(2) is None and stream._symmetric({"obj_id": 2}) is False
    assert stream._symmetries(3) is None and stream._symmetric({"obj_id": 3}) is False
