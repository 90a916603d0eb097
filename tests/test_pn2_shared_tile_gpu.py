"""GPU parity of the centre walk of the persistent SA kernels (csrc/pn2.hip, SPEC 4.5): a wave visits the large centres of
each group of 32 first, then pairs its small ones (at most 48 distinct samples: slot 48 of the ball row repeats slot 0) on
one shared tile. Nothing a kernel writes may change, so every stage is compared bit for bit with the CPU oracle -- at a grid
of 4 workgroups (ossid_pn2_set_persistent_grid), where a wave's slice is 288 centres in SA1 and 72 in SA2 and the group logic
runs at a test-sized batch, and at the default grid.

The inputs are built directly: planar xyz in [-1, 1]^2 with seeded features, the density varied per hypothesis --
  uniform      d around 20 in SA1 (every centre small), around 64 in SA2;
  disc         all 640 points inside one ball: every row full, more hits than slots;
  clumps       tight clumps of chosen sizes on a lattice wider than both radii, so a ball holds exactly its clump: d = the
               clump's size at BOTH levels, from isolated points (d = 1) through 48 and 49 to well past 64. (One clump is far
               tighter than the rest and larger than the 128 points the first sampling drops, so furthest-point sampling drops
               points from it alone and every other clump reaches SA2 whole.)
  sparse       clumps of at most 29 points and three isolated ones: every ball far short of 48 at both levels;
  gradient     density rising across the square: a spread of d.
Before anything is compared, the test replays the schedule in numpy on the ORACLE's ball lists and asserts that the cases it is
about occur (see _require_cases). A group of 32 never straddles a hypothesis in SA1 at 4 workgroups (slices of 288 = 9 x 32
start on multiples of 32, and so do hypotheses of 512), so the pair of two hypotheses is looked for in the walks of both grids
the test runs; every other case is required of the 4-workgroup walk alone."""
import numpy as np
import pytest
import torch

from test_oracle import _model

pytestmark = pytest.mark.gpu

B, M, NP1, NP2 = 9, 640, 512, 128
R1, R2 = 0.2, 0.4
SEED = 5
KINDS = ["uniform", "disc", "clumps", "uniform", "sparse", "clumps", "gradient", "clumps", "gradient"]
CLUMPS = [1, 1, 1, 2, 3, 7, 12, 16, 17, 20, 25, 32, 33, 40, 47, 48, 49, 50, 36]     # and one of 200: 640 points
SPARSE = [1, 1, 1] + [29] * 21 + [28]                                               # 640 points, no clump near 48
OSSID_EINVAL = -22      # include/ossid_hip.h
STAGES = ("ball1", "ball2", "feat1", "feat2", "feat3")


def _xy(kind, rng):
    if kind == "uniform":
        return rng.uniform(-1, 1, (M, 2))
    if kind == "disc":
        r, a = 0.09 * np.sqrt(rng.uniform(0, 1, M)), rng.uniform(0, 2 * np.pi, M)
        return rng.uniform(-0.5, 0.5, 2) + np.stack([r * np.cos(a), r * np.sin(a)], 1)
    if kind == "gradient":
        return np.stack([2 * rng.uniform(0, 1, M) ** 2.5 - 1, rng.uniform(-1, 1, M)], 1)
    sites = np.stack(np.meshgrid(np.arange(5), np.arange(5)), -1).reshape(25, 2) * 0.5 - 1.0     # lattice pitch 0.5 > R2
    sites = sites[rng.permutation(25)]
    if kind == "sparse":
        sizes, radii = list(rng.permutation(SPARSE)), [0.02] * len(SPARSE)
    else:
        sizes, radii = [200] + list(rng.permutation(CLUMPS)), [1e-3] + [0.02] * len(CLUMPS)
    assert sum(sizes) == M
    pts = []
    for s, n, rad in zip(sites, sizes, radii):
        r, a = rad * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
        pts.append(s + np.stack([r * np.cos(a), r * np.sin(a)], 1))
    return np.concatenate(pts)[rng.permutation(M)]


def _point_x(seed=SEED):
    rng = np.random.default_rng(seed)
    px = np.zeros((B, M, 8), np.float32)
    px[..., 3:] = rng.uniform(-1, 1, (B, M, 5)).astype(np.float32)
    for b, kind in enumerate(KINDS):
        px[b, :, :2] = _xy(kind, rng).astype(np.float32)
    return px


def _distinct(ball):
    s = np.sort(ball, axis=-1)
    return 1 + (s[..., 1:] != s[..., :-1]).sum(-1)


def _hits(xyz, centres, radius):
    """points of each set strictly inside each centre's ball (float64: only used to find rows with MORE hits than slots)"""
    d2 = ((centres[:, :, None, :].astype(np.float64) - xyz[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    return (d2 < radius * radius).sum(-1)


def _walk(ball, nwaves, npoint):
    """The schedule of SPEC 4.5 replayed on ball rows [total][64]: per group of 32 consecutive centres of a wave's slice, the
    large centres, the pairs of small ones, and the odd small one. Returns (groups, pairs)."""
    total = ball.shape[0]
    small = ball[:, 48] == ball[:, 0]
    per, rem = divmod(total, nwaves)
    groups, pairs = [], []
    for gw in range(nwaves):
        first = gw * per + min(gw, rem)
        end = first + per + (1 if gw < rem else 0)
        for g in range(first, end, 32):
            idx = np.arange(g, min(g + 32, end))
            sm = idx[small[idx]]
            groups.append((len(idx), len(sm)))
            pairs += [(a, b) for a, b in zip(sm[0::2], sm[1::2])]
    return groups, pairs


def _require_cases(px, wdbg, grids):
    xyz = px[..., :3]
    take = lambda src, idx: np.take_along_axis(src, idx[..., None].astype(np.int64), 1)
    xyz1 = take(xyz, wdbg["fps1"])
    xyz2 = take(xyz1, wdbg["fps2"])
    levels = (("sa1", wdbg["ball1"], _hits(xyz, xyz1, R1), NP1), ("sa2", wdbg["ball2"], _hits(xyz1, xyz2, R2), NP2))
    for name, ball, hits, npoint in levels:
        d = _distinct(ball)
        rows = ball.reshape(-1, 64)
        assert np.array_equal(rows[:, 48] == rows[:, 0], d.reshape(-1) <= 48), name     # what the kernels test IS d <= 48
        for lo, hi in ((1, 1), (2, 16), (17, 32), (33, 47), (48, 48), (49, 49)):
            assert ((d >= lo) & (d <= hi)).any(), (name, lo, hi)
        assert ((d == 64) & (hits > 64)).any(), name
        groups, _ = _walk(rows, 4 * grids[0], npoint)
        assert any(n == 32 and s == 0 for n, s in groups), name         # a group with no small centre
        assert any(n == 32 and s == 32 for n, s in groups), name        # a group of small centres only
        assert any(s % 2 == 1 and s > 1 for n, s in groups), name       # an odd number of them: pairs and one left over
        cross = [(a, b) for g in grids for a, b in _walk(rows, 4 * g, npoint)[1] if a // npoint != b // npoint]
        assert cross, name                                               # a pair whose centres belong to two hypotheses
        print("%s: d min %d mean %.1f, small %d of %d, pairs across hypotheses %s"
              % (name, d.min(), d.mean(), (d <= 48).sum(), d.size, cross[:3]))


def _set_grid(hiplib, workgroups):
    return hiplib.fn("ossid_pn2_set_persistent_grid")(workgroups)


@pytest.fixture(scope="module")
def case(ozr):
    """inputs, model and the oracle's result, computed once and left unchanged"""
    from ossid_code_amd.zephyr.pointnet2 import fold_pn2
    px = _point_x()
    m = _model(B)
    want, wdbg = ozr.pn2_score(px, fold_pn2(m), debug=True)
    # the packed weights, radii included, are made at a model's first score(): the small radius gets a model of its own
    tiny = dict(radius1=1e-6, radius2=1e-6)
    mt = _model(B)
    mt.SA_modules[0].radius, mt.SA_modules[1].radius = tiny["radius1"], tiny["radius2"]
    return dict(px=px, model=m, want=want, wdbg=wdbg, tiny_model=mt, wtiny=ozr.pn2_score(px, fold_pn2(mt), cfg=tiny, debug=True))


def _score(case, model="model"):
    got, dbg = case[model].cuda().score(torch.from_numpy(case["px"]).cuda(), debug=True)
    return got.cpu().numpy(), {k: dbg[k].cpu().numpy() for k in STAGES}


def test_every_stage_bit_exact(hiplib, case):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _require_cases(case["px"], case["wdbg"], (4, cus))
    try:
        for grid in (4, 0):
            assert _set_grid(hiplib, grid) == 0
            got, dbg = _score(case)
            for k in STAGES:
                assert dbg[k].shape == case["wdbg"][k].shape and np.array_equal(dbg[k], case["wdbg"][k]), (grid, k)
            assert np.array_equal(got, case["want"]), grid
    finally:
        _set_grid(hiplib, 0)


def test_duplicates_change_nothing(hiplib, case):
    """A radius below every distance: each row is one hit and 63 copies of it, every centre is small, every group pairs fully."""
    want, wdbg = case["wtiny"]
    assert (_distinct(wdbg["ball1"]) == 1).all() and (_distinct(wdbg["ball2"]) == 1).all()
    try:
        for grid in (4, 0):
            assert _set_grid(hiplib, grid) == 0
            got, dbg = _score(case, "tiny_model")
            for k in ("feat1", "feat2"):
                assert np.array_equal(dbg[k], wdbg[k]), (grid, k)
            assert np.array_equal(got, want), grid
    finally:
        _set_grid(hiplib, 0)


def test_setter_contract(hiplib, case):
    """0 and the CU count are the default grid; a negative size is refused and changes nothing."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    try:
        default, _ = _score(case)
        for grid in (0, cus):
            assert _set_grid(hiplib, grid) == 0
            assert np.array_equal(_score(case)[0], default), grid
        assert _set_grid(hiplib, 4) == 0
        assert _set_grid(hiplib, -1) == OSSID_EINVAL
        assert np.array_equal(_score(case)[0], default)
    finally:
        _set_grid(hiplib, 0)
