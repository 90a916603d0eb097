"""GPU parity of the two sampling kernels (pytest -m gpu): furthest-point sampling and ball query through the C ABI of
libossid_hip.so against the CPU oracle, bit for bit (np.array_equal on integer indices and float centres). The cases sit at
the edges of the register-resident forms -- every points-per-lane count of fps_reg_kernel, every chunk count of
ball_query_reg_kernel, the LDS fallbacks above 3072 points -- and build the situations in which an arg-max without an index,
a sentinel, a tie rule or a count that crosses 64 could go wrong. Each case first asserts ON THE ORACLE'S OUTPUT that its
situation occurs, so that none passes vacuously. B = 3 throughout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 3


def _fps(hiplib, xyz, npoint):
    b, n, stride = xyz.shape
    dx = torch.from_numpy(xyz).cuda()
    idx = torch.full((b, npoint), -7, dtype=torch.int32, device="cuda")
    cen = torch.full((b, npoint, 3), np.nan, dtype=torch.float32, device="cuda")
    rc = hiplib.fn("ossid_pn2_fps")(dx.data_ptr(), stride, b, n, npoint, idx.data_ptr(), cen.data_ptr(), hiplib.stream())
    assert rc == 0
    return idx.cpu().numpy(), cen.cpu().numpy()


def _ball(hiplib, xyz, cen, radius):
    b, n, stride = xyz.shape
    npoint = cen.shape[1]
    dx = torch.from_numpy(xyz).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(cen, np.float32)).cuda()
    out = torch.full((b, npoint, 64), -7, dtype=torch.int32, device="cuda")
    rc = hiplib.fn("ossid_pn2_ball_query")(dx.data_ptr(), stride, b, n, dc.data_ptr(), npoint, radius, 64, out.data_ptr(),
                                           hiplib.stream())
    assert rc == 0
    return out.cpu().numpy()


def _check_fps(hiplib, ozr, xyz, npoint):
    want = ozr.fps(xyz, npoint)
    got, cen = _fps(hiplib, xyz, npoint)
    assert np.array_equal(got, want)
    assert np.array_equal(cen, np.take_along_axis(xyz[..., :3], want[..., None].astype(np.int64), 1))
    return want


# ---- furthest point sampling ---------------------------------------------------------------------------------------

# n at the edges of every per-lane count (2 / 4 / 8 / 12 points per lane of 256) and of the LDS fallback (3073)
FPS_SIZES = [33, 64, 65, 511, 512, 513, 1025, 2047, 2048, 2049, 3072, 3073]


@pytest.mark.parametrize("n", FPS_SIZES)
def test_fps_sizes_planar_single_z_and_general(hiplib, ozr, n):
    """Set 0 is planar (the fast path), set 1 is planar but for ONE point's z (the workgroup-wide OR must select the general
    path: that point is then the second pick, which it is not once its z is dropped), set 2 has z everywhere."""
    stride = 3 if n % 2 else 8
    rng = np.random.default_rng(1000 + n)
    xyz = np.zeros((B, n, stride), np.float32)
    xyz[..., :2] = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    lone = n - 2
    xyz[1, lone, 2] = 5.0
    xyz[2, :, 2] = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    for npoint in ([32, n] if n <= 65 else [32]):
        want = _check_fps(hiplib, ozr, xyz, npoint)
        flat = xyz.copy()
        flat[1, lone, 2] = 0.0
        assert want[1, 1] == lone and ozr.fps(flat, npoint)[1, 1] != lone
        assert (want[0] != want[2]).any()


@pytest.mark.parametrize("n", [130, 2048, 3073])
def test_fps_nothing_selectable_keeps_index_zero(hiplib, ozr, n):
    rng = np.random.default_rng(n)
    xyz = np.zeros((B, n, 8), np.float32)
    xyz[..., :2] = rng.uniform(-0.02, 0.02, (B, n, 2)).astype(np.float32)     # |p|^2 <= 8e-4 < 1e-3 everywhere
    xyz[1, :, 2] = rng.uniform(-0.01, 0.01, n).astype(np.float32)
    assert ((xyz[..., :3].astype(np.float64) ** 2).sum(-1) < 1e-3).all()
    want = _check_fps(hiplib, ozr, xyz, 32)
    assert (want == 0).all()


@pytest.mark.parametrize("n", [65, 513, 2048, 3072])
def test_fps_only_the_last_point_is_live(hiplib, ozr, n):
    rng = np.random.default_rng(n)
    xyz = np.zeros((B, n, 3), np.float32)
    xyz[..., :2] = rng.uniform(-0.02, 0.02, (B, n, 2)).astype(np.float32)
    xyz[:, n - 1, :2] = (0.5, -0.5)
    xyz[2, n - 1, 2] = 0.25
    want = _check_fps(hiplib, ozr, xyz, 32)
    assert (want[:, 0] == 0).all() and (want[:, 1:] == n - 1).all()


@pytest.mark.parametrize("n", [300, 2048])
def test_fps_fewer_live_points_than_picks(hiplib, ozr, n):
    """Once every live point has been picked all running distances are exact zeros: the tie goes to the lowest LIVE index."""
    rng = np.random.default_rng(n)
    live = np.array([7, 100, 130, 250, n - 1])
    xyz = np.zeros((B, n, 8), np.float32)
    xyz[..., :2] = rng.uniform(-0.02, 0.02, (B, n, 2)).astype(np.float32)
    xyz[:, live, :2] = rng.uniform(0.3, 1.0, (B, len(live), 2)).astype(np.float32)
    xyz[1, live, 2] = rng.uniform(0.1, 0.3, len(live)).astype(np.float32)
    want = _check_fps(hiplib, ozr, xyz, 32)
    for b in range(B):
        assert set(want[b, 1:1 + len(live)]) == set(live)
        assert (want[b, 1 + len(live):] == 7).all()


@pytest.mark.parametrize("npoint", [3072, 3073])
def test_fps_more_picks_than_points(hiplib, ozr, npoint):
    """The register form lists its picks in LDS, 3072 at the most; one more pick takes the LDS form. Both go on picking after
    the 300 points are exhausted (exact-zero ties: the lowest live index, over and over)."""
    n = 300
    rng = np.random.default_rng(npoint)
    xyz = np.zeros((B, n, 3), np.float32)
    xyz[..., :2] = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    xyz[1, :, 2] = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    xyz[2, :3, :2] = 0.01                                        # the three lowest indices are dead in set 2
    want = _check_fps(hiplib, ozr, xyz, npoint)
    assert (want[:2, n:] == 0).all() and (want[2, n:] == 3).all()


@pytest.mark.parametrize("n", [130, 2048])
def test_fps_lattice_in_shuffled_index_order(hiplib, ozr, n):
    side = int(np.ceil(np.sqrt(n)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float32)
    lat = g / side * 2 - 0.97
    xyz = np.zeros((B, n, 8), np.float32)
    xyz[0, :, :2] = lat
    for b in (1, 2):
        xyz[b, :, :2] = lat[np.random.default_rng(b).permutation(n)]
    npoint = min(n, 128)
    want = _check_fps(hiplib, ozr, xyz, npoint)
    for b in range(B):   # ties really occur: a third of the distances from the first pick repeat an earlier one exactly
        d0 = ((xyz[b, :, :2] - xyz[b, 0, :2]) ** 2).sum(1)
        assert n - len(np.unique(d0)) >= n // 3
    assert (want[1] != want[2]).any()


def test_fps_equal_maxima_in_one_lane_and_in_two_waves(hiplib, ozr):
    """n = 2048: lane t owns [8t, 8t + 8), wave w owns [512w, 512w + 512). Two exactly equal maxima must resolve to the lower
    index whether they sit inside one lane's eight points (set 0), in two waves as identical points (set 1), or in two waves
    as mirror images with the higher index listed nearer the front of its wave (set 2)."""
    n = 2048
    rng = np.random.default_rng(8)
    xyz = np.zeros((B, n, 8), np.float32)
    xyz[..., :2] = (0.5 + rng.uniform(-0.05, 0.05, (B, n, 2))).astype(np.float32)
    xyz[:, 0, :2] = (0.5, 0.5)
    pairs = [(8 * 37 + 2, 8 * 37 + 5), (700, 1500), (700, 1536)]
    xyz[0, pairs[0], :2] = (-0.9, -0.9)
    xyz[1, pairs[1], :2] = (-0.9, -0.9)
    xyz[2, pairs[2][0], :2] = (0.25, 0.5)       # 0.25 - 0.5 and 0.75 - 0.5 are exact and of equal square
    xyz[2, pairs[2][1], :2] = (0.75, 0.5)
    for b, (lo, hi) in enumerate(pairs):
        d = ((xyz[b, :, :2] - xyz[b, 0, :2]) ** 2).sum(1, dtype=np.float32)
        assert d[lo] == d[hi] == d.max() and (d == d.max()).sum() == 2
    want = _check_fps(hiplib, ozr, xyz, 32)
    assert [want[b, 1] for b in range(B)] == [p[0] for p in pairs]


# ---- ball query ----------------------------------------------------------------------------------------------------

# n at the edges of the chunk counts (8 / 16 / 32 / 48 chunks of 64) and one size over the register form's 3072
BALL_SIZES = [40, 64, 65, 512, 777, 2048, 3000, 3100]
FAR = (50.0, 50.0, 0.0)


@pytest.mark.parametrize("n", BALL_SIZES)
def test_ball_sizes_radii_and_foreign_centres(hiplib, ozr, n):
    """37 centres (no multiple of the waves per workgroup): 32 from the oracle's FPS and five that are no members of the set,
    one of them far outside (its row is all 0). Set 0 is planar, set 1 is not, set 2 is planar with one foreign centre OFF the
    plane, which must select the general path."""
    stride = 3 if n % 2 else 8
    rng = np.random.default_rng(2000 + n)
    xyz = np.zeros((B, n, stride), np.float32)
    xyz[..., :2] = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    xyz[1, :, 2] = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    fidx = ozr.fps(xyz, 32)
    cen = np.zeros((B, 37, 3), np.float32)
    cen[:, :32] = np.take_along_axis(xyz[..., :3], fidx[..., None].astype(np.int64), 1)
    cen[:, 32:36, :2] = rng.uniform(-1, 1, (B, 4, 2)).astype(np.float32)
    cen[:, 36] = FAR
    cen[2, 33] = (0.1, -0.1, 0.3)
    for radius in (0.05, 0.2, 0.4, 1e-4):
        want = ozr.ball_query(xyz, cen, radius, 64)
        assert (want[:, 36] == 0).all()
        if radius == 1e-4:    # only the centre itself: 64 copies of its own index
            assert np.array_equal(want[:, :32], np.repeat(fidx[..., None], 64, 2))
        if radius == 0.4 and n >= 512:     # the off-plane centre sees a smaller disc than its shadow on the plane
            shadow = cen.copy()
            shadow[2, 33, 2] = 0.0
            assert not np.array_equal(ozr.ball_query(xyz, shadow, radius, 64)[2, 33], want[2, 33])
        if radius == 0.4 and n >= 512:     # full rows occur: the early exit is taken
            assert any(len(np.unique(row)) == 64 for row in want[0])
        assert np.array_equal(_ball(hiplib, xyz, cen, radius), want)


def test_ball_more_centres_than_one_workgroup_covers(hiplib, ozr):
    """300 centres: a second workgroup per set (256 centres each in the register form) with 44 centres, no multiple of its
    eight waves."""
    n, npoint = 777, 300
    rng = np.random.default_rng(300)
    xyz = np.zeros((B, n, 8), np.float32)
    xyz[..., :2] = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    xyz[1, :, 2] = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    fidx = ozr.fps(xyz, npoint)
    cen = np.take_along_axis(xyz[..., :3], fidx[..., None].astype(np.int64), 1)
    want = ozr.ball_query(xyz, cen, 0.2, 64)
    assert (want[:, 256:, 0] != want[:, :44, 0]).any()
    assert np.array_equal(_ball(hiplib, xyz, cen, 0.2), want)


def _cluster_scene(n, with_z):
    """Background in [-1, 1]^2 and clusters far from it and from each other, each probing one way of counting to 64."""
    rng = np.random.default_rng(n + int(with_z))
    xyz = np.zeros((n, 8), np.float32)
    xyz[:, :2] = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    if with_z:
        xyz[:, 2] = rng.uniform(-0.2, 0.2, n).astype(np.float32)

    def put(lo, count, at, jitter):
        xyz[lo:lo + count, :2] = np.float32(at) + rng.uniform(-jitter, jitter, (count, 2)).astype(np.float32)
        if with_z:
            xyz[lo:lo + count, 2] = rng.uniform(-jitter, jitter, count).astype(np.float32)
        return (at[0], at[1], 0.0)

    cen = [put(0, 80, (3.0, 3.0), 0.0),          # A: 80 identical points at 0..79, the first chunk alone fills the row
           put(300, 100, (5.0, 3.0), 0.01),      # B: 20 hits in chunk 4, the count crosses 64 in the middle of chunk 5
           put(1000, 64, (7.0, 3.0), 0.01),      # C: exactly 64 hits, over chunks 15 and 16
           put(1500, 10, (9.0, 3.0), 0.01),      # D: 10 hits, the first of them in chunk 23: padding is 1500
           (2.0, 6.0, 0.0),                      # E: a point at distance exactly r (missed) and one just inside
           FAR]
    xyz[1700, :3] = (2.25, 6.0, 0.0)             # 2.0 - 2.25 = -0.25 exactly; radius 0.25: d2 == r2, strict < misses
    xyz[1701, :3] = (2.0, 6.2499, 0.0)
    return xyz, np.array(cen, np.float32)


def test_ball_counting_to_64(hiplib, ozr):
    n, radius = 2048, 0.25
    scenes = [_cluster_scene(n, False), _cluster_scene(n, True), _cluster_scene(n, False)]
    xyz = np.stack([s[0] for s in scenes])
    cen = np.stack([s[1] for s in scenes])
    perm = np.random.default_rng(3).permutation(np.arange(400, 1000))     # set 2: another background order
    xyz[2, 400:1000] = xyz[2, perm]
    want = ozr.ball_query(xyz, cen, radius, 64)
    for b in range(B):
        assert np.array_equal(want[b, 0], np.arange(64))
        assert np.array_equal(want[b, 1], np.arange(300, 364))
        assert np.array_equal(want[b, 2], np.arange(1000, 1064))
        assert np.array_equal(want[b, 3], np.r_[np.arange(1500, 1510), np.full(54, 1500)])
        assert (want[b, 4] == 1701).all()                                  # 1700 sits at exactly r and is missed
        assert (want[b, 5] == 0).all()
    assert np.float32(2.0) - np.float32(2.25) == np.float32(-0.25) and np.float32(radius) ** 2 == np.float32(0.0625)
    assert np.array_equal(_ball(hiplib, xyz, cen, radius), want)


def test_ball_only_hit_in_the_last_partial_chunk(hiplib, ozr):
    """n = 777 = 12 chunks and 9 points: the one hit is index 776, the last lane in use of the last chunk; the lanes past it
    hold padding, which is inside no ball."""
    n = 777
    rng = np.random.default_rng(777)
    xyz = np.zeros((B, n, 3), np.float32)
    xyz[..., :2] = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    xyz[1, :, 2] = rng.uniform(-0.2, 0.2, n).astype(np.float32)
    xyz[:, 776] = (4.0, 4.0, 0.0)
    cen = np.zeros((B, 3, 3), np.float32)
    cen[:, 0] = (4.0, 4.0, 0.0)
    cen[:, 1] = (4.05, 4.0, 0.0)
    cen[:, 2] = (0.0, 0.0, 0.0)       # in the plane, so that sets 0 and 2 stay on the planar path; any radius reaches it
    want = ozr.ball_query(xyz, cen, 0.1, 64)
    assert (want[:, :2] == 776).all() and (want[:, 2] != 776).all()
    assert np.array_equal(_ball(hiplib, xyz, cen, 0.1), want)
