"""Inputs of the Zephyr featurizer's edge tests, built once and shared by the CPU tests (oracle against the float32 and
float64 restatements, tests/test_featurize_edges.py) and the GPU tests (kernels against all three,
tests/test_featurize_edges_gpu.py), in the manner of tests/pipeline_cases.py, whose frame, camera and exact-coordinate
helpers are reused. Every value that decides a comparison is exactly representable in float32, so the float32 kernels /
oracle and the float64 restatement must take the same decisions: a disagreement is a wrong convention, never rounding.
Each builder asserts its own premise on the float32 restatement's output (tests/ref_featurize.py), so that no case passes
vacuously: if a builder's inputs stop producing the edge it is named after, building the case fails.

A case is a dict: name, rgb f32 [H,W,3], depth f32 [H,W], K, T f32 [N,4,4], pts / nrm / col f32 [M,3], margins (tuple),
sels (list of hypothesis selections; None = all hypotheses in order)."""
import functools

import numpy as np

import ref_featurize as rf
from pipeline_cases import EH, EW, EYE, K_EDGE, Z_MIN32, Z_NEXT32, coord, point, proj_case_near

f32 = np.float32
M002 = f32(0.02)                                             # the filter's margin as the C ABI carries it

# Cases that cannot be built so that float32 and float64 decide alike, dropped from the float64 leg BY NAME (never masked
# at run time). They stay in the bit-equality leg (oracle == float32 restatement == kernel).
#   hsv_near_grey_taps: interpolated colours with max - min of a few ulps: the hue branch is decided by rounding.
NOT_IN_F64 = ("hsv_near_grey_taps",)


# (x / 100) * 100 does not return x for every quarter-pixel coordinate, so K_EDGE with z = 100 is exact only for the
# values pipeline_cases.coord asserts. Where a case needs arbitrary quarter-pixel coordinates (bilinear weights, pixel
# centres, shifted hypotheses) it uses a power-of-two camera: (x / 128) * 128 is exact for every float, in both precisions.
Z2 = 128.0
K_P2 = np.array([[128.0, 0.0, 0.0], [0.0, 128.0, 0.0], [0.0, 0.0, 1.0]])


def p2(u, v, z=Z2):
    """the point that K_P2 projects onto exactly (u, v), u and v on a 1/8 grid"""
    p = [f32(u * z / 128.0), f32(v * z / 128.0), f32(z)]
    assert float(p[0]) * 128.0 / z == u and float(p[1]) * 128.0 / z == v
    return p


def frame(H, W, seed, z=100.0):
    """colours on a 1/256 grid with r > g > b by at least 0.1 (a bilinear mix with quarter weights is exact and keeps
    max - min >= 0.45, so its hue is well conditioned), depths z + k/64 (exact; D - z is exact)"""
    rng = np.random.default_rng(seed + 1000 * H + W)
    rgb = np.stack([rng.integers(180, 257, (H, W)), rng.integers(90, 154, (H, W)), rng.integers(0, 64, (H, W))], -1)
    depth = z + rng.integers(-64, 65, (H, W)) / 64.0
    return (rgb / 256.0).astype(f32), depth.astype(f32)


def colours(M, seed=1):
    """model colours on a 1/256 grid, all six orders of the channels"""
    return (np.random.default_rng(seed).integers(0, 257, (M, 3)) / 256.0).astype(f32)


def normals(M, seed=2):
    n = np.random.default_rng(seed).normal(size=(M, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)


def _case(name, rgb, depth, pts, T=None, nrm=None, col=None, K=K_EDGE, margins=(0.02,), sels=(None,)):
    pts = np.asarray(pts, f32).reshape(-1, 3)
    M = len(pts)
    T = np.asarray(EYE[None] if T is None else T, f32).reshape(-1, 4, 4)
    nrm = np.tile(f32([0, 0, -1]), (M, 1)) if nrm is None else np.asarray(nrm, f32)
    col = colours(M) if col is None else np.asarray(col, f32)
    return dict(name=name, rgb=np.ascontiguousarray(rgb, f32), depth=np.ascontiguousarray(depth, f32), K=K,
                T=np.ascontiguousarray(T), pts=pts, nrm=nrm, col=col, margins=tuple(margins), sels=list(sels))


def ref(c, interp, margin=0.02, sel=None, dtype=f32):
    """the restatement's full output for a case"""
    return rf.featurize_full(rf.pack_rgbd(c["rgb"], c["depth"]), c["T"], c["pts"], c["nrm"], c["col"], c["K"],
                             interp=interp, margin=margin, sel=sel, dtype=dtype)


# ---- borders -----------------------------------------------------------------------------------------------------------
U_BORDER = [-1.0, -0.5, 0.0, 0.5, EW - 1.0, EW - 0.5, float(EW), EW + 0.5]
V_BORDER = [-1.0, -0.5, 0.0, 0.5, EH - 1.0, EH - 0.5, float(EH), EH + 0.5]


def borders():
    uv = [(u, v) for v in V_BORDER for u in U_BORDER]
    rgb, depth = frame(EH, EW, 1)
    c = _case("borders", rgb, depth, [point(u, v) for u, v in uv])
    for interp in (0, 1):
        r = ref(c, interp)
        got_uv, inb = r["uv"][0], r["inb"][0]
        for i, (u, v) in enumerate(uv):
            assert got_uv[i].tolist() == [int(u), int(v)], (u, v)          # uv_original = trunc, in frame or not
            assert inb[i] == (-1 < u < EW and -1 < v < EH), (u, v)          # (-1, 0) truncates to 0: in frame
        i = uv.index((-0.5, 0.5))
        assert got_uv[i].tolist() == [0, 0] and inb[i] and not inb[uv.index((-1.0, 0.5))]
        out = ~inb
        assert out.sum() == 64 - 25 and (r["uc"][0][out] == 0).all() and (r["vc"][0][out] == 0).all()
        assert (r["point_x"][0][out, 6] == depth[0, 0] - f32(100)).all() and depth[0, 0] != 100     # ... read pixel (0,0)
        # ... and enter mean and extent as pixel (0,0): the mean over all 64, the out-of-frame ones as zeros
        su = sum(int(u) for u, v in uv if -1 < u < EW and -1 < v < EH)
        sv = sum(int(v) for u, v in uv if -1 < u < EW and -1 < v < EH)
        assert r["mean"][0].tolist() == [f32(su) / f32(64), f32(sv) / f32(64)]
        assert (r["point_x"][0][out, 0] == (f32(0) - r["mean"][0, 0]) / r["extent"][0]).all()
    return c


# ---- bilinear taps -----------------------------------------------------------------------------------------------------
FRACS = [0.0, 0.25, 0.5, 0.75]


def _tap_case(name, H, W, cols, rows, seed):
    us = [c + f for c in cols for f in FRACS]
    vs = [r + f for r in rows for f in FRACS]
    uv = [(u, v) for v in vs for u in us]
    rgb, depth = frame(H, W, seed, Z2)
    c = _case(name, rgb, depth, [p2(u, v) for u, v in uv], K=K_P2)
    r = ref(c, 1)
    assert r["bil"].all() and not r["fallback"].any()
    for i, (u, v) in enumerate(uv):
        k, fr = int(u), u - int(u)
        assert r["wx"][0, i] == {0.0: 0.5, 0.25: 0.75, 0.5: 0.0, 0.75: 0.25}[fr]        # u_f = k + 0.5: weight 0; u_f = k: 0.5
        lo = k if fr >= 0.5 else k - 1                                                   # floor(u_f - 0.5)
        assert r["taps"][0, i, :2].tolist() == [min(max(lo, 0), W - 1), min(max(lo + 1, 0), W - 1)], (u, v)
    return c


def bilinear_taps():
    out = [_tap_case("taps_edge_frame", EH, EW, [0, 1, 20, EW - 2, EW - 1], [0, 1, 12, EH - 2, EH - 1], 2)]
    r = ref(out[0], 1)
    last = len(out[0]["pts"]) - 1                                                       # (W - 0.25, H - 0.25)
    assert r["taps"][0, last].tolist() == [EW - 1, EW - 1, EH - 1, EH - 1]              # the bottom-right corner clamps
    assert r["taps"][0, 0].tolist() == [0, 0, 0, 0]                                     # (0, 0): both taps clamp to 0
    out.append(_tap_case("taps_1x1", 1, 1, [0], [0], 3))
    out.append(_tap_case("taps_1x9", 1, 9, list(range(9)), [0], 4))
    out.append(_tap_case("taps_9x1", 9, 1, [0], list(range(9)), 5))
    return out


# ---- depth fall-back ---------------------------------------------------------------------------------------------------
SUBNORMAL = np.nextafter(f32(0), f32(1))


def depth_fallback():
    """A 4 x 4 grid of 2 x 2 neighbourhoods (top-left pixel (4 + 8i, 3 + 5j)). Row j zeroes tap j (0: top-left, 1:
    top-right, 2: bottom-left, 3: bottom-right); column i puts the NEAREST pixel on tap i (the fractional parts 0.75 /
    0.25 choose it). On the diagonal the nearest pixel is the zeroed one (dD = 0); elsewhere the fall-back reads a valid
    pixel whose depth is none of the other taps'. Then: all four valid, a tap of -1, the nearest pixel -1, a subnormal."""
    rgb, depth = frame(EH, EW, 6, Z2)
    pts, expect = [], []
    tap_xy = [(0, 0), (1, 0), (0, 1), (1, 1)]
    for j in range(4):
        for i in range(4):
            x, y = 4 + 8 * i, 3 + 5 * j
            depth[y:y + 2, x:x + 2] = Z2 + np.array([[0.25, 0.5], [0.75, 1.0]])      # four different depths
            depth[y + tap_xy[j][1], x + tap_xy[j][0]] = 0.0
            nx, ny = tap_xy[i]
            u = x + (0.75 if nx == 0 else 1.25)              # nearest = trunc(u): x (frac 0.75) or x + 1 (frac 0.25)
            v = y + (0.75 if ny == 0 else 1.25)
            pts.append(p2(u, v))
            expect.append(0.0 if i == j else float(depth[y + ny, x + nx]) - Z2)
    extra = [(36.75, 3.75, None), (36.75, 8.75, (1, 1, -1.0)), (36.75, 13.75, (0, 0, -1.0)),
             (36.75, 18.75, (1, 0, SUBNORMAL)), (1.75, 21.75, (0, 0, SUBNORMAL))]
    for u, v, tap in extra:
        x, y = int(u), int(v)
        depth[y:y + 2, x:x + 2] = Z2 + np.array([[0.25, 0.5], [0.75, 1.0]])
        if tap:
            depth[y + tap[1], x + tap[0]] = tap[2]
        pts.append(p2(u, v))
    c = _case("depth_fallback", rgb, depth, pts, K=K_P2)
    r = ref(c, 1)
    dd = r["point_x"][0, :, 6]
    assert r["fallback"][0, :16].all() and dd[:16].tolist() == expect
    assert sum(e != 0 for e in expect) == 12                  # the chosen nearest pixel is not the zeroed tap: 12 of 16
    a, b, cc, d = (f32(Z2 + q) for q in (0.25, 0.5, 0.75, 1.0))
    mixed = ((a * f32(0.5625) + b * f32(0.1875)) + cc * f32(0.1875)) + d * f32(0.0625)
    assert not r["fallback"][0, 16] and dd[16] == mixed - f32(Z2) and dd[16] not in (0.25, 0.5, 0.75, 1.0)
    assert r["fallback"][0, 17] and dd[17] == 0.25            # a tap of -1 is invalid; the nearest pixel is used
    assert r["fallback"][0, 18] and dd[18] == 0               # the nearest pixel itself -1: no depth, dD = 0
    assert not r["fallback"][0, 19] and not r["fallback"][0, 20]       # the smallest subnormal is a valid depth
    assert dd[20] != 0 and ref(c, 0)["point_x"][0, 20, 6] == SUBNORMAL - f32(Z2)
    return c


# ---- margin ------------------------------------------------------------------------------------------------------------
def margin():
    """z' = 2^-6, where z' + float32(0.02) and z' + 0.25 are exact. Pixels (4k, 3): D - z' == 0.02 (no violation: the
    test is strict), one ulp more (violation), == 0.25, one ulp more, D = 0, D in front of the point, a plain violation;
    an out-of-frame point whose pixel (0,0) would be a violation."""
    z = f32(2.0 ** -6)
    d002, d025 = f32(z + M002), f32(z + f32(0.25))
    assert float(d002) == float(z) + float(M002) and d002 - z == M002 and d025 - z == f32(0.25)
    values = [d002, np.nextafter(d002, f32(1)), d025, np.nextafter(d025, f32(1)), f32(0), z / f32(2), f32(1)]
    depth = np.zeros((EH, EW), f32)
    rgb, _ = frame(EH, EW, 7)
    pts = []
    for k, d in enumerate(values):
        depth[3, 4 * k + 2] = d
        pts.append(point(4 * k + 2.25, 3.75, float(z)))
    depth[0, 0] = 50.0
    pts.append(point(float(EW) + 2.25, 3.75, float(z)))      # out of frame: never counted
    c = _case("margin", rgb, depth, pts, margins=(0.02, 0.25))
    for interp in (0, 1):
        assert ref(c, interp, 0.02)["viol"][0].tolist() == [False, True, True, True, False, False, True, False]
        assert ref(c, interp, 0.25)["viol"][0].tolist() == [False, False, False, True, False, False, True, False]
    return c


# ---- HSV ---------------------------------------------------------------------------------------------------------------
HALF_UP = np.nextafter(f32(0.5), f32(1))
HSV_SET = np.array([
    [0.5, 0.5, 0.5], [0, 0, 0], [1, 1, 1],                   # grey, black, white: no hue
    [0.75, 0.75, 0.25], [0.25, 0.75, 0.75], [0.75, 0.25, 0.75], [0.75, 0.75, 0.75 - 2.0 ** -8],   # pairs tied at the maximum
    [1, 0.25, 0.5],                                          # red maximum, g < b: negative hue, wraps
    [1, 0.5, HALF_UP],                                       # hue one ulp below 0: lands on 1.0
    [1, 0.5, 0.5], [1, 0, 0], [0, 1, 0], [0, 0, 1],          # hue 0 (red), the pure primaries
    [0, 1, 1],                                               # hue exactly 0.5
    [0, 1 - 2.0 ** -8, 1],                                   # hue just above 0.5
    [1, 1, 0], [0.25, 0.5, 1.0]], dtype=f32)


def hsv_set_premise():
    hsv, branch, wrap = rf.hsv_full(HSV_SET)
    h = hsv[:, 0]
    assert branch[:3].tolist() == [0, 0, 0] and (h[:3] == 0).all() and hsv[1].tolist() == [0, 0, 0]
    assert branch[3:7].tolist() == [1, 2, 1, 1]              # a tie goes to the first of r, g, b that equals the maximum
    assert wrap[7] and h[7] > 0.9 and wrap[8] and h[8] == 1.0
    assert h[9] == 0 and h[10] == 0 and not wrap[10] and h[13] == 0.5 and 0.5 < h[14] < 0.501
    return hsv


def hsv_pairs():
    """Every colour of HSV_SET as an observed pixel (column i of the frame, staged from a float image) against every
    colour as a model colour (point j of column i), at pixel centres: a bilinear mix there is the pixel itself (weights
    1, 0, 0, 0). |H_obs - H_model| is exactly 0.5 (red, cyan), just above it, and 1 (hue 0 against hue 1.0)."""
    n = len(HSV_SET)
    hsv = hsv_set_premise()
    rgb, depth = frame(EH, EW, 8, Z2)
    rgb[:, :n] = HSV_SET[None]
    uv = [(i + 0.5, j + 0.5) for i in range(n) for j in range(n)]
    c = _case("hsv_pairs", rgb, depth, [p2(u, v) for u, v in uv], col=np.tile(HSV_SET, (n, 1)), K=K_P2)
    for interp in (0, 1):
        r = ref(c, interp)
        assert (r["wx"] == 0).all() and (r["wy"] == 0).all()
        dh = r["point_x"][0, :, 3].reshape(n, n)                      # [observed, model]
        assert dh[13, 10] == 0.5 and dh[10, 13] == 0.5                # exactly 0.5 either way round
        assert dh[14, 10] == f32(1) - hsv[14, 0] and dh[14, 10] < 0.5  # just above 0.5: 1 - d is the smaller
        assert dh[8, 10] == 0 and dh[10, 8] == 0 and dh[8, 9] == 0    # |1.0 - 0| = 1: the same hue
        assert (dh >= 0).all() and (dh <= 0.5).all()
    return c


def hsv_taps():
    """Observed colours through the four bilinear taps: 2 x 2 neighbourhoods whose left and right columns hold two
    different colours with max - min >= 0.1 on a 1/256 grid (the mix with quarter weights is exact and its hue well
    conditioned), points at every quarter offset, against all model colours of HSV_SET."""
    good = [i for i in range(len(HSV_SET)) if i not in (0, 1, 2, 8, 6)]
    rgb, depth = frame(EH, EW, 9, Z2)
    pts, col = [], []
    for k, i in enumerate(good):
        x, y = 3 * (k % 12) + 1, 4 * (k // 12) + 1
        rgb[y:y + 2, x], rgb[y:y + 2, x + 1] = HSV_SET[i], HSV_SET[good[(k + 5) % len(good)]]
        for fu in (0.5, 0.75, 1.0, 1.25):
            for fv in (0.5, 0.75, 1.0, 1.25):
                for j in (7, 10, 13, 14, 16):
                    pts.append(p2(x + fu, y + fv))
                    col.append(HSV_SET[j])
    c = _case("hsv_taps", rgb, depth, pts, col=col, K=K_P2)
    r = ref(c, 1)
    assert len(set(r["branch_obs"][0].tolist())) == 3 and r["wrap_obs"].any() and r["bil"].all()
    return c


def hsv_near_grey_taps():
    """Near-grey interpolated colours (max - min of one 1/256 step and of one ulp): hue is ill-conditioned, the branch can
    turn on a rounding. Bit-equality leg only (NOT_IN_F64)."""
    rgb, depth = frame(EH, EW, 10, Z2)
    g = f32(0.5)
    rgb[4:6, 4], rgb[4:6, 5] = [g, g, HALF_UP], [HALF_UP, g, g]
    rgb[10:12, 4], rgb[10:12, 5] = [g, g + f32(2.0 ** -8), g], [g, g, g]
    rgb[16:18, 4], rgb[16:18, 5] = [f32(0.3), f32(0.3) + f32(1e-7), f32(0.3)], [f32(0.7), f32(0.7), f32(0.7) + f32(1e-7)]
    pts = [[4 + fu, y + fv, Z2] for y in (4, 10, 16) for fu in (0.5, 0.8, 1.0, 1.3) for fv in (0.6, 1.1)]   # inexact weights
    return _case("hsv_near_grey_taps", rgb, depth, pts, K=K_P2)


# ---- normalisation -----------------------------------------------------------------------------------------------------
def normalisation():
    out = []
    rgb, depth = frame(EH, EW, 11)
    c = _case("norm_M1", rgb, depth, [point(7.25, 5.75)])
    r = ref(c, 0)
    assert r["extent"][0] == 1 and r["point_x"][0, 0, :2].tolist() == [0, 0]             # e := 1, x = y = 0
    out.append(c)
    c = _case("norm_one_pixel", rgb, depth, [point(7 + fu, 5 + fv) for fu in FRACS for fv in FRACS])
    r = ref(c, 1)
    assert r["extent"][0] == 1 and (r["point_x"][0, :, :2] == 0).all() and (r["uv"][0] == [7, 5]).all()
    out.append(c)
    T = np.tile(EYE, (2, 1, 1))
    T[1, 2, 3] = -200.0
    c = _case("norm_all_behind", rgb, depth, [point(3.5 + i, 2.5 + i) for i in range(6)], T=T)
    r = ref(c, 1)
    assert (r["uv"][1] == -1).all() and r["extent"][1] == 1 and (r["point_x"][1, :, :2] == 0).all()
    assert (r["point_x"][1, :, 6] == depth[0, 0] + f32(100)).all() and r["count"][1] == 0   # pixel (0,0), never counted
    out.append(c)
    us = [3.5, 4.5, 8.5, 30.5, -2.0, 41.0, 55.5, 1000.0]       # four in, four out
    c = _case("norm_half_out", rgb, depth, [point(u, 6.5 + i) for i, u in enumerate(us)])
    r = ref(c, 1)
    assert r["inb"][0].tolist() == [True] * 4 + [False] * 4
    assert r["mean"][0].tolist() == [45 / 8, 30 / 8] and r["extent"][0] == f32(30) - f32(45 / 8)   # a non-integer mean
    out.append(c)
    vs = [0.5, 3.5, 11.5, 23.5]                               # the extent comes from v alone: |v - mean| > every |u - mean|
    c = _case("norm_extent_from_v", rgb, depth, [point(6.5 + i, v) for i, v in enumerate(vs)])
    r = ref(c, 1)
    assert r["extent"][0] == f32(23) - f32(37 / 4) and r["extent"][0] > np.abs(r["uc"][0] - r["mean"][0, 0]).max() * 4
    out.append(c)
    return out


def norm_sum_past_2p24():
    """2 x 4096 frame, 5000 points at u = 4095 and one at u = 1: the integer sum 20 475 001 is odd and above 2^24, so
    (float)sum rounds (SPEC 3.4: the sum is an integer, the mean is taken from its float32 value)."""
    H, W, M = 2, 4096, 5001
    rgb, depth = frame(H, W, 12)
    pts = [point(4095.5, 0.5 + (i % 2)) for i in range(5000)] + [point(1.5, 0.5)]
    c = _case("norm_sum_past_2p24", rgb, depth, pts)
    r = ref(c, 0)
    su = 5000 * 4095 + 1
    assert int(r["uc"][0].sum()) == su and float(f32(su)) != su and r["mean"][0, 0] == f32(su) / f32(M)
    return c


# ---- projection refusals and degenerate geometry -------------------------------------------------------------------------
def refusals():
    out = []
    T, pts, depth = proj_case_near()                          # z' = 1e-6 (refused), its successor (kept), u_f = 25
    rgb, _ = frame(EH, EW, 13)
    c = _case("refuse_z_min", rgb, depth, pts, T=T[None])
    for interp in (0, 1):
        r = ref(c, interp)
        assert r["uv"][0].tolist() == [[-1, -1], [0, 0], [25, 12], [-1, -1]]
        assert r["viol"][0].tolist() == [False, True, True, False] and r["inb"][0].tolist() == [False, True, True, False]
    out.append(c)

    rgb, depth = frame(EH, EW, 14)
    depth[0, 0] = 150.0                                       # pixel (0,0) would be a violation if a refused point counted
    depth[5, 10] = depth[15, 20] = 99.0                       # the two in-frame points are no violations
    pts = np.array([point(10.25, 5.75), point(20.75, 15.25), [1.0e7, 0, 1.0], [0, -1.0e7, 1.0], [2.0e7, 0, 1.0],
                    [2.0 ** 23, 0, 1.0]], f32)
    T = np.tile(EYE, (6, 1, 1))
    T[1, 0, 0], T[2, 2, 3], T[3, 0, 3], T[4, 1, 1], T[5, 2, 3] = np.nan, np.nan, np.inf, -np.inf, np.inf
    c = _case("refuse_nonfinite_and_1e9", rgb, depth, pts, T=T)
    for interp in (0, 1):
        r = ref(c, interp)
        assert r["uv"][0].tolist() == [[10, 5], [20, 15], [-1, -1], [-1, -1], [-1, -1], [838860800, 0]]
        for n in (1, 2, 3, 4):                                # NaN / inf in the transform: every point is refused
            assert (r["uv"][n][:2] == -1).all() and not r["inb"][n].any() and r["count"][n] == 0
            assert (r["uc"][n] == 0).all() and (r["vc"][n] == 0).all()
        assert r["count"][0] == 0 and not r["inb"][0, 2:].any()
        assert r["uv"][5, :2].tolist() == [[0, 0], [0, 0]]    # z' = inf: u_f = 0, a finite pixel, D - inf never a violation
    out.append(c)

    rgb, depth = frame(EH, EW, 15)
    T = EYE.copy()
    T[:3, 3] = [-1.0, -2.0, -3.0]
    pts = np.array([[1, 2, 3], [1 + coord(5.5), 2 + coord(5.5), 103.0], [1 + coord(9.5), 2 + coord(3.5), 103.0]], f32)
    nrm = np.array([[0, 0, -1], [0, 0, 0], [0, 0, -1]], f32)
    c = _case("degenerate_geometry", rgb, depth, pts, T=T[None], nrm=nrm)
    r = ref(c, 0)
    assert r["uv"][0].tolist() == [[-1, -1], [5, 5], [9, 3]]
    assert r["point_x"][0, :2, 7].tolist() == [0, 0] and r["point_x"][0, 2, 7] < -0.99       # |p'| = 0; zero normal
    return out + [c]


# ---- sizes -------------------------------------------------------------------------------------------------------------
SIZES_M = [1, 63, 64, 65, 255, 256, 257, 1023, 1025]


def _scatter(M, seed, H=EH, W=EW):
    """M points at z = 128 (K_P2) whose pixel coordinates have fractional part 0.25 or 0.75 (trunc and floor(. - 0.5) are then
    safe from rounding under integer shifts and a doubling of z), spread over the frame and a little past it"""
    rng = np.random.default_rng(seed)
    u = rng.integers(-3, W + 3, M) + rng.choice([0.25, 0.75], M)
    v = rng.integers(-2, H + 2, M) + rng.choice([0.25, 0.75], M)
    return np.stack([u, v, np.full(M, Z2)], 1).astype(f32)


def _shifts():
    T = np.tile(EYE, (3, 1, 1))
    T[1, :3, 3] = [-7.0, 3.0, 0.0]
    T[2, :3, 3] = [4.0, -2.0, Z2]                             # z' = 256: the pixel coordinates halve
    return T


def sizes():
    """M around the wave (64) and workgroup (256) sizes and past four sweeps; N' = 3 (all) and N' = 1 (sel = [1])"""
    out = []
    for M in SIZES_M:
        rgb, depth = frame(EH, EW, 20 + M, Z2)
        depth[::3, ::4] = 0                                   # some invalid depth: fall-backs and dD = 0 at every size
        c = _case("size_M%d" % M, rgb, depth, _scatter(M, M), T=_shifts(), nrm=normals(M), K=K_P2, sels=[None, [1]])
        r = ref(c, 1)
        assert M < 60 or (r["inb"].any(1).all() and not r["inb"].all(1).any() and r["fallback"].any())
        out.append(c)
    return out


def sel_variants():
    M = 65
    T = np.tile(EYE, (5, 1, 1))
    T[:, 0, 3] = [0.0, -5.0, 3.0, -11.0, 8.0]
    rgb, depth = frame(EH, EW, 16, Z2)
    c = _case("sel_variants", rgb, depth, _scatter(M, 99), T=T, nrm=normals(M),
              K=K_P2, sels=[[4, 3, 2, 1, 0], [2, 2, 0, 2], [3], []])
    cnt = ref(c, 0)["uv"]
    assert len({cnt[n].tobytes() for n in range(5)}) == 5     # five different hypotheses: a wrong selection shows
    return c


N_MANY = 65537


def many_hypotheses():
    """65537 hypotheses of 3 points: hypotheses ride on grid.x, nothing may wrap at 65535"""
    rng = np.random.default_rng(17)
    T = np.tile(EYE, (N_MANY, 1, 1))
    T[:, 0, 3] = rng.integers(-8, 3, N_MANY)
    T[-1, 0, 3], T[-2, 0, 3], T[0, 0, 3], T[1, 0, 3] = 2.0, -5.0, -1.0, 1.0          # the ends differ from each other
    rgb, depth = frame(EH, EW, 18, Z2)
    return _case("many_hypotheses", rgb, depth, [p2(10.25, 5.75), p2(20.75, 15.25), p2(3.25, 20.75)], T=T, K=K_P2)


# ---- staging -----------------------------------------------------------------------------------------------------------
BLUR_SHAPES = [(h, w) for h in (1, 2, 3, 4) for w in (1, 2, 3, 4, 7)] + [(7, 1), (7, 2), (9, 33), (8, 32), (9, 32), (8, 33)]


def staging_cases():
    """(name, uint8 image, depth): frames whose height or width is 1..4 (the 5-tap reflection folds more than once),
    9 x 33 (one pixel past the 8 x 32 tile both ways), an all-255 image, and a patch whose weighted sum is 128 mod 256"""
    out = []
    for h, w in BLUR_SHAPES:
        rng = np.random.default_rng(100 * h + w)
        out.append(("blur_%dx%d" % (h, w), rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.random((h, w)).astype(f32)))
    out.append(("all_255", np.full((9, 33, 3), 255, np.uint8), np.ones((9, 33), f32)))
    img = np.zeros((9, 9, 3), np.uint8)
    img[4, 4], img[2, 2] = 3, 20                              # 36 * 3 + 1 * 20 = 128 at (4,4): rounds up to 1
    k = np.array([1, 4, 6, 4, 1])
    assert int((np.outer(k, k) * img[2:7, 2:7, 0]).sum()) == 128 and rf.blur5_u8(img)[4, 4, 0] == 1
    out.append(("half_rounds_up", img, np.ones((9, 9), f32)))
    return out


# ---- the hypothesis filter's threshold ---------------------------------------------------------------------------------
def filter_edge():
    """M = 200 points on 5 rows of the edge frame at z = 128 (K_P2); three hypotheses shifted down by 0, 6 and 12 rows, whose rows
    hold exactly 20, 21 and 19 pixels of depth 129 (violations) among pixels of depth 127. At inconst_ratio_th = 10:
    100 * 20 <= 10 * 200 keeps the first, 100 * 21 > 2000 drops the second (SPEC 3.5)."""
    rgb, _ = frame(EH, EW, 19)
    depth = np.full((EH, EW), Z2 - 1, f32)
    for n, k in enumerate((20, 21, 19)):
        depth[6 * n: 6 * n + 5].reshape(-1)[np.arange(k) * 7] = Z2 + 1       # a view: the five rows are contiguous
    pts = [p2((i % EW) + 0.5, (i // EW) + 0.5) for i in range(200)]
    T = np.tile(EYE, (3, 1, 1))
    T[:, 1, 3] = [0.0, 6.0, 12.0]
    c = _case("filter_edge", rgb, depth, pts, T=T, nrm=normals(200), K=K_P2)
    assert ref(c, 0)["count"].tolist() == [20, 21, 19]
    return c


@functools.lru_cache(maxsize=None)
def featurize_cases():
    """every featurizer case, name -> case, built (and its premises asserted) once per process"""
    cs = [borders()] + bilinear_taps() + [depth_fallback(), margin(), hsv_pairs(), hsv_taps(), hsv_near_grey_taps()]
    cs += normalisation() + [norm_sum_past_2p24()] + refusals() + sizes() + [sel_variants(), many_hypotheses(),
                                                                            filter_edge()]
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names) and set(NOT_IN_F64) <= set(names)
    return {c["name"]: c for c in cs}


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """bit equality of two arrays; NaNs must sit at the same places (their payloads differ between CPUs and GPUs and
    carry nothing), and -0.0 is not 0.0"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != f32:
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


CHANNELS = ("x", "y", "zero", "dH", "dS", "dV", "dD", "cosN")
FLOOR = 2.0 ** -24


def channel_errors(got, want64):
    """per channel of point_x: max|got - f64| / max(max|f64|, 1) over the finite entries. Where the float64 value is
    not finite (a NaN or inf put into a transform) `got` must be the same non-finite value: asserted, not skipped."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    fin = np.isfinite(want64)
    assert np.array_equal(fin, np.isfinite(got)) and np.array_equal(np.isnan(want64), np.isnan(got))
    assert np.array_equal(got[~fin & ~np.isnan(got)], want64[~fin & ~np.isnan(want64)])          # the same infinities
    err = np.zeros(8)
    for ch in range(8):
        f = fin[..., ch]
        if f.any():
            g, w = got[..., ch][f], want64[..., ch][f]
            err[ch] = np.abs(g - w).max() / max(np.abs(w).max(), 1.0)
    return err


def within_4x(err, err32):
    """SPEC 3.6: per channel, the error against float64 is at most 4 x the float32 restatement's own (floor 2^-24)"""
    return [CHANNELS[ch] for ch in range(8) if not err[ch] <= 4 * max(err32[ch], FLOOR)]
