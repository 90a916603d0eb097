"""Inputs of the frame-side edge tests, built once and shared by the CPU tests (float32 oracle against the float64
restatement, tests/test_pipeline.py) and the GPU tests (kernels against both, tests/test_pipeline_edges_gpu.py).
Every value that decides a comparison is exactly representable in float32, so the float32 kernels / oracle and the
float64 restatement must agree exactly: a disagreement is a wrong convention, never rounding."""
import numpy as np

f32 = np.float32
EH, EW = 24, 40                                              # the edge frame
K_EDGE = np.array([[100.0, 0.0, 0.0], [0.0, 100.0, 0.0], [0.0, 0.0, 1.0]])
EYE = np.eye(4)
Z_MIN32 = f32(1e-6)
Z_NEXT32 = np.nextafter(Z_MIN32, f32(1))


def coord(target, z=100.0, f=100.0):
    """x (float32) whose pixel coordinate (x / z) * f is `target`: exactly `target` in float32, and in float64 a value
    that floors and truncates like it. z = 100 * 2^k gives that for every edge value used here (x / 100 * 100 returns x
    for them, and a power of two scales exactly). A coordinate well inside a pixel (further than 0.01 from an integer)
    need not be exact: there every rounding floors and truncates alike. Asserted, not assumed."""
    z32, f32_ = f32(z), f32(f)
    x = f32(target * z / f)
    got32 = (x / z32) * f32_
    got64 = (float(x) / float(z32)) * float(f32_)
    same = all(fn(g) == fn(target) for fn in (np.floor, np.trunc) for g in (got32, got64))
    inside = abs(target - round(target)) > 0.01
    assert same and (got32 == f32(target) or inside), "no exact float32 coordinate for u_f = %r at z = %r" % (target, z)
    return x


def point(u, v, z=100.0):
    return [coord(u, z), coord(v, z), f32(z)]


# ---- sample producer ---------------------------------------------------------------------------------------------------
PREP_PAIRS = [((37, 53), (37, 53)), ((37, 53), (37, 255)), ((37, 53), (37, 256)), ((37, 53), (37, 257)),
              ((37, 53), (74, 53)), ((37, 53), (19, 106)), ((37, 53), (1, 1)), ((1, 9), (5, 513)), ((9, 1), (3, 255)),
              ((480, 640), (224, 224))]


def prep_frame(h, w, seed=11):
    """uint8 image, depth with about 10 % zeros, a mask of a few rectangles (0/1 float32), a camera"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    depth = rng.uniform(0.4, 1.6, (h, w)).astype(f32)
    depth[rng.random((h, w)) < 0.1] = 0
    mask = np.zeros((h, w), f32)
    for _ in range(3):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        mask[y0:y0 + 1 + int(rng.integers(0, max(h // 3, 1))), x0:x0 + 1 + int(rng.integers(0, max(w // 3, 1)))] = 1
    K = np.array([[0.9 * w, 0, 0.5 * w - 0.25], [0, 0.95 * w, 0.5 * h + 0.125], [0, 0, 1.0]])
    return img, depth, mask, K


# ---- box and heat map --------------------------------------------------------------------------------------------------
def _one(h, w, index, value=1.0):
    m = np.zeros(h * w, f32)
    m[index] = value
    return m.reshape(h, w)


def bbox_masks():
    """name -> mask"""
    out = {"corner_tl": _one(480, 640, 0), "corner_tr": _one(480, 640, 639), "corner_bl": _one(480, 640, 479 * 640),
           "corner_br_last_index": _one(480, 640, 480 * 640 - 1),
           "index_1023": _one(40, 52, 1023), "index_1024": _one(40, 52, 1024),
           "w1": _one(300, 1, 217), "all_zero": np.zeros((23, 31), f32)}
    m = np.zeros((5, 7), f32)
    m[1, 2] = m[3, 5] = 1
    out["fewer_pixels_than_threads"] = m
    m = np.full((6, 9), f32(-0.0))                          # -0.0 is zero: not in the box
    m[2, 3], m[4, 1] = f32(1e-30), f32(-3.0)                # tiny and negative values are non-zero: in it
    out["signed_and_tiny_values"] = m
    m = np.zeros((300, 1), f32)
    m[[3, 298], 0] = 1
    out["w1_two"] = m
    m = np.zeros((40, 52), f32)                             # the bottom edge is decided by thread 1007, in the 16th wave
    m[39, 3] = m[1, 51] = m[30, 0] = 1                      # linear indices 2031 (= 1024 + 1007), 103, 1560
    out["sixteenth_wave"] = m
    return out


def heat_cases():
    """(mask, hh, hw, scale): the heat map follows from the mask's box"""
    a = np.zeros((58, 78), f32)
    a[10:21, 30:42] = 1                                     # box (30,10,41,20): centre x 35.5 is a half-integer
    b = np.zeros((7, 300), f32)
    b[2:5, 100:251] = 1
    return [(a, 29, 39, 0.5), (a, 1, 1, 1.0 / 58), (b, 7, 300, 1.0), (a, 29, 39, 1.0)]


# ---- splat -------------------------------------------------------------------------------------------------------------
U_EDGES = [-0.5, 0.0, EW - 1.0, EW - 0.5, float(EW)]
V_EDGES = [-0.5, 0.0, EH - 1.0, EH - 0.5, float(EH)]


def splat_points():
    """float32 [M,3] under the identity pose and K_EDGE on the EH x EW frame (what they must draw at radius 0:
    tests/test_pipeline.py::_check_splat_r0)"""
    p = [point(u, 10.5 + i, 100.0) for i, u in enumerate(U_EDGES)]           # rows 10..14
    p += [point(20.5 + i, v, 200.0) for i, v in enumerate(V_EDGES)]          # columns 20..24
    p += [point(5.5, EW - 1.0, 50.0), point(6.5, EW - 0.5, 50.0), point(7.5, float(EW), 50.0)]   # the u set as v_f: off
    p += [point(-0.5, -0.5, 25.0), point(EW - 0.5, EH - 0.5, 400.0), point(float(EW), float(EH), 800.0)]   # corners
    p += [point(10.25, 5.5, 100.0), point(10.25, 5.5, 50.0),           # one pixel, far then near: the nearer wins
          point(30.25, 3.5, 50.0), point(30.25, 3.5, 100.0)]           # ... and near then far
    p += [[0, 0, Z_MIN32], [0, 0, Z_NEXT32]]                           # z' = 1e-6 dropped; the next float kept, on pixel (0, 0)
    p += [[1, 1, -100.0], [0.1, 0.1, np.nan], [np.nan, 0.1, 50.0], [0.1, 0.1, np.inf], [np.inf, 0.1, 50.0]]
    p += [[1.0e7, 0, 1.0], [0, -1.0e7, 1.0], [2.0e7, 0, 1.0]]          # |u_f| = 1e9 exactly, |v_f| = 1e9, 2e9: dropped
    p += [[np.nextafter(f32(1.0e7), f32(0)), 0, 1.0]]                  # just below 1e9: used, far off the image
    return np.array(p, dtype=f32)


def splat_random(M=257, seed=4):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 2.0, M)
    return np.stack([rng.uniform(-0.02, 0.25, M) * z, rng.uniform(-0.02, 0.13, M) * z, z], 1).astype(f32)


# ---- visibility ----------------------------------------------------------------------------------------------------------
DELTA = 2.0 ** -6


def visib_frame(H, W, seed=7):
    """depths on a 2^-10 grid (differences exact in float32, many exactly at DELTA = 16 * 2^-10), zeros in both,
    ground-truth masks drawn independently of the prediction"""
    rng = np.random.default_rng(seed + H * 1000 + W)
    d_obs = rng.integers(400, 1600, (H, W)) / 1024.0
    d_pred = d_obs + rng.integers(-32, 33, (H, W)) / 1024.0
    d_obs[rng.random((H, W)) < 0.15] = 0
    d_pred[rng.random((H, W)) < 0.4] = 0
    gt, gtv = rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.35
    return d_obs.astype(f32), d_pred.astype(f32), gt, gtv


def visib_edge_row():
    """d_obs, d_pred [1,7], expected predicted mask, expected visible mask at DELTA = 2^-6"""
    above = np.nextafter(f32(0.515625), f32(1))
    d_obs = np.array([[0.5, 0.5, 0.0, 0.5, 0.5, 0.5, np.nan]], f32)
    d_pred = np.array([[0.515625, above, 0.3, 0.0, -0.2, -0.0, 0.4]], f32)
    pm = np.array([[1, 1, 1, 0, 0, 0, 1]], bool)
    vm = np.array([[1, 0, 1, 0, 0, 0, 0]], bool)
    return d_obs, d_pred, pm, vm


# ---- ADD / ADI ------------------------------------------------------------------------------------------------------------
def _rot(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def pose_case(N, M, seed=5):
    """float64 poses [N,4,4] (hypothesis 0 IS the ground truth), ground truth [4,4], points [M,3]"""
    rng = np.random.default_rng(seed + 7 * N + M)
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = _rot(rng, 1.1), [0.03, -0.02, 0.8]
    T = np.tile(gt, (N, 1, 1))
    if N > 1:
        d = rng.normal(size=(N, 3)) * 0.01
        d[0] = 0
        T[:, :3, 3] += d
    for n in range(1, min(N, 8)):
        T[n, :3, :3] = _rot(rng, 0.05 * n) @ gt[:3, :3]
    return T, gt, rng.uniform(-0.1, 0.1, (M, 3))


ADI_SIZES = [6400, 2731, 2730, 2729, 2049, 2048, 257, 256, 255, 1]      # the largest first


# ---- projection ---------------------------------------------------------------------------------------------------------
MARGIN = 2.0 ** -5
PU_EDGES = [-1.0, -0.5, 0.0, 39.99, 40.0]
PV_EDGES = [-1.0, -0.5, 0.0, 23.99, 24.0]


def proj_case():
    """points f32 [M,3], depth f32 [EH,EW], for the identity pose: the edge coordinates of the truncating projection,
    z' = 1e-6 and the next float, and depth pixels at exactly MARGIN behind a point (not a violation) and one float more
    (a violation)."""
    p = [point(u, 10.5 + i) for i, u in enumerate(PU_EDGES)] + [point(20.5 + i, v) for i, v in enumerate(PV_EDGES)]
    p += [point(39.99, -0.5), point(-0.5, -0.5), point(-1.0, 0.0)]
    p += [point(30.5, 3.5), point(32.5, 3.5), point(34.5, 3.5), point(36.5, 3.5)]      # the margin pixels, see below
    p += [[0, 0, Z_MIN32], [0, 0, Z_NEXT32], [0, 0, 0], [0, 0, -1]]
    pts = np.array(p, dtype=f32)
    depth = np.zeros((EH, EW), f32)
    depth[:, 0] = 101.0                                      # pixel column 0: what u_f = -0.5 truncates to
    depth[0, :] = 101.0
    depth[3, 30] = f32(100.0 + MARGIN)                       # d - z' == margin: not counted
    depth[3, 32] = np.nextafter(f32(100.0 + MARGIN), f32(1000))   # one float more: counted
    depth[3, 34] = 0.0                                       # no depth: not counted
    depth[3, 36] = 99.0                                      # in front of the point: not counted
    depth[10:15, 39] = 100.5                                 # u_f = 39.99 truncates to 39: counted
    return pts, depth


def proj_case_near():
    """one pose 1e-6 in front of the camera with its own points: z' = 1e-6 exactly (dropped), the next float (kept),
    and a point at x = z'/4, so u_f = 25 exactly"""
    T = np.eye(4)
    T[2, 3] = float(Z_MIN32)
    step = Z_NEXT32 - Z_MIN32                                # exact: neighbouring floats
    assert f32(Z_MIN32 + step) == Z_NEXT32
    pts = np.array([[0, 0, 0], [0, 0, step], [Z_NEXT32 * f32(0.25), Z_NEXT32 * f32(0.125), step], [0, 0, -step]], f32)
    depth = np.full((EH, EW), 0.5, f32)
    return T, pts, depth


def model_table_inputs(M, seed=9):
    """normals and colours to go with M points (the featurizer needs them; they decide nothing here)"""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(M, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32), rng.random((M, 3)).astype(f32)


def rgb_frame(seed=10):
    return np.random.default_rng(seed).random((EH, EW, 3)).astype(f32)


def mask_filter_case():
    """points [4,3] at u_f = -0.5, 0.25, 0.5, 5.5 (z = 100, so x IS u_f), poses [5,4,4] that shift x, a mask [EH,EW]
    with only column 0 set, and the fraction of points on the mask per pose:
      shift  0    -> u_f -0.5, 0.25, 0.5, 5.5   -> 3 of 4 on column 0 (u_f = -0.5 counts as pixel 0): above th = 0.5
      shift -0.5  -> u_f -1.0, -0.25, 0.0, 5.0  -> 2 of 4 (-1.0 is pixel -1, off the image): exactly th, not kept
      shift -5.5  -> only the last; shift 1.0 -> only the first (u_f 0.5); shift -41 -> none"""
    pts = np.array([point(-0.5, 3.5), point(0.25, 9.5), point(0.5, 15.5), point(5.5, 20.5)], f32)
    assert pts[:, 0].tolist() == [-0.5, 0.25, 0.5, 5.5]
    mask = np.zeros((EH, EW), np.int64)
    mask[:, 0] = 1
    T = np.tile(np.eye(4), (5, 1, 1))
    T[:, 0, 3] = [0.0, -0.5, -5.5, 1.0, -41.0]
    return pts, T, mask, np.array([0.75, 0.5, 0.25, 0.25, 0.0])


def many_poses(N, seed=2):
    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4), (N, 1, 1))
    T[:, 0, 3] = rng.integers(-8, 3, N).astype(np.float64)
    return T
