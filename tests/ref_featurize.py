"""Independent numpy restatement of SPEC.md sections 2-3 -- test infrastructure that pins oracle/zephyr_oracle.c and
csrc/zephyr.hip from a second implementation (vectorised arrays instead of scalar loops), written from SPEC.md alone.

Every function takes `dtype`. With float32 (the default) each operation is one float32 numpy operation in the explicit
parenthesisation of SPEC 3.2-3.4, and the result is held to BIT EQUALITY with the oracle and the kernels. With float64
the same text is evaluated in double precision on the same (float32) inputs: the plain high-precision statement the
float channels are measured against, and whose DECISIONS (uv, in-frame, tap indices, depth fall-back, violations, hue
branch) must agree exactly on the edge inputs of tests/featurize_cases.py. The constants a decision compares against
(1e-6, 1e9, the margin) are the float32 values the C ABI carries, in both precisions."""
import numpy as np

f32 = np.float32
f64 = np.float64
Z_MIN = f32(1e-6)
UV_LIMIT = f32(1.0e9)


def _reflect101(i, n):
    """BORDER_REFLECT_101 index (SPEC 3.1), any overhang: ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..."""
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.abs(i) % p
    return np.where(i >= n, p - i, i)


def blur5_u8(img):
    k = np.array([1, 4, 6, 4, 1], dtype=np.int64)
    H, W = img.shape[:2]
    v = img.astype(np.int64)
    ys, xs = np.arange(H), np.arange(W)
    rows = sum(k[i] * v[:, _reflect101(xs + i - 2, W)] for i in range(5))
    S = sum(k[i] * rows[_reflect101(ys + i - 2, H)] for i in range(5))
    return ((S + 128) >> 8).astype(np.uint8)


def u8_to_unit(a):
    return a.astype(f32) / f32(255)


def pack_rgbd(rgb, depth):
    return np.concatenate([np.asarray(rgb, f32), np.asarray(depth, f32)[..., None]], -1)


def _hsv(rgb, dtype):
    """HSV of values already held in `dtype` (SPEC 3.4, matplotlib's rgb_to_hsv)"""
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    mx, mn = rgb.max(-1), rgb.min(-1)
    delta = mx - mn
    one, two, four, six = dtype(1), dtype(2), dtype(4), dtype(6)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(mx > 0, delta / mx, dtype(0))
        hr, hg, hb = (g - b) / delta, two + (b - r) / delta, four + (r - g) / delta
    branch = np.where(delta > 0, np.where(r == mx, 1, np.where(g == mx, 2, 3)), 0)
    h = np.where(branch == 1, hr, np.where(branch == 2, hg, hb))
    h = np.where(branch > 0, h, dtype(0)) / six
    wrap = h < 0
    h = np.where(wrap, h + one, h)
    return np.stack([h, s, mx], -1).astype(dtype), branch, wrap


def hsv_full(rgb, dtype=f32):
    """rgb: float32 values (anything else is rounded to float32 first, as staging does).
    -> hsv [...,3] dtype, branch [...] (0: no hue, delta = 0; 1, 2, 3: r, g, b is the maximum, first match wins),
    wrap [...] bool (the hue was negative and 1 was added)"""
    return _hsv(np.asarray(rgb, f32).astype(dtype), dtype)


def rgb_to_hsv(rgb, dtype=f32):
    return hsv_full(rgb, dtype)[0]


def model_table(pts, nrm, col_rgb):
    """the staged model table [M,12] float32: p(3) n(3) hsv(3) 0(3)"""
    M = len(pts)
    tab = np.zeros((M, 12), f32)
    tab[:, 0:3], tab[:, 3:6], tab[:, 6:9] = np.asarray(pts, f32), np.asarray(nrm, f32), rgb_to_hsv(col_rgb)
    return tab


def project(T, pts, K, dtype=f32):
    """-> cam [N,M,3], uf, vf [N,M] (dtype), uv [N,M,2] int32"""
    T, p = np.asarray(T, f32).astype(dtype), np.asarray(pts, f32).astype(dtype)
    fx, fy, cx, cy = (dtype(f32(K[0, 0])), dtype(f32(K[1, 1])), dtype(f32(K[0, 2])), dtype(f32(K[1, 2])))
    R, t = T[:, None, :3, :3], T[:, None, :3, 3]
    x, y, z = p[None, :, 0], p[None, :, 1], p[None, :, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cam = np.stack([((R[..., i, 0] * x + R[..., i, 1] * y) + R[..., i, 2] * z) + t[..., i] for i in range(3)], -1)
        ok = cam[..., 2] > dtype(Z_MIN)
        zs = np.where(ok, cam[..., 2], dtype(1))
        uf = (cam[..., 0] / zs) * fx + cx
        vf = (cam[..., 1] / zs) * fy + cy
        ok &= np.isfinite(uf) & np.isfinite(vf) & (np.abs(uf) < dtype(UV_LIMIT)) & (np.abs(vf) < dtype(UV_LIMIT))
    u = np.where(ok, np.trunc(np.where(ok, uf, 0)), -1).astype(np.int32)
    v = np.where(ok, np.trunc(np.where(ok, vf, 0)), -1).astype(np.int32)
    return cam.astype(dtype), uf, vf, np.stack([u, v], -1)


def featurize_full(rgbd, T, pts, nrm, col_rgb, K, interp=0, margin=0.02, sel=None, dtype=f32):
    """SPEC 3.2-3.5 for the hypotheses `sel` (None: all, in order). rgbd is the staged float32 frame [H,W,4].
    -> dict: point_x [N',M,8] dtype, uv [N',M,2] int32, count [N'] int32 and the decisions behind them:
    inb, uc, vc (the clamped pixel), viol [N',M], taps [N',M,4] = (x0, x1, y0, y1) and wx, wy (meaningful where `bil`),
    bil (bilinear gather used), fallback (bilinear colour, nearest-pixel depth), branch_obs / wrap_obs [N',M] and
    branch_model / wrap_model [M] (hsv_full), mean [N',2], extent [N']."""
    rgbd = np.asarray(rgbd, f32)
    H, W = rgbd.shape[:2]
    T = np.asarray(T, f32).reshape(-1, 4, 4)
    if sel is not None:
        T = T[np.asarray(sel, np.int64)]
    M = len(pts)
    cam, uf, vf, uv = project(T, pts, K, dtype)
    u, v = uv[..., 0], uv[..., 1]
    inb = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    uc, vc = np.where(inb, u, 0), np.where(inb, v, 0)
    near = rgbd[vc, uc].astype(dtype)                         # out-of-frame points read pixel (0, 0)
    obs = near
    bil = inb & bool(interp)
    one, half = dtype(1), dtype(0.5)
    xf, yf = np.where(bil, uf, half) - half, np.where(bil, vf, half) - half
    x0f, y0f = np.floor(xf), np.floor(yf)
    wx, wy = xf - x0f, yf - y0f
    x0, x1 = np.clip(x0f.astype(np.int64), 0, W - 1), np.clip(x0f.astype(np.int64) + 1, 0, W - 1)
    y0, y1 = np.clip(y0f.astype(np.int64), 0, H - 1), np.clip(y0f.astype(np.int64) + 1, 0, H - 1)
    a, b, c, d = (rgbd[y0, x0].astype(dtype), rgbd[y0, x1].astype(dtype), rgbd[y1, x0].astype(dtype),
                  rgbd[y1, x1].astype(dtype))
    w00, w10, w01, w11 = ((one - wx) * (one - wy))[..., None], (wx * (one - wy))[..., None], \
        ((one - wx) * wy)[..., None], (wx * wy)[..., None]
    mix = ((a * w00 + b * w10) + c * w01) + d * w11
    valid4 = (a[..., 3] > 0) & (b[..., 3] > 0) & (c[..., 3] > 0) & (d[..., 3] > 0)
    fallback = bil & ~valid4
    if interp:
        obs = np.where(bil[..., None], mix, near)
        obs[..., 3] = np.where(bil & valid4, mix[..., 3], near[..., 3])
    ohsv, branch_obs, wrap_obs = _hsv(obs[..., :3], dtype)
    mhsv, branch_model, wrap_model = hsv_full(col_rgb, dtype)
    dh = np.abs(ohsv[..., 0] - mhsv[None, :, 0])
    dh = np.minimum(dh, one - dh)
    od = obs[..., 3]
    R = T.astype(dtype)[:, None, :3, :3]
    n = np.asarray(nrm, f32).astype(dtype)[None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dd = np.where(od > 0, od - cam[..., 2], dtype(0))
        nr = np.stack([(R[..., i, 0] * n[..., 0] + R[..., i, 1] * n[..., 1]) + R[..., i, 2] * n[..., 2]
                       for i in range(3)], -1)
        dot = (nr[..., 0] * cam[..., 0] + nr[..., 1] * cam[..., 1]) + nr[..., 2] * cam[..., 2]
        ln = np.sqrt((cam[..., 0] * cam[..., 0] + cam[..., 1] * cam[..., 1]) + cam[..., 2] * cam[..., 2])
        cosn = np.where(ln > 0, dot / ln, dtype(0))
        nd = near[..., 3]                                    # the filter looks at the nearest pixel in both modes
        viol = inb & (nd > 0) & ((nd - cam[..., 2]) > dtype(f32(margin)))
    su, sv = uc.astype(np.int64).sum(1), vc.astype(np.int64).sum(1)
    mu, mv = (su.astype(dtype) / dtype(M))[:, None], (sv.astype(dtype) / dtype(M))[:, None]
    du, dv = uc.astype(dtype) - mu, vc.astype(dtype) - mv
    ext = np.maximum(np.abs(du).max(1, initial=0), np.abs(dv).max(1, initial=0))[:, None]
    ext = np.where(ext > 0, ext, one)
    px = np.stack([du / ext, dv / ext, np.zeros_like(du), dh, ohsv[..., 1] - mhsv[None, :, 1],
                   ohsv[..., 2] - mhsv[None, :, 2], dd, cosn], -1).astype(dtype)
    return dict(point_x=px, uv=uv, count=viol.sum(1).astype(np.int32), inb=inb, uc=uc, vc=vc, viol=viol,
                taps=np.stack([x0, x1, y0, y1], -1), wx=wx, wy=wy, bil=bil, fallback=fallback, branch_obs=branch_obs,
                wrap_obs=wrap_obs, branch_model=branch_model, wrap_model=wrap_model, mean=np.concatenate([mu, mv], 1),
                extent=ext[:, 0])


DECISIONS = ("uv", "count", "inb", "uc", "vc", "viol", "bil", "fallback", "taps", "branch_obs", "wrap_obs", "branch_model",
             "wrap_model")


def featurize(rgbd, T, pts, nrm, col_rgb, K, interp=0, margin=0.02, sel=None, dtype=f32):
    """-> point_x [N',M,8], uv_original [N',M,2] i32, free-space-violation counts [N'] i32"""
    r = featurize_full(rgbd, T, pts, nrm, col_rgb, K, interp, margin, sel, dtype)
    return r["point_x"], r["uv"], r["count"]
