"""Independent float64 numpy restatement of the frame-side steps (SPEC.md section 14) -- test
infrastructure. It imports nothing from oracle/ or the package and is written from the formulas the reference's lines
state (the lines oracle/pipeline_oracle.py cites): depth2xyz, the pixel-centre-aligned bilinear resize with clamped
borders, the rounded image, the mask's box and Gaussian heat map, the point splat, the bop19 visibility mask with the
four set sizes of the two IoUs, ADD / ADI, the truncating projection, the free-space count and the mask-hit fraction.

Everything is float64. The only float32 quantities are the thresholds the kernels hold as float32 constants (1e-6 and
1e9, taken at their float32 values) and whatever the caller passes in already rounded (depths, points, delta, margin)."""
import numpy as np

Z_MIN = float(np.float32(1e-6))      # a point is used iff z' > Z_MIN
UV_MAX = 1.0e9                       # ... and |u_f|, |v_f| < UV_MAX (exact in float32)
EMPTY_BOX = (1 << 30, 1 << 30, -1, -1, -1)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- sample producer ---------------------------------------------------------------------------------------------------
def depth2xyz(depth, K):
    """x = (col - cx) z / fx, y = (row - cy) z / fy, z -> [H,W,3]"""
    z = _f64(depth)
    K = _f64(K)
    rows, cols = np.indices(z.shape)
    return np.stack([(cols - K[0, 2]) * z / K[0, 0], (rows - K[1, 2]) * z / K[1, 1], z], -1)


def resize_taps(n_dst, n_src):
    """Source taps i0, i1 and the weight of i1 per destination index: s = (d + 1/2) n_src / n_dst - 1/2; below the
    first centre both taps are 0, above the last both are n_src - 1. Same size is the identity."""
    d = np.arange(n_dst)
    if n_dst == n_src:
        return d, d, np.zeros(n_dst)
    s = (d + 0.5) * (n_src / n_dst) - 0.5
    lo = np.floor(s)
    w = s - lo
    i0 = lo.astype(np.int64)
    i1 = i0 + 1
    w = np.where(i0 < 0, 0.0, w)
    return np.clip(i0, 0, n_src - 1), np.clip(i1, 0, n_src - 1), w


def resize_bilinear(a, H, W):
    """[h,w] or [h,w,C] -> [H,W(,C)]"""
    a = _f64(a)
    y0, y1, wy = resize_taps(H, a.shape[0])
    x0, x1, wx = resize_taps(W, a.shape[1])
    wy = wy.reshape((H, 1) + (1,) * (a.ndim - 2))
    wx = wx.reshape((1, W) + (1,) * (a.ndim - 2))
    top = a[y0][:, x0] * (1 - wx) + a[y0][:, x1] * wx
    bot = a[y1][:, x0] * (1 - wx) + a[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def round_half_up(a):
    """the uint8 an 8-bit image holds after the resize"""
    return np.floor(_f64(a) + 0.5)


def process_data(img, mask, depth, K, H, W):
    """img u8 [h,w,3], mask [h,w] in [0,1], depth [h,w] -> img [3,H,W] in [0,1], mask [1,H,W], xyz [3,H,W]"""
    xyz = depth2xyz(depth, K)
    if (H, W) == tuple(np.shape(depth)):
        im, m = _f64(img), _f64(mask)
    else:
        im, m, xyz = round_half_up(resize_bilinear(img, H, W)), resize_bilinear(mask, H, W), resize_bilinear(xyz, H, W)
    return np.moveaxis(im, 2, 0) / 255.0, m[None], np.moveaxis(xyz, 2, 0)


def mask_bbox(mask):
    """(x1, y1, x2, y2, label) of the non-zero pixels; -0.0 is zero. Empty: (2^30, 2^30, -1, -1, -1)."""
    on = _f64(mask) != 0
    rows, cols = np.flatnonzero(on.any(1)), np.flatnonzero(on.any(0))
    if rows.size == 0:
        return EMPTY_BOX
    return int(cols[0]), int(rows[0]), int(cols[-1]), int(rows[-1]), 1


def heatmap(box, hh, hw, scale, sigma):
    """exp(-d^2 / (2 sigma^2)) around the box centre times `scale`; all zero for the empty box"""
    if box[4] <= 0:
        return np.zeros((hh, hw))
    cx, cy = (box[0] + box[2]) / 2.0 * scale, (box[1] + box[3]) / 2.0 * scale
    y, x = np.indices((hh, hw))
    return np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * sigma ** 2))


# ---- camera ------------------------------------------------------------------------------------------------------------
def _camera_points(T, pts):
    T, p = _f64(T).reshape(-1, 4, 4), _f64(pts).reshape(-1, 3)
    with np.errstate(invalid="ignore"):                                      # 0 * inf of a non-finite point: NaN, dropped later
        return p @ np.swapaxes(T[:, :3, :3], 1, 2) + T[:, None, :3, 3]      # [N,M,3]


def _pixel_coordinates(cam, K):
    K = _f64(K)
    ok = cam[..., 2] > Z_MIN
    with np.errstate(all="ignore"):
        z = np.where(ok, cam[..., 2], 1.0)
        uf, vf = cam[..., 0] / z * K[0, 0] + K[0, 2], cam[..., 1] / z * K[1, 1] + K[1, 2]
        ok = ok & (np.abs(uf) < UV_MAX) & (np.abs(vf) < UV_MAX)            # NaN and inf compare false
    return np.where(ok, uf, 0.0), np.where(ok, vf, 0.0), ok


def splat(T, pts, K, H, W, radius):
    """Depth image of a point cloud: every usable point writes its z' to the (2r+1)^2 pixels around
    (floor(u_f), floor(v_f)), the smallest z' per pixel wins, 0 where nothing lands."""
    cam = _camera_points(T, pts)[0]
    uf, vf, ok = _pixel_coordinates(cam, K)
    out = np.full((H, W), np.inf)
    for m in np.flatnonzero(ok):
        u, v = int(np.floor(uf[m])), int(np.floor(vf[m]))
        r0, r1, c0, c1 = max(v - radius, 0), min(v + radius + 1, H), max(u - radius, 0), min(u + radius + 1, W)
        if r0 < r1 and c0 < c1:
            out[r0:r1, c0:c1] = np.minimum(out[r0:r1, c0:c1], cam[m, 2])
    return np.where(np.isinf(out), 0.0, out)


def project(T, pts, K):
    """-> uv [N,M,2] int64 = trunc(u_f, v_f), (-1,-1) for an unusable point; z' [N,M]"""
    cam = _camera_points(T, pts)
    uf, vf, ok = _pixel_coordinates(cam, K)
    uv = np.stack([np.trunc(uf), np.trunc(vf)], -1).astype(np.int64)
    return np.where(ok[..., None], uv, -1), cam[..., 2]


def _in_frame(uv, H, W):
    return (uv[..., 0] >= 0) & (uv[..., 0] < W) & (uv[..., 1] >= 0) & (uv[..., 1] < H)


def inconst_count(depth, T, pts, K, margin):
    """per hypothesis: points in the frame whose pixel has a depth > 0 that lies more than `margin` behind the point"""
    depth = _f64(depth)
    uv, z = project(T, pts, K)
    inb = _in_frame(uv, *depth.shape)
    d = depth[np.where(inb, uv[..., 1], 0), np.where(inb, uv[..., 0], 0)]
    return (inb & (d > 0) & (d - z > float(margin))).sum(1)


def mask_fraction(mask, T, pts, K):
    """per hypothesis: the share of ALL M points that project into the frame onto a set pixel of `mask`"""
    mask = _f64(mask)
    uv, _ = project(T, pts, K)
    inb = _in_frame(uv, *mask.shape)
    hit = mask[np.where(inb, uv[..., 1], 0), np.where(inb, uv[..., 0], 0)] * inb
    return hit.sum(1) / uv.shape[1]


# ---- visibility and the two IoUs ----------------------------------------------------------------------------------------
def visibility(d_obs, d_pred, gt, gt_visib, delta):
    """-> predicted mask, visible mask, (|pred & gt|, |pred | gt|, |visib & gt_visib|, |visib | gt_visib|);
    a missing ground-truth mask counts as empty."""
    dob, dpr = _f64(d_obs), _f64(d_pred)
    with np.errstate(invalid="ignore"):
        pm = dpr > 0
        vm = ((dpr - dob <= float(delta)) | (dob == 0)) & pm
    g = np.zeros(pm.shape, bool) if gt is None else np.asarray(gt) > 0
    gv = np.zeros(pm.shape, bool) if gt_visib is None else np.asarray(gt_visib) > 0
    return pm, vm, (int((pm & g).sum()), int((pm | g).sum()), int((vm & gv).sum()), int((vm | gv).sum()))


def ratio(num, den):
    return num / den if den > 0 else float("nan")


# ---- ADD / ADI ----------------------------------------------------------------------------------------------------------
def add_adi(T, T_gt, pts, symmetric, chunk=256):
    """ADD = mean_i |T p_i - T_gt p_i|; ADI = mean_i min_j |T p_i - T_gt p_j| (rows of `chunk` points at a time)."""
    est = _camera_points(T, pts)
    ref = _camera_points(T_gt, pts)[0]
    if not symmetric:
        return np.sqrt(((est - ref[None]) ** 2).sum(-1)).mean(1)
    out = np.zeros(est.shape[0])
    for n in range(est.shape[0]):
        for i in range(0, est.shape[1], chunk):
            d2 = ((est[n, i:i + chunk, None, :] - ref[None, :, :]) ** 2).sum(-1)
            out[n] += np.sqrt(d2.min(1)).sum()
    return out / est.shape[1]
