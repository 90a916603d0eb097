"""ScoreDataset.getPointNetData and projectPointsUv -- host-side mirrors of the Zephyr featurizer.

Reference interface (the implementation lives in the un-vendored `zephyr` package; SPEC.md states what
this build computes):
  ScoreDataset([], "", name, zephyr_args, mode='test'), .dim_point
                                   /root/reference/python/ossid/scripts/online_learning.py:206-207
  dataset.getPointNetData(scoring_data, return_uv_original=True) -> (point_x, uv_original), filtering
  scoring_data['transforms'] / ['pp_err'] in place           utils/zephyr_utils.py:31,39-43
  zephyr.utils.projectPointsUv(pose_hypos, model_points, meta_data) -> int [N, M, 2]
                                                              utils/zephyr_utils.py:58
All device work goes through libossid_hip.so (include/ossid_hip.h); torch only owns the buffers.
"""
import numpy as np
import torch

from .. import _lib

DIM_POINT = 8  # (x, y, 0, dH, dS, dV, dD, cosN)
INCONST_MARGIN = 0.02  # metres, SPEC.md 3.4


def _dev(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("the OSSID hot path needs a GPU: torch.cuda.is_available() is False and there is no "
                           "CPU fallback")
    return _lib._dev()


def _f32(x, dev):
    """numpy / torch (any float dtype, any device) -> contiguous float32 tensor on dev."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()


def _cam(meta):
    return tuple(float(np.float32(meta[k])) for k in ("camera_fx", "camera_fy", "camera_cx", "camera_cy"))


class FrameCache:
    """Device-resident staged frame + model table, so a caller scoring several hypothesis sets against the same
    frame/object uploads and converts them once (bigger batches, fewer host round trips)."""

    def __init__(self, rgbd, tab, H, W, M):
        self.rgbd, self.tab, self.H, self.W, self.M = rgbd, tab, H, W, M


def _need(ok, what):
    if not ok:
        raise ValueError(what)


def _check(t, name, shape, dtype=torch.float32, dev=None):
    """t is a contiguous tensor of `dtype` whose shape matches `shape` (None: any extent) on `dev` (None: any device).
    Host-side only: nothing is launched and nothing is read back."""
    _need(torch.is_tensor(t), "%s: a torch tensor is required, got %s" % (name, type(t).__name__))
    want = "[%s]" % ",".join("*" if d is None else str(d) for d in shape)
    _need(t.dim() == len(shape) and all(d is None or int(s) == d for s, d in zip(t.shape, shape)),
          "%s: shape %s required, got %s" % (name, want, list(t.shape)))
    _need(t.dtype == dtype, "%s: %s required, got %s" % (name, dtype, t.dtype))
    _need(t.is_contiguous(), "%s: a contiguous tensor is required (strides %s)" % (name, list(t.stride())))
    _need(dev is None or t.device == dev, "%s: on %s, the other operands on %s" % (name, t.device, dev))
    return t


def _check_scene(rgbd, transforms, tab):
    """the operands inconst_count and featurize share -> (H, W, N, M)"""
    _check(rgbd, "rgbd", (None, None, 4))
    _need(rgbd.is_cuda, "rgbd: a staged frame on the GPU is required, got one on %s" % rgbd.device)
    H, W = int(rgbd.shape[0]), int(rgbd.shape[1])
    _need(H >= 1 and W >= 1, "rgbd: an empty frame %s" % list(rgbd.shape))
    _check(transforms, "transforms", (None, 4, 4), dev=rgbd.device)
    _check(tab, "tab", (None, 12), dev=rgbd.device)
    _need(int(tab.shape[0]) >= 1, "tab: at least one model point is required")
    return H, W, int(transforms.shape[0]), int(tab.shape[0])


def _as_tensor(x):
    return torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x


def stage_frame(img, depth, dev=None, blur=False, out=None):
    """img: uint8 [H,W,3] (blurred on the GPU when blur) or float [H,W,3] in [0,1]; depth [H,W] metres (numpy or torch,
    any float dtype, any device: converted). -> rgbd [H,W,4] float32 on dev (`out` if given). Everything is validated
    before the first launch; a ValueError leaves `out` untouched."""
    dev = _dev(dev)
    img, depth = _as_tensor(img), _as_tensor(depth)
    _need(torch.is_tensor(img) and img.dim() == 3 and int(img.shape[2]) == 3,
          "img: [H,W,3] required, got %s" % (list(img.shape) if torch.is_tensor(img) else type(img).__name__))
    H, W = int(img.shape[0]), int(img.shape[1])
    _need(H >= 1 and W >= 1, "img: an empty image %s" % list(img.shape))
    _need(img.dtype == torch.uint8 or img.dtype.is_floating_point, "img: uint8 or a float type required, got %s" % img.dtype)
    _need(torch.is_tensor(depth) and tuple(depth.shape) == (H, W),
          "depth: [%d,%d] required to match img, got %s" % (H, W, list(depth.shape) if torch.is_tensor(depth) else None))
    _need(depth.dtype.is_floating_point, "depth: a float type required, got %s" % depth.dtype)
    _need(img.dtype == torch.uint8 or not blur,
          "blur is defined on the uint8 image (cv2.GaussianBlur, zephyr_utils.py:13)")
    if out is not None:
        _check(out, "out", (H, W, 4), dev=dev)
    depth = _f32(depth, dev)
    rgbd = torch.empty(H, W, 4, dtype=torch.float32, device=dev) if out is None else out
    with torch.cuda.device(dev):
        if img.dtype == torch.uint8:
            img = img.to(dev).contiguous()
            rc = _lib.fn("ossid_zephyr_prep_frame_u8")(img.data_ptr(), depth.data_ptr(), H, W, int(bool(blur)),
                                                       rgbd.data_ptr(), _lib.stream())
        else:
            img = _f32(img, dev)
            rc = _lib.fn("ossid_zephyr_prep_frame_f32")(img.data_ptr(), depth.data_ptr(), H, W, rgbd.data_ptr(),
                                                        _lib.stream())
    _lib.check(rc, "ossid_zephyr_prep_frame")
    return rgbd


def stage_model(points, normals, colors, dev=None, out=None):
    """points, normals, colors [M,3] (numpy or torch, any float dtype, any device: converted), M >= 1 -> the model table
    [M,12] float32 on dev (`out` if given). Validated before the first launch; a ValueError leaves `out` untouched."""
    dev = _dev(dev)
    points, normals, colors = _as_tensor(points), _as_tensor(normals), _as_tensor(colors)
    _need(torch.is_tensor(points) and points.dim() == 2 and int(points.shape[1]) == 3 and int(points.shape[0]) >= 1,
          "points: [M,3] with M >= 1 required, got %s" % (list(points.shape) if torch.is_tensor(points) else None))
    M = int(points.shape[0])
    for name, t in (("points", points), ("normals", normals), ("colors", colors)):
        _need(torch.is_tensor(t) and tuple(t.shape) == (M, 3),
              "%s: [%d,3] required to match points, got %s" % (name, M, list(t.shape) if torch.is_tensor(t) else None))
        _need(t.dtype.is_floating_point, "%s: a float type required, got %s" % (name, t.dtype))
    if out is not None:
        _check(out, "out", (M, 12), dev=dev)
    p, n, c = _f32(points, dev), _f32(normals, dev), _f32(colors, dev)
    tab = torch.empty(M, 12, dtype=torch.float32, device=dev) if out is None else out
    with torch.cuda.device(dev):
        rc = _lib.fn("ossid_zephyr_prep_model")(p.data_ptr(), n.data_ptr(), c.data_ptr(), M, tab.data_ptr(),
                                                _lib.stream())
    _lib.check(rc, "ossid_zephyr_prep_model")
    return tab


def inconst_count(rgbd, transforms, tab, cam, margin=INCONST_MARGIN, out=None):
    """rgbd [H,W,4], transforms [N,4,4], tab [M,12]: float32, contiguous, on one GPU -> free-space-violation counts [N]
    int32 (`out` if given). The kernel reads raw pointers, so anything else is refused with a ValueError before the
    launch."""
    H, W, N, M = _check_scene(rgbd, transforms, tab)
    _need(len(cam) == 4, "cam: (fx, fy, cx, cy) required")
    if out is not None:
        _check(out, "out", (N,), torch.int32, rgbd.device)
    cnt = torch.empty(N, dtype=torch.int32, device=rgbd.device) if out is None else out
    with torch.cuda.device(rgbd.device):
        rc = _lib.fn("ossid_zephyr_inconst_count")(rgbd.data_ptr(), H, W, transforms.data_ptr(), N, tab.data_ptr(), M,
                                                   *cam, float(margin), cnt.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_zephyr_inconst_count")
    return cnt


def featurize(rgbd, transforms, tab, cam, sel=None, interp=0, want_uv=True, out_px=None, out_uv=None):
    """-> point_x [N', M, 8] float32, uv_original [N', M, 2] int32 (or None); into out_px / out_uv if given.
    rgbd [H,W,4], transforms [N,4,4], tab [M,12]: float32, contiguous, on one GPU. sel: None (all hypotheses, N' = N) or a
    one-dimensional contiguous integer tensor on that GPU; the kernel reads int32, an int64 selection (what
    torch.nonzero returns) is CONVERTED to int32, any other dtype is refused. The values of sel (0 <= sel < N) are the
    caller's responsibility: checking them would need a read-back. interp: 0 nearest pixel, 1 bilinear. Everything is
    validated before the first launch; a ValueError leaves out_px / out_uv untouched."""
    H, W, N, M = _check_scene(rgbd, transforms, tab)
    _need(len(cam) == 4, "cam: (fx, fy, cx, cy) required")
    _need(interp in (0, 1), "interp: 0 (nearest pixel) or 1 (bilinear) required, got %r" % (interp,))
    dev = rgbd.device
    if sel is not None:
        _need(torch.is_tensor(sel) and sel.dtype in (torch.int32, torch.int64),
              "sel: an int32 (or int64, converted) tensor required, got %s" % (sel.dtype if torch.is_tensor(sel) else
                                                                               type(sel).__name__))
        _check(sel, "sel", (None,), sel.dtype, dev)
        _need(N >= 1 or int(sel.shape[0]) == 0, "sel: selects from no hypotheses")
    n = int(sel.shape[0]) if sel is not None else N
    if out_px is not None:
        _check(out_px, "out_px", (n, M, DIM_POINT), dev=dev)
    if out_uv is not None:
        _need(want_uv, "out_uv given but want_uv is False")
        _check(out_uv, "out_uv", (n, M, 2), torch.int32, dev)
    if sel is not None and sel.dtype == torch.int64:
        sel = sel.to(torch.int32)
    px = torch.empty(n, M, DIM_POINT, dtype=torch.float32, device=dev) if out_px is None else out_px
    uv = (torch.empty(n, M, 2, dtype=torch.int32, device=dev) if out_uv is None else out_uv) if want_uv else None
    with torch.cuda.device(dev):
        rc = _lib.fn("ossid_zephyr_featurize")(rgbd.data_ptr(), H, W, transforms.data_ptr(),
                                               None if sel is None else sel.data_ptr(), n, tab.data_ptr(), M, *cam,
                                               int(interp), px.data_ptr(), None if uv is None else uv.data_ptr(),
                                               _lib.stream())
    _lib.check(rc, "ossid_zephyr_featurize")
    return px, uv


PROJECT_MAX_HYPOS = 65535  # ossid_zephyr_project_uv puts the hypotheses on grid.y


def project_uv(T, P, cam):
    """T f32 [N,4,4], P f32 [M,3] on one device, cam = (fx, fy, cx, cy) -> uv int32 [N,M,2] on that device; any N: the
    entry point is called on at most PROJECT_MAX_HYPOS hypotheses at a time."""
    N, M = int(T.shape[0]), int(P.shape[0])
    uv = torch.empty(N, M, 2, dtype=torch.int32, device=T.device)
    if N and M:
        with torch.cuda.device(T.device):
            for n0 in range(0, N, PROJECT_MAX_HYPOS):
                n = min(PROJECT_MAX_HYPOS, N - n0)
                rc = _lib.fn("ossid_zephyr_project_uv")(T[n0:n0 + n].data_ptr(), P.data_ptr(), n, M, *cam,
                                                        uv[n0:n0 + n].data_ptr(), _lib.stream())
                _lib.check(rc, "ossid_zephyr_project_uv")
    return uv


def projectPointsUv(pose_hypos, model_points, meta_data):
    """zephyr.utils.projectPointsUv: (N,4,4), (M,3), camera dict -> integer pixel coordinates [N, M, 2]
    (numpy int64, [..., 0] = x / column, [..., 1] = y / row), as utils/zephyr_utils.py:58-65 consumes them."""
    dev = _dev()
    T = _f32(pose_hypos, dev).reshape(-1, 4, 4)
    P = _f32(model_points, dev)
    return project_uv(T, P, _cam(meta_data)).cpu().numpy().astype(np.int64)


class ScoreDataset:
    """Only the surface the OSSID loop touches: the constructor, .dim_point and getPointNetData."""

    def __init__(self, datapoints, dataset_root, dataset_name, args, mode="train"):
        self.datapoints, self.dataset_root, self.dataset_name = datapoints, dataset_root, dataset_name
        self.args, self.mode = args, mode
        name = getattr(args, "dataset", "HSVD_diff_uv_norm")
        if name != "HSVD_diff_uv_norm" or not getattr(args, "no_valid_proj", True) or \
                not getattr(args, "no_valid_depth", True):
            raise NotImplementedError(
                "only dataset='HSVD_diff_uv_norm' with no_valid_proj and no_valid_depth is built "
                "(the configuration of scripts/online_learning.py:191-196)")
        self.inconst_ratio_th = float(getattr(args, "inconst_ratio_th", 100))
        self.interp = int(getattr(args, "interp", 0))  # build option: 0 nearest pixel, 1 bilinear (SPEC.md 3.3)
        self.dim_point = DIM_POINT

    def __len__(self):
        return len(self.datapoints)

    def getPointNetData(self, data, return_uv_original=False):
        with torch.no_grad():
            dev = _dev()
            cam = _cam(data["meta_data"])
            cache = data.get("_frame_cache")
            if cache is None:
                blur = bool(data.get("_blur_on_device", False))
                rgbd = stage_frame(data["img"], data["depth"], dev, blur=blur)
                tab = stage_model(data["model_points"], data["model_normals"], data["model_colors"], dev)
            else:
                rgbd, tab = cache.rgbd, cache.tab
            T = _f32(data["transforms"], dev).reshape(-1, 4, 4)
            N = int(T.shape[0])
            sel = None
            if self.mode == "test" and self.inconst_ratio_th < 100 and N > 0:
                # drop hypotheses with too many free-space violations; the caller reads the filtered
                # transforms / pp_err back from the dict (utils/zephyr_utils.py:39-43)
                cnt = inconst_count(rgbd, T, tab, cam)
                keep = cnt.double() * 100.0 <= self.inconst_ratio_th * float(tab.shape[0])
                sel = torch.nonzero(keep).flatten().to(torch.int32)
                keep_cpu = keep.cpu()
                tr = data["transforms"]
                data["transforms"] = tr[keep_cpu.to(tr.device)] if torch.is_tensor(tr) else tr[keep_cpu.numpy()]
                pe = data.get("pp_err")
                if pe is not None:
                    data["pp_err"] = pe[keep_cpu.to(pe.device)] if torch.is_tensor(pe) else \
                        np.asarray(pe)[keep_cpu.numpy()]
            px, uv = featurize(rgbd, T, tab, cam, sel=sel, interp=self.interp, want_uv=return_uv_original)
            if return_uv_original:
                data["uv_original"] = uv
                return px, uv
            return px
