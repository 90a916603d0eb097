"""Zephyr scoring entry points with the call signatures of ossid.utils.zephyr_utils
(/root/reference/python/ossid/utils/zephyr_utils.py:10-47 networkInference, :49-71 filterHypoByMask), so
scripts/online_learning.py:464 can call them unchanged.

What differs from the reference is where the work happens: the 5x5 blur + /255 that the reference does with
OpenCV on the host (:13-14) is part of the frame-staging kernel, the featurizer runs on the GPU instead of the
CPU, point_x goes from featurizer to scorer without leaving HBM, and the mask test of filterHypoByMask is a
device-side gather over the projected pixels.
"""
import time

import numpy as np
import torch

from .hostutil import K2meta, to_np
from .zephyr import score_dataset as _sd

_MODEL_KEYS = ("model_points", "model_colors", "model_normals")


ADI_MAX_POINTS = 150 * 1024 // 24    # ossid_pose_errors: 24 bytes of LDS per ground-truth point, 150 KiB at the most


def _as_tensor(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))


def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def _need_points(p):
    if len(_shape(p)) != 2 or _shape(p)[1] != 3:
        raise ValueError("model_points must be [M,3], got %s" % (_shape(p),))


def _need_poses(name, T):
    if len(_shape(T)) < 2 or _shape(T)[-2:] != (4, 4):
        raise ValueError("%s must be [...,4,4], got %s" % (name, _shape(T)))


def networkInference(model, dataset, data, return_time=False):
    """data: img uint8 [H,W,3], depth [H,W] (m), cam_K [3,3], pose_hypos [N,4,4], model_points/colors/normals [M,3],
    optional pp_err [N].  Returns (poses [N',4,4], scores [N',1], pp_err [N'], uv_original [N',M,2][, seconds])."""
    frame = _as_tensor(data["img"])
    pack = {"img": frame, "_blur_on_device": frame.dtype == torch.uint8,
            "depth": _as_tensor(data["depth"]), "transforms": _as_tensor(data["pose_hypos"]),
            "meta_data": K2meta(data["cam_K"])}
    for key in _MODEL_KEYS:
        pack[key] = _as_tensor(data[key])
    pack["pp_err"] = data["pp_err"] if "pp_err" in data else torch.zeros(len(data["pose_hypos"]))

    with torch.no_grad():
        t0 = time.time()
        point_x, uv_original = dataset.getPointNetData(pack, return_uv_original=True)
        scores = to_np(model({"point_x": point_x.to(model.device)}))  # the D2H copy synchronises the stream
        elapsed = time.time() - t0

    # getPointNetData drops hypotheses with too many free-space violations and leaves the survivors in the dict
    out = (to_np(pack["transforms"]), scores, pack["pp_err"], uv_original)
    return out + (elapsed,) if return_time else out


def networkInferenceMany(model, dataset, frames, streams=2, return_time=False):
    """ADDITIVE API: networkInference for a list of frames (dicts as networkInference takes), kept `streams` frames in
    flight on alternating HIP streams: the VALU/LDS-bound sampling kernels of one frame (FPS, ball query) overlap the
    MFMA-bound MLP kernels of another (+3.6 % hypotheses/s measured at 1000 x 2048, `bench.py --streams 2`). Results
    are exactly those of per-frame networkInference calls (each frame's kernels run in order on its own stream, the
    scorer's scratch is per stream); device->host copies happen once, after the last launch. Returns a list of the
    per-frame tuples."""
    dev = model.device
    pool = [torch.cuda.Stream(device=dev) for _ in range(max(1, int(streams)))]
    cur = torch.cuda.current_stream(dev)
    pending = []
    t0 = time.time()
    with torch.no_grad():
        for i, data in enumerate(frames):
            frame = _as_tensor(data["img"])
            pack = {"img": frame, "_blur_on_device": frame.dtype == torch.uint8,
                    "depth": _as_tensor(data["depth"]), "transforms": _as_tensor(data["pose_hypos"]),
                    "meta_data": K2meta(data["cam_K"])}
            for key in _MODEL_KEYS:
                pack[key] = _as_tensor(data[key])
            pack["pp_err"] = data["pp_err"] if "pp_err" in data else torch.zeros(len(data["pose_hypos"]))
            st = pool[i % len(pool)]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                point_x, uv_original = dataset.getPointNetData(pack, return_uv_original=True)
                scores = model({"point_x": point_x.to(dev)})
            pending.append((pack, scores, uv_original))
        for st in pool:
            cur.wait_stream(st)
        out = []
        for pack, scores, uv in pending:
            res = (to_np(pack["transforms"]), to_np(scores), pack["pp_err"], uv)
            out.append(res)
    elapsed = time.time() - t0
    return [r + (elapsed / max(1, len(out)),) for r in out] if return_time else out


def filterHypoByMask(model_points, meta_data, pose_hypos, mask, th=0.5):
    """Boolean [N]: hypotheses whose model points land inside `mask` (h x w, {0,1}) for more than a fraction th."""
    _need_points(model_points)
    _need_poses("pose_hypos", pose_hypos)
    if len(_shape(mask)) != 2 or min(_shape(mask)) <= 0:
        raise ValueError("mask must be [h,w], got %s" % (_shape(mask),))
    dev = _sd._dev()
    T = _sd._f32(pose_hypos, dev).reshape(-1, 4, 4)
    P = _sd._f32(model_points, dev)
    N, M = int(T.shape[0]), int(P.shape[0])
    if N == 0 or M == 0:
        return np.zeros(N, dtype=bool)
    uv = _sd.project_uv(T, P, _sd._cam(meta_data))
    m = (mask if torch.is_tensor(mask) else _as_tensor(np.asarray(mask))).to(dev)
    h, w = m.shape
    x, y = uv[..., 0].long(), uv[..., 1].long()
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    hit = m[y.clamp(0, h - 1), x.clamp(0, w - 1)].to(torch.float64) * inside
    return (hit.sum(-1) / float(M) > th).cpu().numpy()


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def select_instances(poses, scores, model_points, max_instances, sep, symmetries=None, min_score=None):
    """ADDITIVE API (SPEC.md section 16): from N scored poses the best `max_instances` that are different objects in space --
    greedy non-maximum suppression under the MSSD distance of 8.7 (max over model_points, min over `symmetries`), so two
    poses of a symmetric object related by a symmetry are one instance. poses [N,4,4], scores [N] or [N,1], model_points
    [M,3], symmetries f64 [S,4,4] in the unit of model_points (None: the identity), sep a length in that unit: a candidate
    within sep of a pick belongs to it. min_score (None: no bound): candidates below it are never picked.
    Returns (selected int32 [K], count int32 [1], owner int32 [N]) as device tensors -- the picks in order (-1 past the
    last), their number, and per candidate the round that took it (-1 = never) -- without synchronising. numpy arrays or
    tensors. ValueError before the device is touched for what does not fit."""
    _need_poses("poses", poses)
    _need_points(model_points)
    if len(_shape(poses)) != 3:
        raise ValueError("poses must be [N,4,4], got %s" % (_shape(poses),))
    N, M = _shape(poses)[0], _shape(model_points)[0]
    sshape = _shape(scores)
    if sshape not in ((N,), (N, 1)):
        raise ValueError("scores must be [N] or [N,1] with N = %d, got %s" % (N, sshape))
    for name, a in (("poses", poses), ("scores", scores), ("model_points", model_points)):
        dt = str(a.dtype) if hasattr(a, "dtype") else ""
        if "float" not in dt:
            raise ValueError("%s must be a floating-point array, got %s" % (name, dt or type(a).__name__))
    K = int(max_instances)
    if K != max_instances or not 1 <= K <= _sd._lib.BOP_MAX_INSTANCES:
        raise ValueError("max_instances must be an integer in [1, %d], got %r" % (_sd._lib.BOP_MAX_INSTANCES, max_instances))
    if not 1 <= N <= _sd._lib.SELECT_MAX_POSES:
        raise ValueError("select_instances takes 1 to %d poses, got %d" % (_sd._lib.SELECT_MAX_POSES, N))
    if not 1 <= M <= 1 << 22:
        raise ValueError("select_instances takes 1 to 2^22 model_points, got %d" % M)
    sep = float(sep)
    if not (np.isfinite(sep) and sep >= 0.0):
        raise ValueError("sep must be finite and >= 0, got %r" % sep)
    min_score = -np.inf if min_score is None else float(min_score)
    if np.isnan(min_score):
        raise ValueError("min_score must not be NaN")
    if symmetries is None:
        symmetries = np.eye(4, dtype=np.float64)[None]
    if len(_shape(symmetries)) != 3 or _shape(symmetries)[1:] != (4, 4) or not 1 <= _shape(symmetries)[0] <= _sd._lib.BOP_MAX_SYMMETRIES:
        raise ValueError("symmetries must be [S,4,4] with 1 <= S <= %d, got %s" % (_sd._lib.BOP_MAX_SYMMETRIES, _shape(symmetries)))
    if not torch.is_tensor(poses) or not poses.is_cuda:                      # a device tensor is the caller's to vouch for
        if not np.isfinite(_host(poses)).all():
            raise ValueError("poses must be finite")
    dev = _sd._dev()
    T = _as_tensor(poses).to(dev, torch.float64).reshape(N, 4, 4).contiguous()
    sc = _as_tensor(scores).to(dev, torch.float32).reshape(N).contiguous()
    P = _as_tensor(model_points).to(dev, torch.float32).contiguous()
    Sm = _as_tensor(symmetries).to(dev, torch.float64).contiguous()
    out = torch.empty(K + 1 + N, dtype=torch.int32, device=dev)
    keys = torch.empty(K, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = _sd._lib.fn("ossid_pose_select")(T.data_ptr(), sc.data_ptr(), N, P.data_ptr(), M, Sm.data_ptr(), int(Sm.shape[0]), K,
                                              sep, min_score, out.data_ptr(), out.data_ptr() + 4 * K, out.data_ptr() + 4 * (K + 1),
                                              keys.data_ptr(), _sd._lib.stream())
    _sd._lib.check(rc, "ossid_pose_select")
    return out[:K], out[K:K + 1], out[K + 1:]


def pose_errors(pose_hypos, pose_gt, model_points, symmetric=False):
    """ADD (symmetric=False) or ADI (True) of every hypothesis against the ground-truth pose, float64 numpy [N]:
    the device-side form of online_learning.py:452's per-hypothesis Python loop over zephyr.utils.metrics.add / adi."""
    _need_poses("pose_hypos", pose_hypos)
    if _shape(pose_gt) != (4, 4):
        raise ValueError("pose_gt must be [4,4], got %s" % (_shape(pose_gt),))
    _need_points(model_points)
    if _shape(model_points)[0] < 1:
        raise ValueError("model_points must hold at least one point")
    if symmetric and _shape(model_points)[0] > ADI_MAX_POINTS:
        raise ValueError("ADI takes at most %d model_points (the ground-truth cloud is kept in LDS), got %d"
                         % (ADI_MAX_POINTS, _shape(model_points)[0]))
    dev = _sd._dev()
    T = _as_tensor(np.asarray(pose_hypos, dtype=np.float64)).to(dev).reshape(-1, 4, 4).contiguous()
    G = _as_tensor(np.asarray(pose_gt, dtype=np.float64)).to(dev).reshape(4, 4).contiguous()
    P = _as_tensor(np.asarray(model_points, dtype=np.float64)).to(dev).contiguous()
    N, M = int(T.shape[0]), int(P.shape[0])
    err = torch.empty(N, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _sd._lib.fn("ossid_pose_errors")(T.data_ptr(), G.data_ptr(), P.data_ptr(), N, M, int(bool(symmetric)),
                                              err.data_ptr(), _sd._lib.stream())
    _sd._lib.check(rc, "ossid_pose_errors")
    return err.cpu().numpy()
