"""Keypoint-feature pose hypotheses on the device (csrc/features.hip, SPEC.md section 11), in place of zephyr's SIFT
featurization that scripts/online_learning.py reaches with --use_sift_hypos:

    obj = FeatureModel(dataset_root, is_sym, args, create_index=True); obj.construct(obj_id, obj_path, dataset_camera)  :52-76
    keypoints, features, cloud, frames = featurizeScene(img, dist_im, dtoid_mask, scene_meta, [11], [11])             :427
    poses_sift, match_aux = featured_objects[obj_id].match(features, frames, mat_gt)                                   :435

zephyr's source is absent, so this is this build's own definition: a difference-of-Gaussians detector in integer
arithmetic, a 4 x 4 x 8 gradient descriptor (i8), one oriented 3-D frame per keypoint so that a single match gives a full
pose, nearest-neighbour matching on the i8 matrix cores and SPEC 6.6's clustering of the matched poses.

featurizeScene / FeatureModel.match are the drop-ins (host arrays in and out); featurize and FeatureModel.find_hypotheses
are the device forms that OnlineStream uses: one launch chain, no host copy.
"""
import numpy as np
import torch

from . import _lib, hostutil
from .render import _intrinsics

CONTRAST = 192                      # SPEC 11.2: |D| >= 3 grey levels (6 fractional bits)
OCTAVES = 3
MAX_KEYPOINTS = _lib.FEAT_MAX_KEYPOINTS


def _call(name, *args):
    with torch.cuda.device(_lib._dev()):
        rc = _lib.fn(name)(*args)
    _lib.check(rc, name)


def _u8(a, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev).to(torch.uint8).contiguous()


def featurize(img, depth, mask, cam_K, contrast=CONTRAST, max_keypoints=None, octaves=OCTAVES):
    """SPEC 11.1-11.5 on one frame: img u8 [H,W,3] RGB, depth f32 [H,W] (0 = invalid), mask [H,W] (pixel used iff mask &&
    depth > 0), cam_K [3,3] -> dict of device tensors: "descriptors" u8 [cap,128] (values 0..127), "frames" f64 [cap,4,4],
    "keypoints" int32 [cap,4] = (octave, level, y, x), "count" int32 [2] = (keypoints found, 1 iff over the cap), "ok" u8
    [cap] (0 = dropped, its rows are zero), "bins" int32 [cap], "pyramid" (int32, opaque). Rows past count[0] are
    unspecified. Nothing is copied to the host: check_count raises on a frame over the cap."""
    dev = _lib._dev()
    cap = _lib.FEAT_MAX_KEYPOINTS if max_keypoints is None else int(max_keypoints)
    if not 1 <= cap <= _lib.FEAT_MAX_KEYPOINTS:
        raise ValueError("featurize: max_keypoints must lie in [1, %d], got %r" % (_lib.FEAT_MAX_KEYPOINTS, max_keypoints))
    if int(contrast) < 1:
        raise ValueError("featurize: contrast must be >= 1, got %r" % (contrast,))
    I = _u8(img, dev)
    if I.dim() != 3 or I.shape[2] != 3:
        raise ValueError("featurize: img must be u8 [H,W,3], got %s" % (tuple(I.shape),))
    H, W = int(I.shape[0]), int(I.shape[1])
    D = (depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(np.asarray(depth, dtype=np.float32))))
    D = D.to(dev, torch.float32).contiguous()
    M = _u8(mask, dev)
    if tuple(D.shape) != (H, W) or tuple(M.shape) != (H, W):
        raise ValueError("featurize: depth and mask must both be [H,W] = [%d,%d]" % (H, W))
    fx, fy, cx, cy = _intrinsics(cam_K)
    pb = int(_lib.fn("ossid_feat_pyramid_bytes")(H, W, int(octaves)))
    if pb == 0:
        raise ValueError("featurize: frame %d x %d with %r octaves is outside what this build takes" % (H, W, octaves))
    st = _lib.stream()
    pyr = torch.empty(pb // 4, dtype=torch.int32, device=dev)
    _call("ossid_feat_pyramid", I.data_ptr(), H, W, int(octaves), pyr.data_ptr(), pb, st)
    wb = int(_lib.fn("ossid_feat_detect_workspace_bytes")(H, W, int(octaves)))
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    kps = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    _call("ossid_feat_detect", pyr.data_ptr(), H, W, int(octaves), D.data_ptr(), M.data_ptr(), int(contrast), cap,
          ws.data_ptr(), wb, kps.data_ptr(), count.data_ptr(), st)
    bins = torch.empty(cap, dtype=torch.int32, device=dev)
    desc = torch.empty(cap, 128, dtype=torch.uint8, device=dev)
    frames = torch.empty(cap, 4, 4, dtype=torch.float64, device=dev)
    ok = torch.empty(cap, dtype=torch.uint8, device=dev)
    _call("ossid_feat_describe", pyr.data_ptr(), H, W, int(octaves), D.data_ptr(), fx, fy, cx, cy, kps.data_ptr(),
          count.data_ptr(), cap, bins.data_ptr(), desc.data_ptr(), frames.data_ptr(), ok.data_ptr(), st)
    return {"descriptors": desc, "frames": frames, "keypoints": kps, "count": count, "ok": ok, "bins": bins, "pyramid": pyr,
            "cap": cap, "hw": (H, W), "contrast": int(contrast)}


def check_count(feat):
    """count of a featurize (device) -> the number of keypoints on the host; raises when the frame was over the cap."""
    n = int(feat["count"][0].item())
    if n > feat["cap"]:
        raise ValueError("featurize: contrast=%d keeps %d keypoints, more than the %d this call takes; raise contrast or "
                         "shrink the mask" % (feat["contrast"], n, feat["cap"]))
    return n


def match_descriptors(desc_s, ok_s, count, desc_m):
    """SPEC 11.7: scene descriptors u8 [cap,128], ok u8 [cap], count int32 [>=1] (device), model descriptors u8 [Nm,128] ->
    device int32 [cap,3] = (best model index, d2, weight); (-1, 0, 0) for a row with ok = 0. Rows past count are unspecified."""
    dev = desc_s.device
    cap, Nm = int(desc_s.shape[0]), int(desc_m.shape[0])
    wb = int(_lib.fn("ossid_feat_match_workspace_bytes")(cap))
    if wb == 0:
        raise ValueError("match: %d scene rows is outside [1, %d]" % (cap, _lib.FEAT_MAX_KEYPOINTS))
    if Nm > _lib.FEAT_MAX_MODEL_FEATURES:
        raise ValueError("match: %d model features, more than the %d this build takes" % (Nm, _lib.FEAT_MAX_MODEL_FEATURES))
    ws = torch.empty(wb // 8, dtype=torch.int64, device=dev)
    out = torch.empty(cap, 3, dtype=torch.int32, device=dev)
    _call("ossid_feat_match", desc_s.data_ptr(), ok_s.data_ptr(), count.data_ptr(), cap, desc_m.data_ptr() if Nm else None, Nm,
          ws.data_ptr(), wb, out.data_ptr(), _lib.stream())
    return out


def box_diameter(vertices):
    """SPEC 6.1's D: the f32 diagonal of the bounding box of f32 vertices (a tensor or an array [V,3])."""
    P = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.asarray(vertices, dtype=np.float64).astype(np.float32))
    lo, hi = P.min(0).values.cpu().numpy().astype(np.float32), P.max(0).values.cpu().numpy().astype(np.float32)
    e = (hi - lo).astype(np.float32)
    return np.float32(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


def _rigid_inverse(T):
    """[R | t] -> [R^T | -(R^T t)], f64, the written order (SPEC 11.6)."""
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    for j in range(3):
        out[j, 3] = -((R[0, j] * t[0] + R[1, j] * t[1]) + R[2, j] * t[2])
    return out


def _rigid_mul(A, B):
    """A . B for A [4,4] and B [n,4,4], each element (a0 b0 + a1 b1) + a2 b2, the translation + A's (SPEC 11.6)."""
    out = np.zeros_like(B)
    out[:, 3, 3] = 1.0
    for a in range(3):
        for b in range(3):
            out[:, a, b] = (A[a, 0] * B[:, 0, b] + A[a, 1] * B[:, 1, b]) + A[a, 2] * B[:, 2, b]
        out[:, a, 3] = ((A[a, 0] * B[:, 0, 3] + A[a, 1] * B[:, 1, 3]) + A[a, 2] * B[:, 2, 3]) + A[a, 3]
    return out


class FeatureModel:
    """The keypoint features of one object (SPEC 11.6): descriptors u8 [Nm,128] and frames f64 [Nm,4,4] in the object's
    frame, on the device, and the diameter D of 6.1. The constructor has the reference's signature (:73) and ignores its
    arguments; construct / from_mesh / load fill the model."""

    def __init__(self, dataset_root=None, is_sym=False, args=None, create_index=True):
        self.dataset_root, self.is_sym = dataset_root, bool(is_sym)
        self.descriptors = self.frames = self.D = None

    # ---- building -------------------------------------------------------------------------------------------------------
    def construct(self, obj_id, obj_path, dataset_camera, mm2m=True, **kwargs):
        """The reference's call (:74): a BOP .ply with vertex colours or a texture (millimetres; mm2m scales it to metres, the unit of
        the scene depth, SPEC 7.1), dataset_camera["K"] the camera the scenes are taken with."""
        from . import render
        mesh = render.load_mesh(obj_path, scale=0.001 if mm2m else 1.0)
        self.obj_id = obj_id
        return self._build(mesh, np.asarray(dataset_camera["K"], dtype=np.float64), **kwargs)

    @classmethod
    def from_mesh(cls, mesh, cam_K, **kwargs):
        """From a vertex-coloured or texture-mapped render.Mesh (already in the scene's units) -> FeatureModel."""
        return cls()._build(mesh, np.asarray(cam_K, dtype=np.float64), **kwargs)

    def _build(self, mesh, cam_K, level=2, view_size=256, distance=0.8, contrast=CONTRAST, pad=1.1, z_near=0.05,
               rotations=None, views_per_call=16):
        from . import render
        if getattr(mesh, "colors", None) is None and not render._has_texture(mesh):
            raise ValueError("FeatureModel: the mesh has no vertex colours and no texture")
        R = render.view_grid(level=level, inplane=1) if rotations is None else np.asarray(rotations, dtype=np.float64)
        S, n = int(view_size), len(R)
        cams, _tz = render._frame_views(mesh.vertices, R, float(distance), cam_K, S, S, float(pad), float(z_near))
        cams = cams.astype(np.float32)
        poses = np.tile(np.eye(4), (n, 1, 1))
        poses[:, :3, :3], poses[:, 2, 3] = R, float(distance)
        descs, frames = [], []
        total = 0
        for a in range(0, n, views_per_call):
            b = min(n, a + views_per_call)
            color, depth = render.render_color(mesh, poses[a:b], None, (S, S), 0.5, z_near, intrinsics=cams[a:b])
            for v in range(a, b):
                K = np.array([[cams[v, 0], 0, cams[v, 2]], [0, cams[v, 1], cams[v, 3]], [0, 0, 1]], dtype=np.float64)
                dep = depth[v - a]
                f = featurize(color[v - a], dep, dep > 0, K, contrast=contrast)
                k = check_count(f)
                keep = torch.nonzero(f["ok"][:k]).flatten()
                if len(keep) == 0:
                    continue
                descs.append(f["descriptors"][keep])
                frames.append(_rigid_mul(_rigid_inverse(poses[v]), f["frames"][keep].cpu().numpy()))
                total += len(keep)
        if total > _lib.FEAT_MAX_MODEL_FEATURES:
            raise ValueError("FeatureModel: contrast=%d and level=%d give %d model features, more than the %d this build "
                             "takes; raise contrast or lower level" % (contrast, level, total, _lib.FEAT_MAX_MODEL_FEATURES))
        dev = mesh.device
        self.descriptors = (torch.cat(descs) if descs else torch.zeros(0, 128, dtype=torch.uint8, device=dev)).contiguous()
        Fm = np.concatenate(frames) if frames else np.zeros((0, 4, 4))
        self.frames = torch.from_numpy(np.ascontiguousarray(Fm)).to(dev)
        self.D = box_diameter(mesh.vertices)
        self.view_cams, self.view_poses = cams, poses          # the virtual cameras (fx, fy, cx, cy) f32 and poses T_v
        self.contrast = int(contrast)
        return self

    def save(self, path):
        np.savez(path, descriptors=self.descriptors.cpu().numpy(), frames=self.frames.cpu().numpy(), D=np.float32(self.D),
                 contrast=np.int32(self.contrast))

    @classmethod
    def load(cls, path, device=None):
        z = np.load(path)
        self = cls()
        dev = torch.device(device) if device is not None else _lib._dev()
        self.descriptors = torch.from_numpy(np.ascontiguousarray(z["descriptors"], dtype=np.uint8)).to(dev)
        self.frames = torch.from_numpy(np.ascontiguousarray(z["frames"], dtype=np.float64)).to(dev)
        self.D, self.contrast = np.float32(z["D"]), int(z["contrast"])
        return self

    def __len__(self):
        return 0 if self.descriptors is None else int(self.descriptors.shape[0])

    # ---- matching -------------------------------------------------------------------------------------------------------
    def _need(self):
        if self.descriptors is None:
            raise ValueError("FeatureModel: no features yet (construct, from_mesh or load)")

    def _hypotheses(self, desc, frames, ok, count, NumResult=100, PoseClusterDistRel=0.1):
        """SPEC 11.7-11.8 on device rows -> dict of device tensors of every stage."""
        self._need()
        if int(NumResult) <= 0:
            raise ValueError("FeatureModel: NumResult must be >= 1")
        dev, cap, Nm = desc.device, int(desc.shape[0]), len(self)
        m = match_descriptors(desc, ok, count, self.descriptors)
        peaks = torch.empty(cap, 3, dtype=torch.int32, device=dev)
        cand = torch.empty(cap, 4, 4, dtype=torch.float64, device=dev)
        st = _lib.stream()
        _call("ossid_feat_hypotheses", m.data_ptr(), frames.data_ptr(), count.data_ptr(), cap,
              self.frames.data_ptr() if Nm else None, Nm, peaks.data_ptr(), cand.data_ptr(), st)
        poses = torch.empty(int(NumResult), 4, 4, dtype=torch.float64, device=dev)
        scores = torch.empty(int(NumResult), dtype=torch.float64, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        # 6.6 unchanged: votes w, reference index = scene feature index (ref_step 1), score = sum w / 1024
        _call("ossid_ppf_cluster", peaks.data_ptr(), cand.data_ptr(), count.data_ptr(), cap, 1, 1024, float(self.D),
              float(np.float32(PoseClusterDistRel)), int(NumResult), poses.data_ptr(), scores.data_ptr(), info.data_ptr(), st)
        return {"match": m, "peaks": peaks, "cand_poses": cand, "poses": poses, "scores": scores, "info": info}

    def find_hypotheses(self, depth, img, mask, cam_K, NumResult=100, contrast=None, max_keypoints=None):
        """Device form: depth f32 [H,W], img u8 [H,W,3], mask [H,W], cam_K -> device tensors (poses f64 [NumResult,4,4],
        scores f64 [NumResult], info int32 [4] = results, keypoints found, candidates, clusters). Rows past info[0] are
        zero. Nothing is copied to the host: a frame over the keypoint cap shows as info[1] > the cap and has no result."""
        f = featurize(img, depth, mask, cam_K, contrast=self.contrast if contrast is None else contrast,
                      max_keypoints=max_keypoints)
        r = self._hypotheses(f["descriptors"], f["frames"], f["ok"], f["count"], NumResult)
        return r["poses"], r["scores"], r["info"]

    def match(self, features, frames, mat_gt=None, NumResult=100):
        """The reference's call (:435): features [n,128] and frames [n,4,4] as featurizeScene returns them -> (poses
        np.float64 [K,4,4], aux); K may be 0. mat_gt is ignored: the result does not depend on the ground truth."""
        self._need()
        Fe = np.ascontiguousarray(np.asarray(features)).astype(np.uint8).reshape(-1, 128)
        Fr = np.ascontiguousarray(np.asarray(frames, dtype=np.float64)).reshape(-1, 4, 4)
        n = len(Fe)
        if len(Fr) != n:
            raise ValueError("match: %d features but %d frames" % (n, len(Fr)))
        if n == 0:
            return np.zeros((0, 4, 4)), {"scores": np.zeros(0), "match": np.zeros((0, 3), dtype=np.int32)}
        if n > _lib.FEAT_MAX_KEYPOINTS:
            raise ValueError("match: %d scene features, more than the %d this build takes" % (n, _lib.FEAT_MAX_KEYPOINTS))
        dev = self.descriptors.device
        r = self._hypotheses(torch.from_numpy(Fe).to(dev), torch.from_numpy(Fr).to(dev),
                             torch.ones(n, dtype=torch.uint8, device=dev), torch.tensor([n, 0], dtype=torch.int32, device=dev),
                             NumResult)
        k = int(r["info"][0].item())
        return r["poses"][:k].cpu().numpy(), {"scores": r["scores"][:k].cpu().numpy(), "match": r["match"][:n].cpu().numpy()}


def featurizeScene(img, dist_im, mask, scene_meta, *_unused, contrast=CONTRAST):
    """The reference's call (:427): img u8 [H,W,3], dist_im the DISTANCE image (depth_im_to_dist_im_fast), mask, scene_meta
    with the camera -> (keypoints int [n,2] = full-resolution (x, y), features u8 [n,128], cloud f64 [n,3] = the keypoints'
    3-D points, frames f64 [n,4,4]) as host arrays, the dropped keypoints left out. The distance is turned back into Z
    by SPEC 8.3's s in f64. Raises ValueError when no feature survives (the reference's "mask too small" path) and when
    the frame is over the keypoint cap."""
    K = hostutil.meta2K(scene_meta)
    fx, fy, cx, cy = (float(v) for v in _intrinsics(K))
    dist = np.asarray(dist_im, dtype=np.float64)
    H, W = dist.shape
    a = (np.arange(W, dtype=np.float64)[None, :] - cx) / fx
    b = (np.arange(H, dtype=np.float64)[:, None] - cy) / fy
    depth = (dist / np.sqrt((a * a + b * b) + 1.0)).astype(np.float32)
    f = featurize(img, depth, np.asarray(mask) != 0, K, contrast=contrast)
    n = check_count(f)
    keep = torch.nonzero(f["ok"][:n]).flatten()
    if len(keep) == 0:
        raise ValueError("featurizeScene: no keypoint feature in the mask (%d keypoints, none with a descriptor and a frame)" % n)
    kp = f["keypoints"][keep].cpu().numpy().astype(np.int64)
    frames = f["frames"][keep].cpu().numpy()
    xy = np.stack([kp[:, 3] << kp[:, 0], kp[:, 2] << kp[:, 0]], 1)
    return xy, f["descriptors"][keep].cpu().numpy(), np.ascontiguousarray(frames[:, :3, 3]), frames
