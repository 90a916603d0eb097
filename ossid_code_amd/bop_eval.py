"""BOP-19 pose-error evaluation on the device (csrc/bop_eval.hip, SPEC.md section 8): VSD, MSSD, MSPD and the average
recall, the figure the reference's run ends with --

    saveResultsBop(..., run_eval_script=True)                                      scripts/online_learning.py:603-608
    os.system("cd BOP_TOOLKIT_PATH; python scripts/eval_bop19.py --renderer_type=cpp --result_filenames=...")
                                                                                   utils/bop_utils.py:51-53

bop_toolkit is not part of the reference tree: the definitions are this build's own restatement of the published ones
(Hodan et al., "BOP Challenge 2020 on 6D Object Localization", section 2.2); parity with bop_toolkit is unpinned.

vsd renders every estimate and its ground truth with render.render_depth (pixel_offset = 0) and counts on the device;
mssd_mspd is one launch per 256 estimates; average_recall and symmetry_transformations are host code; evaluate ties them
together over a dataset object, BopFolder is that object over the standard BOP folder layout, and tools/eval_bop19.py the
command line. Everything works in ONE length unit, the caller's: metres with the device pipeline (delta = 0.015,
z_near = 0.05), millimetres with BOP folders and the BOP csv (delta = 15, z_near = 50).
"""
import csv
import json
import os

import numpy as np
import torch

from . import _lib
from . import render as _render

VSD_TAUS = tuple(k * 0.05 for k in range(1, 11))          # 8.1: tau_k = k * 0.05
THETAS = tuple(k * 0.05 for k in range(1, 11))            # 8.8: correctness thresholds of VSD and (x diameter) MSSD
THETAS_PX = tuple(5.0 * k for k in range(1, 11))          # 8.8: MSPD thresholds in pixels at a 640-wide image


# ---- 8.6 symmetry transformations ------------------------------------------------------------------------------------------
def symmetry_transformations(model_info, max_sym_disc_step=0.01):
    """models_info.json entry -> f64 [S,4,4] (SPEC 8.6): the identity and the `symmetries_discrete`, each preceded on the
    left by every step of the `symmetries_continuous` (ceil(pi / max_sym_disc_step) rotations about the axis through
    `offset`). More than 4096 transformations raise ValueError."""
    if not (float(max_sym_disc_step) > 0.0):
        raise ValueError("max_sym_disc_step must be > 0, got %r" % (max_sym_disc_step,))
    disc = [np.eye(4)]
    for m in model_info.get("symmetries_discrete", ()):
        M = np.asarray(m, dtype=np.float64)
        if M.size != 16:
            raise ValueError("a discrete symmetry is 16 numbers (4x4 row-major), got %d" % M.size)
        disc.append(M.reshape(4, 4))
    cont = []
    for sym in model_info.get("symmetries_continuous", ()):
        axis, off = np.asarray(sym["axis"], dtype=np.float64), np.asarray(sym["offset"], dtype=np.float64)
        norm = np.sqrt(axis @ axis)
        if axis.shape != (3,) or off.shape != (3,) or not norm > 0.0:
            raise ValueError("a continuous symmetry needs a non-zero axis [3] and an offset [3]")
        a = axis / norm
        n = int(np.ceil(np.pi / float(max_sym_disc_step)))
        Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
        K2 = Kx @ Kx
        for i in range(n):
            th = i * (2.0 * np.pi / n)
            R = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * K2          # Rodrigues
            cont.append((R, -(R @ off) + off))
    n_out = len(disc) * max(len(cont), 1)
    if n_out > _lib.BOP_MAX_SYMMETRIES:
        raise ValueError("%d symmetry transformations (at most %d): raise max_sym_disc_step" % (n_out, _lib.BOP_MAX_SYMMETRIES))
    out = np.tile(np.eye(4), (n_out, 1, 1))
    k = 0
    for D in disc:
        if not cont:
            out[k] = D
            k += 1
        for Rc, tc in cont:
            out[k, :3, :3], out[k, :3, 3] = Rc @ D[:3, :3], Rc @ D[:3, 3] + tc
            k += 1
    return out


# ---- argument plumbing -------------------------------------------------------------------------------------------------------
def _poses(pose_est, pose_gt):
    pe, pg = np.asarray(pose_est, dtype=np.float64), np.asarray(pose_gt, dtype=np.float64)
    pe, pg = (p[None] if p.ndim == 2 else p for p in (pe, pg))
    if pe.ndim != 3 or pe.shape[1:] != (4, 4) or pg.shape != pe.shape or len(pe) < 1:
        raise ValueError("pose_est and pose_gt must both be [N,4,4] with N >= 1, got %s and %s" % (pe.shape, pg.shape))
    return np.ascontiguousarray(pe), np.ascontiguousarray(pg)


def _cameras(cam_K, n_frames=None):
    """cam_K [3,3] or [Fr,3,3] -> f32 [Fr,4] = fx, fy, cx, cy."""
    K = np.asarray(cam_K, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.repeat(K[None], n_frames or 1, 0)
    if K.ndim != 3 or K.shape[1:] != (3, 3) or (n_frames is not None and len(K) != n_frames):
        raise ValueError("cam_K must be [3,3] or one [3,3] per frame, got %s" % (K.shape,))
    return np.ascontiguousarray(np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1).astype(np.float32))


def _frames(frame, N, Fr):
    f = np.zeros(N, dtype=np.int32) if frame is None else np.asarray(frame)
    if f.shape != (N,) or not np.issubdtype(f.dtype, np.integer):
        raise ValueError("frame must be N = %d integers, got %s %s" % (N, f.dtype, f.shape))
    if len(f) and (f.min() < 0 or f.max() >= Fr):
        raise ValueError("frame index outside [0, %d)" % Fr)
    return np.ascontiguousarray(f, dtype=np.int32)


# ---- 8.2-8.5 VSD ---------------------------------------------------------------------------------------------------------------
def vsd(mesh, diameter, depth_obs, cam_K, pose_est, pose_gt, frame=None, delta=0.015, taus=None, z_near=0.05,
        return_counts=False, chunk=64):
    """Visible surface discrepancy of N estimates (SPEC 8.2-8.5) -> errors f64 numpy [N,T]; with return_counts also counts
    int32 [N,T+2] = (n_U, n_I, c_0 .. c_{T-1}). mesh: a render.Mesh; depth_obs [H,W] or [Fr,H,W] (numpy or tensor; not > 0 =
    invalid); cam_K [3,3] or [Fr,3,3]; frame [N] picks each estimate's image (default 0). Estimates are grouped by camera and
    rendered `chunk` at a time (two f32 [chunk,H,W] images live at once); the result does not depend on `chunk`."""
    pe, pg = _poses(pose_est, pose_gt)
    N = len(pe)
    dev = mesh.device
    O = depth_obs if torch.is_tensor(depth_obs) else torch.from_numpy(np.asarray(depth_obs, dtype=np.float32))
    O = O[None] if O.dim() == 2 else O
    if O.dim() != 3:
        raise ValueError("depth_obs must be [H,W] or [Fr,H,W], got %s" % (tuple(O.shape),))
    Fr, H, W = (int(v) for v in O.shape)
    O = O.to(dev, torch.float32).contiguous()
    cams = _cameras(cam_K, Fr)
    fidx = _frames(frame, N, Fr)
    tau = np.ascontiguousarray(VSD_TAUS if taus is None else taus, dtype=np.float64).reshape(-1)
    T = len(tau)
    if not 1 <= T <= _lib.BOP_MAX_TAUS or not np.isfinite(tau).all():
        raise ValueError("taus must be 1 to %d finite values, got %r" % (_lib.BOP_MAX_TAUS, taus))
    if not (float(diameter) > 0.0 and np.isfinite(diameter)):
        raise ValueError("diameter must be finite and > 0, got %r" % (diameter,))
    if not (float(delta) >= 0.0 and np.isfinite(delta)):
        raise ValueError("delta must be finite and >= 0, got %r" % (delta,))
    chunk = int(chunk)
    if not 1 <= chunk <= _lib.RASTER_MAX_POSES:
        raise ValueError("chunk must lie in [1, %d], got %r" % (_lib.RASTER_MAX_POSES, chunk))
    cams_dev = torch.from_numpy(cams).to(dev)
    counts = torch.empty(N, T + 2, dtype=torch.int32, device=dev)
    errors = torch.empty(N, T, dtype=torch.float64, device=dev)
    groups = {}
    for i in range(N):                                           # the rasteriser takes one camera per call
        groups.setdefault(cams[fidx[i]].tobytes(), []).append(i)
    fn = _lib.fn("ossid_bop_vsd")
    for rows in groups.values():
        fx, fy, cx, cy = (float(v) for v in cams[fidx[rows[0]]])
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        for a in range(0, len(rows), chunk):
            sel = np.asarray(rows[a:a + chunk])
            z_est = _render.render_depth(mesh, pe[sel], K, (H, W), pixel_offset=0.0, z_near=z_near)
            z_gt = _render.render_depth(mesh, pg[sel], K, (H, W), pixel_offset=0.0, z_near=z_near)
            c = torch.empty(len(sel), T + 2, dtype=torch.int32, device=dev)
            e = torch.empty(len(sel), T, dtype=torch.float64, device=dev)
            fsel = np.ascontiguousarray(fidx[sel])
            with _lib.on_device(dev):
                rc = fn(O.data_ptr(), cams_dev.data_ptr(), Fr, H, W, z_est.data_ptr(), z_gt.data_ptr(), fsel.ctypes.data, len(sel),
                        float(diameter), float(delta), tau.ctypes.data, T, c.data_ptr(), e.data_ptr(), _lib.stream())
            _lib.check(rc, "ossid_bop_vsd")
            idx = torch.from_numpy(sel).to(dev)
            counts[idx], errors[idx] = c, e
    errors = errors.cpu().numpy()
    return (errors, counts.cpu().numpy()) if return_counts else errors


# ---- 8.7 MSSD / MSPD -------------------------------------------------------------------------------------------------------------
def mssd_mspd(vertices, symmetries, pose_est, pose_gt, cam_K, frame=None):
    """Maximum symmetry-aware surface and projection distances (SPEC 8.7) -> (mssd f64 numpy [N] in the vertices' unit,
    mspd f64 numpy [N] in pixels; +inf where a vertex is at Z <= 0 under either pose for every symmetry). vertices: a
    render.Mesh (its scaled f32 vertices), or [V,3] (cast to f32); symmetries f64 [S,4,4] (symmetry_transformations);
    cam_K [3,3] or [Fr,3,3] with frame [N]."""
    pe, pg = _poses(pose_est, pose_gt)
    N = len(pe)
    S = np.ascontiguousarray(symmetries, dtype=np.float64)
    if S.ndim != 3 or S.shape[1:] != (4, 4) or not 1 <= len(S) <= _lib.BOP_MAX_SYMMETRIES:
        raise ValueError("symmetries must be [S,4,4] with 1 <= S <= %d, got %s" % (_lib.BOP_MAX_SYMMETRIES, S.shape))
    K = np.asarray(cam_K, dtype=np.float64)
    cams = _cameras(K, None if K.ndim == 3 else 1)
    fidx = _frames(frame, N, len(cams))
    if isinstance(vertices, _render.Mesh):
        P, dev = vertices.vertices, vertices.device
    else:
        P = vertices if torch.is_tensor(vertices) else torch.from_numpy(np.asarray(vertices, dtype=np.float64).astype(np.float32))
        if P.dim() != 2 or P.shape[1] != 3 or not 1 <= P.shape[0] <= _lib.RASTER_MAX_VERTICES:
            raise ValueError("vertices must be [V,3] with 1 <= V <= %d, got %s" % (_lib.RASTER_MAX_VERTICES, tuple(P.shape)))
        dev = P.device if P.is_cuda else torch.device("cuda", torch.cuda.current_device())
        P = P.to(dev, torch.float32).contiguous()
    Sd, ped, pgd, cd = (torch.from_numpy(a).to(dev) for a in (S, pe, pg, cams))
    mssd = torch.empty(N, dtype=torch.float64, device=dev)
    mspd = torch.empty(N, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_bop_mssd_mspd")(P.data_ptr(), int(P.shape[0]), Sd.data_ptr(), len(S), ped.data_ptr(), pgd.data_ptr(),
                                            cd.data_ptr(), len(cams), fidx.ctypes.data, N, mssd.data_ptr(), mspd.data_ptr(),
                                            _lib.stream())
    _lib.check(rc, "ossid_bop_mssd_mspd")
    return mssd.cpu().numpy(), mspd.cpu().numpy()


# ---- 8.8 recall ------------------------------------------------------------------------------------------------------------------
def _target_key(t):
    if isinstance(t, dict):
        if int(t.get("inst_count", 1)) != 1:
            raise ValueError("target %r has %d ground-truth instances: multi-instance matching is not supported"
                             % (t, int(t["inst_count"])))
        return int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"])
    s, i, o = t
    return int(s), int(i), int(o)


def _target_keys(targets):
    keys = [_target_key(t) for t in targets]
    if len(set(keys)) != len(keys):
        raise ValueError("a (scene_id, im_id, obj_id) target is listed more than once: multi-instance matching is not supported")
    if not keys:
        raise ValueError("no targets")
    return keys


def _best_rows(rows, keys):
    """The estimate of each target: its highest-scored row (the first among equal scores)."""
    want, best = set(keys), {}
    for r in rows:
        k = (int(r["scene_id"]), int(r["im_id"]), int(r["obj_id"]))
        if k in want and (k not in best or float(r["score"]) > float(best[k]["score"])):
            best[k] = r
    return best


def average_recall(errors, targets, diameters, image_width):
    """SPEC 8.8. errors: rows (dicts) with scene_id, im_id, obj_id, score, vsd [T], mssd, mspd; targets: (scene_id, im_id,
    obj_id) triples or BOP target dicts (inst_count must be 1); diameters: {obj_id: diameter} in the unit of mssd;
    image_width in pixels -> {"AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "recall_vsd" [T][10], "recall_mssd" [10],
    "recall_mspd" [10], "targets", "estimates"}. A target without a row is a miss; a row is correct iff error < threshold."""
    keys = _target_keys(targets)
    best = _best_rows(errors, keys)
    n = float(len(keys))
    T = len(next(iter(best.values()))["vsd"]) if best else 0
    if any(len(r["vsd"]) != T for r in best.values()):
        raise ValueError("rows carry different numbers of VSD taus")
    hit = [best[k] for k in keys if k in best]
    rec_vsd = [[sum(1 for r in hit if r["vsd"][t] < th) / n for th in THETAS] for t in range(T)]
    rec_mssd = [sum(1 for r in hit if r["mssd"] < th * float(diameters[int(r["obj_id"])])) / n for th in THETAS]
    ratio = float(image_width) / 640.0
    rec_mspd = [sum(1 for r in hit if r["mspd"] < px * ratio) / n for px in THETAS_PX]
    ar_vsd = float(np.mean(rec_vsd)) if T else 0.0
    ar_mssd, ar_mspd = float(np.mean(rec_mssd)), float(np.mean(rec_mspd))
    return {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0,
            "recall_vsd": rec_vsd, "recall_mssd": rec_mssd, "recall_mspd": rec_mspd, "targets": len(keys), "estimates": len(hit)}


def evaluate(results, dataset):
    """results: rows (dicts) with scene_id, im_id, obj_id, score and pose (4x4 in the dataset's unit), e.g.
    read_results_csv's. dataset: an object with mesh(obj_id) -> render.Mesh or (vertices, faces), model_info(obj_id) -> dict
    with "diameter" and optional symmetries, frame(scene_id, im_id) -> (depth [H,W], cam_K), gt_pose(scene_id, im_id, obj_id)
    -> [4,4], `targets`, and optionally `delta` / `z_near` (defaults 0.015 / 0.05: metres). Rows are grouped by object, the
    highest-scored row of every target is evaluated -> average_recall's dict plus "rows": the evaluated rows with their
    vsd / mssd / mspd."""
    keys = _target_keys(dataset.targets)
    best = _best_rows(results, keys)
    delta, z_near = float(getattr(dataset, "delta", 0.015)), float(getattr(dataset, "z_near", 0.05))
    by_obj = {}
    for k in keys:
        if k in best:
            by_obj.setdefault(k[2], []).append(k)
    rows, diameters, width = [], {}, None
    for k in keys:
        diameters.setdefault(k[2], float(dataset.model_info(k[2])["diameter"]))
    for obj_id, ks in by_obj.items():
        mesh = dataset.mesh(obj_id)
        if not isinstance(mesh, _render.Mesh):
            mesh = _render.Mesh(*mesh)
        info = dataset.model_info(obj_id)
        syms = symmetry_transformations(info)
        images = sorted(set((k[0], k[1]) for k in ks))
        frames = [dataset.frame(*im) for im in images]
        shapes = set(np.asarray(d).shape for d, _K in frames)
        if len(shapes) != 1:
            raise ValueError("object %d: its images have different sizes %s" % (obj_id, sorted(shapes)))
        width = frames[0][0].shape[1] if width is None else width
        if frames[0][0].shape[1] != width:
            raise ValueError("images of different widths in one evaluation")
        depth = np.stack([np.asarray(d, dtype=np.float32) for d, _K in frames])
        cam_K = np.stack([np.asarray(K, dtype=np.float64).reshape(3, 3) for _d, K in frames])
        fidx = np.asarray([images.index((k[0], k[1])) for k in ks], dtype=np.int32)
        pe = np.stack([np.asarray(best[k]["pose"], dtype=np.float64).reshape(4, 4) for k in ks])
        pg = np.stack([np.asarray(dataset.gt_pose(*k), dtype=np.float64).reshape(4, 4) for k in ks])
        e_vsd = vsd(mesh, diameters[obj_id], depth, cam_K, pe, pg, fidx, delta=delta, z_near=z_near)
        e_mssd, e_mspd = mssd_mspd(mesh, syms, pe, pg, cam_K, fidx)
        for i, k in enumerate(ks):
            rows.append({"scene_id": k[0], "im_id": k[1], "obj_id": k[2], "score": float(best[k]["score"]),
                         "vsd": [float(v) for v in e_vsd[i]], "mssd": float(e_mssd[i]), "mspd": float(e_mspd[i])})
    if width is None:
        width = np.asarray(dataset.frame(keys[0][0], keys[0][1])[0]).shape[1]
    out = average_recall(rows, keys, diameters, width)
    out["rows"] = rows
    return out


# ---- BOP files -------------------------------------------------------------------------------------------------------------------
def read_results_csv(path):
    """The csv pipeline.save_results_bop writes (scene_id,im_id,obj_id,score,R,t,time; t in millimetres) -> rows with a
    4x4 `pose` in millimetres."""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            pose = np.eye(4)
            pose[:3, :3] = np.array(r["R"].split(), dtype=np.float64).reshape(3, 3)
            pose[:3, 3] = np.array(r["t"].split(), dtype=np.float64)
            rows.append({"scene_id": int(r["scene_id"]), "im_id": int(r["im_id"]), "obj_id": int(r["obj_id"]),
                         "score": float(r["score"]), "pose": pose, "time": float(r["time"])})
    return rows


class BopFolder:
    """evaluate's dataset over the standard BOP layout, in millimetres (delta = 15, z_near = 50):
    <root>/<dataset_name>/models_eval/models_info.json and obj_%06d.ply, test_targets_bop19.json, and per scene
    <split>/%06d/scene_gt.json, scene_camera.json (cam_K, depth_scale), depth/%06d.png."""

    delta, z_near = 15.0, 50.0

    def __init__(self, root, dataset_name, split="test", targets_filename="test_targets_bop19.json"):
        self.base = os.path.join(root, dataset_name)
        self.split = os.path.join(self.base, split)
        with open(os.path.join(self.base, "models_eval", "models_info.json")) as f:
            self._info = {int(k): v for k, v in json.load(f).items()}
        with open(os.path.join(self.base, targets_filename)) as f:
            self.targets = json.load(f)
        self._gt, self._cam = {}, {}

    def _scene(self, cache, scene_id, name):
        if scene_id not in cache:
            with open(os.path.join(self.split, "%06d" % scene_id, name)) as f:
                cache[scene_id] = {int(k): v for k, v in json.load(f).items()}
        return cache[scene_id]

    def model_info(self, obj_id):
        return self._info[int(obj_id)]

    def mesh(self, obj_id):
        """(vertices f64 [V,3] in millimetres, faces int32 [F,3]): evaluate uploads them once per object."""
        return _render.read_ply_mesh(os.path.join(self.base, "models_eval", "obj_%06d.ply" % obj_id))

    def frame(self, scene_id, im_id):
        from PIL import Image
        cam = self._scene(self._cam, scene_id, "scene_camera.json")[int(im_id)]
        png = np.asarray(Image.open(os.path.join(self.split, "%06d" % scene_id, "depth", "%06d.png" % im_id)))
        depth = (png.astype(np.float64) * float(cam.get("depth_scale", 1.0))).astype(np.float32)
        return depth, np.asarray(cam["cam_K"], dtype=np.float64).reshape(3, 3)

    def gt_pose(self, scene_id, im_id, obj_id):
        found = [g for g in self._scene(self._gt, scene_id, "scene_gt.json")[int(im_id)] if int(g["obj_id"]) == int(obj_id)]
        if len(found) != 1:
            raise ValueError("scene %d image %d has %d instances of object %d: exactly one is supported"
                             % (scene_id, im_id, len(found), obj_id))
        T = np.eye(4)
        T[:3, :3] = np.asarray(found[0]["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
        T[:3, 3] = np.asarray(found[0]["cam_t_m2c"], dtype=np.float64).reshape(3)
        return T
