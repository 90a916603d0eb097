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
command line. Targets with several ground-truth instances (SPEC 8.10-8.12) are opt-in, evaluate(..., multi_instance=True):
vsd_pairs renders every kept estimate and every instance of a target once and counts every pair through a table,
match_instances is BOP's greedy matching per threshold on the device, instance_recall the recall of the matches. What is
still not BOP-19: no per-object averaging variants, no time limits. Everything works in ONE length unit, the caller's:
metres with the device pipeline (delta = 0.015, z_near = 0.05), millimetres with BOP folders and the BOP csv (delta = 15,
z_near = 50).
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


# ---- 8.11 VSD of pairs ---------------------------------------------------------------------------------------------------------
def _pose_stack(p, name):
    p = np.asarray(p, dtype=np.float64)
    p = p[None] if p.ndim == 2 else p
    if p.ndim != 3 or p.shape[1:] != (4, 4) or len(p) < 1:
        raise ValueError("%s must be [N,4,4] with N >= 1, got %s" % (name, p.shape))
    return np.ascontiguousarray(p)


def _pair_table(pairs, Ne, Ng, Fr):
    t = np.asarray(pairs)
    if t.ndim != 2 or t.shape[1] != 3 or len(t) < 1 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("pairs must be [P,3] integers (est_row, gt_row, frame) with P >= 1, got %s %s" % (t.dtype, t.shape))
    for col, (what, n) in enumerate((("est_row", Ne), ("gt_row", Ng), ("frame", Fr))):
        if t[:, col].min() < 0 or t[:, col].max() >= n:
            raise ValueError("pairs: %s outside [0, %d)" % (what, n))
    return np.ascontiguousarray(t, dtype=np.int32)


def vsd_pairs(mesh, diameter, depth_obs, cam_K, pose_est, pose_gt, pairs, delta=0.015, taus=None, z_near=0.05,
              return_counts=False, chunk=64):
    """Visible surface discrepancy of P (estimate, instance) pairs (SPEC 8.11) -> errors f64 numpy [P,T]; with return_counts
    also counts int32 [P,T+2]. pose_est [Ne,4,4] and pose_gt [Ng,4,4] are two separate lists; pairs int [P,3] = (row of
    pose_est, row of pose_gt, frame). Row p equals vsd's row for (pose_est[pairs[p,0]], pose_gt[pairs[p,1]]) in frame
    pairs[p,2], but every pose a run of pairs names is rendered once, not once per pair. Pairs are grouped by camera and
    taken in order, as many as name at most `chunk` distinct estimates and `chunk` distinct instances at a time (two f32
    [chunk,H,W] stacks live at once); the result does not depend on `chunk`."""
    pe, pg = _pose_stack(pose_est, "pose_est"), _pose_stack(pose_gt, "pose_gt")
    dev = mesh.device
    O = depth_obs if torch.is_tensor(depth_obs) else torch.from_numpy(np.asarray(depth_obs, dtype=np.float32))
    O = O[None] if O.dim() == 2 else O
    if O.dim() != 3:
        raise ValueError("depth_obs must be [H,W] or [Fr,H,W], got %s" % (tuple(O.shape),))
    Fr, H, W = (int(v) for v in O.shape)
    cams = _cameras(cam_K, Fr)
    table = _pair_table(pairs, len(pe), len(pg), Fr)
    P = len(table)
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
    O = O.to(dev, torch.float32).contiguous()
    cams_dev = torch.from_numpy(cams).to(dev)
    counts = torch.empty(P, T + 2, dtype=torch.int32, device=dev)
    errors = torch.empty(P, T, dtype=torch.float64, device=dev)
    by_cam = {}
    for p in range(P):                                           # the rasteriser takes one camera per call
        by_cam.setdefault(cams[table[p, 2]].tobytes(), []).append(p)
    fn = _lib.fn("ossid_bop_vsd_pairs")
    for rows in by_cam.values():
        fx, fy, cx, cy = (float(v) for v in cams[table[rows[0], 2]])
        K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        a = 0
        while a < len(rows):
            est, gt, b = {}, {}, a                               # pose row -> row of this run's stack
            while b < len(rows):
                e, g = int(table[rows[b], 0]), int(table[rows[b], 1])
                if len(est) + (e not in est) > chunk or len(gt) + (g not in gt) > chunk:
                    break
                est.setdefault(e, len(est)), gt.setdefault(g, len(gt))
                b += 1
            sel = np.asarray(rows[a:b])
            local = np.ascontiguousarray(np.stack([[est[int(e)] for e in table[sel, 0]], [gt[int(g)] for g in table[sel, 1]],
                                                   table[sel, 2]], 1), dtype=np.int32)
            z_est = _render.render_depth(mesh, pe[list(est)], K, (H, W), pixel_offset=0.0, z_near=z_near)
            z_gt = _render.render_depth(mesh, pg[list(gt)], K, (H, W), pixel_offset=0.0, z_near=z_near)
            tab = torch.from_numpy(local).to(dev)
            c = torch.empty(len(sel), T + 2, dtype=torch.int32, device=dev)
            er = torch.empty(len(sel), T, dtype=torch.float64, device=dev)
            with _lib.on_device(dev):
                rc = fn(O.data_ptr(), cams_dev.data_ptr(), Fr, H, W, z_est.data_ptr(), len(est), z_gt.data_ptr(), len(gt),
                        tab.data_ptr(), len(sel), float(diameter), float(delta), tau.ctypes.data, T, c.data_ptr(), er.data_ptr(),
                        _lib.stream())
            _lib.check(rc, "ossid_bop_vsd_pairs")
            idx = torch.from_numpy(sel).to(dev)
            counts[idx], errors[idx] = c, er
            a = b
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


# ---- 8.10-8.12 several instances per target ----------------------------------------------------------------------------------------
MAX_INSTANCES = _lib.BOP_MAX_INSTANCES


def _groups(targets):
    """Targets -> [((scene_id, im_id, obj_id), inst_count)] (SPEC 8.10); a triple counts one instance."""
    out = []
    for t in targets:
        if isinstance(t, dict):
            key, n = (int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"])), int(t.get("inst_count", 1))
        else:
            key, n = tuple(int(v) for v in t), 1
        if not 1 <= n <= MAX_INSTANCES:
            raise ValueError("target %r: inst_count %d outside [1, %d]" % (key, n, MAX_INSTANCES))
        out.append((key, n))
    if len(set(k for k, _n in out)) != len(out):
        raise ValueError("a (scene_id, im_id, obj_id) target is listed more than once")
    if not out:
        raise ValueError("no targets")
    return out


def _kept_rows(rows, groups):
    """The estimates of each group (8.10): its rows by score descending, ties by input order, the first inst_count."""
    n_top = dict(groups)
    found = {}
    for r in rows:
        k = (int(r["scene_id"]), int(r["im_id"]), int(r["obj_id"]))
        if k in n_top:
            found.setdefault(k, []).append(r)
    return {k: sorted(v, key=lambda r: -float(r["score"]))[:n_top[k]] for k, v in found.items()}       # sorted is stable


def match_instances(err, E, G, valid, thr, device=None):
    """SPEC 8.12 on the device (ossid_bop_match). err f64 [Ptot,T+2]: per pair the T VSD errors, MSSD, MSPD, the pairs of
    group i stored [e][g] row-major, groups one after the other; E, G int [Gr] (0 <= E <= 64 estimates in rank order,
    1 <= G <= 64 instances); valid bool [sum G]; thr f64 [Gr,T+2,10] -> (match int32 numpy [sum E,T+2,10]: the instance each
    estimate is matched to, -1 for none; tp int32 numpy [T+2,10]: the matches whose instance is valid)."""
    E, G = np.asarray(E, dtype=np.int64).reshape(-1), np.asarray(G, dtype=np.int64).reshape(-1)
    Gr = len(E)
    if Gr < 1 or len(G) != Gr or E.min() < 0 or E.max() > MAX_INSTANCES or G.min() < 1 or G.max() > MAX_INSTANCES:
        raise ValueError("E and G must be [Gr >= 1] with 0 <= E <= %d and 1 <= G <= %d" % (MAX_INSTANCES, MAX_INSTANCES))
    thr = np.ascontiguousarray(thr, dtype=np.float64)
    if thr.ndim != 3 or thr.shape[0] != Gr or thr.shape[2] != 10 or not 1 <= thr.shape[1] - 2 <= _lib.BOP_MAX_TAUS:
        raise ValueError("thr must be [Gr = %d, T+2, 10] with 1 <= T <= %d, got %s" % (Gr, _lib.BOP_MAX_TAUS, thr.shape))
    K = thr.shape[1]
    Ptot, Etot, Itot = int((E * G).sum()), int(E.sum()), int(G.sum())
    if Ptot >= 2 ** 31 // K:
        raise ValueError("%d pairs are more than one call takes" % Ptot)
    err = np.ascontiguousarray(err, dtype=np.float64).reshape(-1, K) if Ptot else np.zeros((0, K))
    valid = np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, dtype=np.uint8)
    if len(err) != Ptot or len(valid) != Itot:
        raise ValueError("err must hold sum(E G) = %d rows and valid sum(G) = %d entries, got %d and %d"
                         % (Ptot, Itot, len(err), len(valid)))
    first = lambda n: np.concatenate([[0], np.cumsum(n)[:-1]])  # noqa: E731
    table = np.ascontiguousarray(np.stack([first(E * G), first(E), first(G), E, G], 1), dtype=np.int32)
    dev = _lib._dev() if device is None else torch.device(device)
    err_d, tab_d, val_d, thr_d = (torch.from_numpy(a).to(dev) for a in (err, table, valid, thr))
    match = torch.empty(Etot, K, 10, dtype=torch.int32, device=dev)
    tp = torch.empty(K, 10, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_bop_match")(err_d.data_ptr() if Ptot else None, Ptot, tab_d.data_ptr(), Gr, val_d.data_ptr(), Itot,
                                        thr_d.data_ptr(), K - 2, match.data_ptr() if Etot else None, Etot, tp.data_ptr(),
                                        _lib.stream())
    _lib.check(rc, "ossid_bop_match")
    return match.cpu().numpy(), tp.cpu().numpy()


def instance_recall(errors, targets, diameters, image_width, valid=None, matcher=None):
    """average_recall's counterpart for targets with several instances (SPEC 8.10-8.12). errors: rows (dicts) with
    scene_id, im_id, obj_id, score and the errors against each of the G instances of their target: vsd [G][T], mssd [G],
    mspd [G] ([T] and scalars where G = 1); targets: BOP target dicts (inst_count = n: the n best-scored rows are kept) or
    triples (n = 1); valid: {(scene_id, im_id, obj_id): [G] flags}, instances that count (default: all) -> average_recall's
    keys, the recall of a column being its valid matches / sum of inst_count, and "match" int32 [Etot][T+2][10]: per kept
    estimate (groups in target order, estimates by rank), error kind (the T taus, MSSD, MSPD) and threshold column the
    matched instance or -1. The matching is BOP's greedy rule, not an optimal assignment, and runs on the device
    (match_instances); `matcher` takes its place in a test that holds it against the restatement's loop."""
    groups = _groups(targets)
    kept = _kept_rows(errors, groups)
    T = None
    E, G, err, val = [], [], [], []
    for key, _n in groups:
        rows = kept.get(key, [])
        g = None
        for r in rows:
            v = np.atleast_2d(np.asarray(r["vsd"], dtype=np.float64))
            m3, m2 = (np.atleast_1d(np.asarray(r[k], dtype=np.float64)) for k in ("mssd", "mspd"))
            T = v.shape[1] if T is None else T
            g = len(v) if g is None else g
            if v.ndim != 2 or v.shape != (g, T) or m3.shape != (g,) or m2.shape != (g,):
                raise ValueError("target %r: rows carry different numbers of instances or VSD taus" % (key,))
            err.append(np.concatenate([v, m3[:, None], m2[:, None]], 1))
        flags = None if valid is None or key not in valid else np.asarray(valid[key]).reshape(-1) != 0
        g = (1 if flags is None else len(flags)) if g is None else g
        if not 1 <= g <= MAX_INSTANCES:
            raise ValueError("target %r: %d ground-truth instances (1 to %d are supported)" % (key, g, MAX_INSTANCES))
        if flags is not None and len(flags) != g:
            raise ValueError("target %r: %d valid flags for %d instances" % (key, len(flags), g))
        E.append(len(rows)), G.append(g), val.append(np.ones(g, bool) if flags is None else flags)
    n = float(sum(c for _k, c in groups))
    Etot = sum(E)
    if T is None:                                                # no target has an estimate: every column is empty
        match, rec = np.zeros((0, 2, 10), np.int32), np.zeros((2, 10))
        T = 0
    else:
        ratio = float(image_width) / 640.0
        thr = np.empty((len(groups), T + 2, 10))
        for i, (key, _n) in enumerate(groups):
            thr[i, :T] = THETAS
            thr[i, T] = [th * float(diameters[key[2]]) for th in THETAS]
            thr[i, T + 1] = [px * ratio for px in THETAS_PX]
        match, tp = (matcher or match_instances)(np.concatenate(err) if err else np.zeros((0, T + 2)), E, G, np.concatenate(val), thr)
        rec = np.asarray(tp, dtype=np.int64) / n
    rec_vsd, rec_mssd, rec_mspd = [[float(v) for v in rec[t]] for t in range(T)], [float(v) for v in rec[T]], [float(v) for v in rec[T + 1]]
    ar_vsd = float(np.mean(rec_vsd)) if T else 0.0
    ar_mssd, ar_mspd = float(np.mean(rec_mssd)), float(np.mean(rec_mspd))
    return {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0,
            "recall_vsd": rec_vsd, "recall_mssd": rec_mssd, "recall_mspd": rec_mspd, "targets": len(groups), "estimates": Etot,
            "match": np.asarray(match, dtype=np.int32)}


def _evaluate_instances(results, dataset, visib_gt_min):
    """evaluate(..., multi_instance=True): per object one vsd_pairs and one mssd_mspd call over every (kept estimate,
    instance) pair of its targets, then instance_recall."""
    groups = _groups(dataset.targets)
    kept = _kept_rows(results, groups)
    delta, z_near = float(getattr(dataset, "delta", 0.015)), float(getattr(dataset, "z_near", 0.05))
    gts, valid, diameters, by_obj, width = {}, {}, {}, {}, None
    for key, _n in groups:
        diameters.setdefault(key[2], float(dataset.model_info(key[2])["diameter"]))
        g = np.asarray(dataset.gt_poses(*key), dtype=np.float64).reshape(-1, 4, 4)
        if not 1 <= len(g) <= MAX_INSTANCES:
            raise ValueError("target %r: %d ground-truth instances (1 to %d are supported)" % (key, len(g), MAX_INSTANCES))
        gts[key] = g
        visib = dataset.gt_visib(*key) if hasattr(dataset, "gt_visib") else None
        if visib is not None:
            visib = np.asarray(visib, dtype=np.float64).reshape(-1)
            if len(visib) != len(g):
                raise ValueError("target %r: %d visibilities for %d instances" % (key, len(visib), len(g)))
            valid[key] = visib >= float(visib_gt_min)
        if key in kept:
            by_obj.setdefault(key[2], []).append(key)
    done = {}
    for obj_id, ks in by_obj.items():
        mesh = dataset.mesh(obj_id)
        if not isinstance(mesh, _render.Mesh):
            mesh = _render.Mesh(*mesh)
        syms = symmetry_transformations(dataset.model_info(obj_id))
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
        pe, pg, pairs = [], [], []
        for k in ks:
            f, e0, g0 = images.index((k[0], k[1])), len(pe), len(pg)
            pe += [np.asarray(r["pose"], dtype=np.float64).reshape(4, 4) for r in kept[k]]
            pg += list(gts[k])
            pairs += [(e0 + e, g0 + g, f) for e in range(len(kept[k])) for g in range(len(gts[k]))]
        pe, pg, pairs = np.stack(pe), np.stack(pg), np.asarray(pairs, dtype=np.int32)
        e_vsd = vsd_pairs(mesh, diameters[obj_id], depth, cam_K, pe, pg, pairs, delta=delta, z_near=z_near)
        e_mssd, e_mspd = mssd_mspd(mesh, syms, pe[pairs[:, 0]], pg[pairs[:, 1]], cam_K, pairs[:, 2])      # 16 doubles per pair
        p = 0
        for k in ks:
            G = len(gts[k])
            for r in kept[k]:
                done[id(r)] = {"scene_id": k[0], "im_id": k[1], "obj_id": k[2], "score": float(r["score"]),
                               "vsd": [[float(v) for v in row] for row in e_vsd[p:p + G]],
                               "mssd": [float(v) for v in e_mssd[p:p + G]], "mspd": [float(v) for v in e_mspd[p:p + G]]}
                p += G
    rows = [done[id(r)] for key, _n in groups for r in kept.get(key, [])]          # the order of "match"
    if width is None:
        width = np.asarray(dataset.frame(*groups[0][0][:2])[0]).shape[1]
    for key, _n in groups:                                       # a target without an estimate still states its instances
        valid.setdefault(key, np.ones(len(gts[key]), bool))
    out = instance_recall(rows, dataset.targets, diameters, width, valid=valid)
    out["rows"] = rows
    return out


def evaluate(results, dataset, multi_instance=False, visib_gt_min=0.1):
    """With multi_instance (SPEC 8.10-8.12; off by default, the rest of this text): targets may have inst_count > 1; the
    dataset supplies gt_poses(scene_id, im_id, obj_id) -> [G,4,4] and optionally gt_visib(...) -> [G] visible fractions
    (or None), an instance counting iff its fraction is >= visib_gt_min; the inst_count best-scored rows of a target are
    evaluated against all its instances -> instance_recall's dict plus "rows" (vsd [G][T], mssd [G], mspd [G] each, in the
    order of "match").

    results: rows (dicts) with scene_id, im_id, obj_id, score and pose (4x4 in the dataset's unit), e.g.
    read_results_csv's. dataset: an object with mesh(obj_id) -> render.Mesh or (vertices, faces), model_info(obj_id) -> dict
    with "diameter" and optional symmetries, frame(scene_id, im_id) -> (depth [H,W], cam_K), gt_pose(scene_id, im_id, obj_id)
    -> [4,4], `targets`, and optionally `delta` / `z_near` (defaults 0.015 / 0.05: metres). Rows are grouped by object, the
    highest-scored row of every target is evaluated -> average_recall's dict plus "rows": the evaluated rows with their
    vsd / mssd / mspd."""
    if multi_instance:
        return _evaluate_instances(results, dataset, visib_gt_min)
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
        self._gt, self._cam, self._gt_info = {}, {}, {}

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

    def _instances(self, scene_id, im_id, obj_id):
        """Indices into the image's scene_gt list of the object's instances, in file order (SPEC 8.10)."""
        gt = self._scene(self._gt, scene_id, "scene_gt.json")[int(im_id)]
        idx = [i for i, g in enumerate(gt) if int(g["obj_id"]) == int(obj_id)]
        if not idx:
            raise ValueError("scene %d image %d has no instance of object %d" % (scene_id, im_id, obj_id))
        return gt, idx

    def gt_poses(self, scene_id, im_id, obj_id):
        """f64 [G,4,4]: every instance of the object in the image, in file order (evaluate(..., multi_instance=True))."""
        gt, idx = self._instances(scene_id, im_id, obj_id)
        out = np.tile(np.eye(4), (len(idx), 1, 1))
        for n, i in enumerate(idx):
            out[n, :3, :3] = np.asarray(gt[i]["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
            out[n, :3, 3] = np.asarray(gt[i]["cam_t_m2c"], dtype=np.float64).reshape(3)
        return out

    def gt_visib(self, scene_id, im_id, obj_id):
        """f64 [G]: the instances' visib_fract from scene_gt_info.json, or None when the scene has no such file."""
        if not os.path.exists(os.path.join(self.split, "%06d" % scene_id, "scene_gt_info.json")):
            return None
        _gt, idx = self._instances(scene_id, im_id, obj_id)
        info = self._scene(self._gt_info, scene_id, "scene_gt_info.json")[int(im_id)]
        return np.asarray([float(info[i]["visib_fract"]) for i in idx], dtype=np.float64)
