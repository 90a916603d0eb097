"""Independent numpy restatement of SPEC.md section 8 (BOP-19 pose errors: VSD, MSSD, MSPD, recall), the yardstick of
csrc/bop_eval.hip and ossid_code_amd/bop_eval.py. Nothing here imports the package's evaluation code; the renders come from
ref_raster.render (SPEC 7) with pixel_offset = 0.

Everything is float64 with the written parenthesisation, one numpy operation per written operation (numpy does not contract a
multiply and an add), correctly rounded / and sqrt. Matrix products are spelled out: a BLAS may fuse.
"""
import numpy as np

import ref_raster as rr

F32 = np.float32
DEFAULT_TAUS = np.array([k * 0.05 for k in range(1, 11)])


def cam4(cam_K):
    """fx, fy, cx, cy as the f32 values the device gets."""
    K = np.asarray(cam_K, dtype=np.float64)
    return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]).astype(F32)


# ---- 8.3-8.5 ----------------------------------------------------------------------------------------------------------------
def distance_scale(hw, cam):
    """s [H,W] f64: distance from the camera centre = Z * s (8.3)."""
    H, W = hw
    fx, fy, cx, cy = (float(v) for v in np.asarray(cam, dtype=F32))
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        a = (x - cx) / fx
        b = (y - cy) / fy
        return np.sqrt((a * a + b * b) + 1.0)


def vsd_from_renders(O, cam, Z_est, Z_gt, diameter, delta=0.015, taus=None):
    """One estimate: observed depth O, the two renders f32 [H,W] -> (counts int32 [T+2], errors f64 [T])."""
    taus = DEFAULT_TAUS if taus is None else np.asarray(taus, dtype=np.float64)
    O, Z_est, Z_gt = (np.asarray(a, dtype=F32) for a in (O, Z_est, Z_gt))
    s = distance_scale(O.shape, cam)
    with np.errstate(all="ignore"):
        Do, De, Dg = O.astype(np.float64) * s, Z_est.astype(np.float64) * s, Z_gt.astype(np.float64) * s
        oinv = ~(O > 0)
        Vg = (Dg > 0) & (oinv | (Dg - Do <= delta))
        Ve = ((De > 0) & (oinv | (De - Do <= delta))) | (Vg & (De > 0))
        I, U = Vg & Ve, Vg | Ve
        d = np.abs(Dg - De)[I] / float(diameter)
    nU, nI = int(U.sum()), int(I.sum())
    c = [int((d >= t).sum()) for t in taus]
    err = np.array([1.0 if nU == 0 else float(ck + (nU - nI)) / float(nU) for ck in c])
    return np.array([nU, nI] + c, dtype=np.int32), err


def vsd(V, F, diameter, depth_obs, cam_K, pose_est, pose_gt, frame=None, delta=0.015, taus=None, z_near=0.05):
    """Mesh (V, F) rendered by ref_raster at both poses -> (counts [N,T+2], errors [N,T]). depth_obs [H,W] or [Fr,H,W],
    cam_K [3,3] or [Fr,3,3]."""
    O = np.asarray(depth_obs, dtype=F32)
    O = O[None] if O.ndim == 2 else O
    K = np.asarray(cam_K, dtype=np.float64)
    K = np.repeat(K[None], len(O), 0) if K.ndim == 2 else K
    pe, pg = np.asarray(pose_est).reshape(-1, 4, 4), np.asarray(pose_gt).reshape(-1, 4, 4)
    frame = np.zeros(len(pe), dtype=np.int64) if frame is None else np.asarray(frame)
    counts, errors = [], []
    for n in range(len(pe)):
        f = int(frame[n])
        hw = O[f].shape
        ze = rr.render(V, F, pe[n], K[f], hw, pixel_offset=0.0, z_near=z_near)[0]
        zg = rr.render(V, F, pg[n], K[f], hw, pixel_offset=0.0, z_near=z_near)[0]
        c, e = vsd_from_renders(O[f], cam4(K[f]), ze, zg, diameter, delta, taus)
        counts.append(c), errors.append(e)
    return np.stack(counts), np.stack(errors)


# ---- 8.6 --------------------------------------------------------------------------------------------------------------------
def symmetry_transformations(info, max_sym_disc_step=0.01):
    """models_info entry -> f64 [S,4,4]."""
    disc = [np.eye(4)]
    for m in info.get("symmetries_discrete", []):
        disc.append(np.asarray(m, dtype=np.float64).reshape(4, 4))
    cont = []
    for sym in info.get("symmetries_continuous", []):
        axis = np.asarray(sym["axis"], dtype=np.float64)
        axis = axis / np.sqrt(axis @ axis)
        off = np.asarray(sym["offset"], dtype=np.float64)
        n = int(np.ceil(np.pi / max_sym_disc_step))
        Kx = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        for i in range(n):
            th = i * (2.0 * np.pi / n)
            R = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R, -(R @ off) + off
            cont.append(T)
    out = []
    for D in disc:
        if not cont:
            out.append(D)
        for Cm in cont:
            T = np.eye(4)
            T[:3, :3] = Cm[:3, :3] @ D[:3, :3]
            T[:3, 3] = Cm[:3, :3] @ D[:3, 3] + Cm[:3, 3]
            out.append(T)
    if len(out) > 4096:
        raise ValueError("more than 4096 symmetry transformations")
    return np.stack(out)


# ---- 8.7 --------------------------------------------------------------------------------------------------------------------
def _compose(Pg, S):
    G = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            G[r, c] = (Pg[r, 0] * S[0, c] + Pg[r, 1] * S[1, c]) + Pg[r, 2] * S[2, c]
        G[r, 3] = ((Pg[r, 0] * S[0, 3] + Pg[r, 1] * S[1, 3]) + Pg[r, 2] * S[2, 3]) + Pg[r, 3]
    return G


def _transform(M, P):
    return [((M[r, 0] * P[:, 0] + M[r, 1] * P[:, 1]) + M[r, 2] * P[:, 2]) + M[r, 3] for r in range(3)]


def _project(X, Y, Z, cam):
    fx, fy, cx, cy = (float(v) for v in np.asarray(cam, dtype=F32))
    u = (X / Z) * fx + cx
    v = (Y / Z) * fy + cy
    ok = (Z > 0) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & np.isfinite(u) & np.isfinite(v)
    return u, v, ok


def mssd_mspd(vertices, syms, pose_est, pose_gt, cam_K, frame=None):
    """vertices [V,3] (cast to f32 first, as the device holds them) -> (mssd f64 [N], mspd f64 [N])."""
    P = np.asarray(vertices).astype(F32).astype(np.float64)
    syms = np.asarray(syms, dtype=np.float64).reshape(-1, 4, 4)
    K = np.asarray(cam_K, dtype=np.float64)
    K = K[None] if K.ndim == 2 else K
    pe, pg = np.asarray(pose_est, dtype=np.float64).reshape(-1, 4, 4), np.asarray(pose_gt, dtype=np.float64).reshape(-1, 4, 4)
    frame = np.zeros(len(pe), dtype=np.int64) if frame is None else np.asarray(frame)
    mssd, mspd = np.empty(len(pe)), np.empty(len(pe))
    with np.errstate(all="ignore"):
        for n in range(len(pe)):
            cam = cam4(K[int(frame[n])])
            Xe, Ye, Ze = _transform(pe[n], P)
            ue, ve, oke = _project(Xe, Ye, Ze, cam)
            best3, best2 = np.inf, np.inf
            for S in syms:
                Xg, Yg, Zg = _transform(_compose(pg[n], S), P)
                dx, dy, dz = Xe - Xg, Ye - Yg, Ze - Zg
                q = (dx * dx + dy * dy) + dz * dz
                q = np.where(np.isnan(q), np.inf, q)
                best3 = min(best3, float(np.sqrt(q.max())))
                ug, vg, okg = _project(Xg, Yg, Zg, cam)
                du, dv = ue - ug, ve - vg
                p = np.where(oke & okg, du * du + dv * dv, np.inf)
                best2 = min(best2, float(np.sqrt(p.max())))
            mssd[n], mspd[n] = best3, best2
    return mssd, mspd


# ---- 8.8 --------------------------------------------------------------------------------------------------------------------
THETAS = [k * 0.05 for k in range(1, 11)]


def average_recall(rows, targets, diameters, image_width):
    """rows: dicts scene_id, im_id, obj_id, score, vsd [T], mssd, mspd; targets: (scene_id, im_id, obj_id) triples."""
    keys = [tuple(int(v) for v in t) for t in targets]
    if len(set(keys)) != len(keys):
        raise ValueError("a target is listed twice")
    best = {}
    for r in rows:
        k = (int(r["scene_id"]), int(r["im_id"]), int(r["obj_id"]))
        if k in keys and (k not in best or r["score"] > best[k]["score"]):
            best[k] = r
    n = float(len(keys))
    T = len(next(iter(best.values()))["vsd"]) if best else 0
    rec_vsd = [[sum(1 for k in keys if k in best and best[k]["vsd"][t] < th) / n for th in THETAS] for t in range(T)]
    rec_mssd = [sum(1 for k in keys if k in best and best[k]["mssd"] < th * diameters[k[2]]) / n for th in THETAS]
    ratio = float(image_width) / 640.0
    rec_mspd = [sum(1 for k in keys if k in best and best[k]["mspd"] < (5.0 * j) * ratio) / n for j in range(1, 11)]
    ar_vsd = float(np.mean(rec_vsd)) if T else 0.0
    ar_mssd, ar_mspd = float(np.mean(rec_mssd)), float(np.mean(rec_mspd))
    return {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0,
            "recall_vsd": rec_vsd, "recall_mssd": rec_mssd, "recall_mspd": rec_mspd}


# ---- test meshes with symmetries ----------------------------------------------------------------------------------------------
def prism_mesh(a=0.03, h=0.05):
    """Square prism, side 2a, height 2h along z: four discrete symmetries about z (0, 90, 180, 270 degrees)."""
    V = np.array([[sx * a, sy * a, sz * h] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], dtype=np.float64)
    F = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6],
                  [1, 3, 5], [3, 7, 5]], dtype=np.int32)
    return V, F


def rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def lathe_mesh(n_seg=48):
    """Surface of revolution about z of a vase-like profile r(z) -> (V, F, r_max)."""
    prof = np.array([[0.010, -0.04], [0.030, -0.03], [0.022, 0.0], [0.035, 0.025], [0.012, 0.04]])
    ang = np.arange(n_seg) * (2.0 * np.pi / n_seg)
    V = np.array([[r * np.cos(t), r * np.sin(t), z] for r, z in prof for t in ang])
    F = []
    for i in range(len(prof) - 1):
        for j in range(n_seg):
            a, b = i * n_seg + j, i * n_seg + (j + 1) % n_seg
            F += [[a, b, a + n_seg], [b, b + n_seg, a + n_seg]]
    return V, np.asarray(F, dtype=np.int32), float(prof[:, 0].max())


# ---- a tiny BOP folder ---------------------------------------------------------------------------------------------------------
def write_ply_ascii(path, V, F):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(V))
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(F))
        for v in V:
            f.write("%r %r %r\n" % tuple(float(x) for x in v))
        for t in F:
            f.write("3 %d %d %d\n" % tuple(int(i) for i in t))


def write_bop_folder(root, name="tiny", split="test", hw=(60, 80)):
    """Two objects (a prism with discrete symmetries, a lathe with a continuous one) in millimetres, one scene of three
    images whose depth is a flat wall at 900 mm -> (targets, {key: gt pose})."""
    import json
    import os

    from PIL import Image
    base = os.path.join(root, name)
    os.makedirs(os.path.join(base, "models_eval"))
    Vp, Fp = prism_mesh()
    Vl, Fl, _r = lathe_mesh(24)
    write_ply_ascii(os.path.join(base, "models_eval", "obj_000001.ply"), Vp * 1000.0, Fp)
    write_ply_ascii(os.path.join(base, "models_eval", "obj_000002.ply"), Vl * 1000.0, Fl)
    info = {"1": {"diameter": 116.0, "symmetries_discrete": [rot_z(a).reshape(-1).tolist() for a in (90, 180, 270)]},
            "2": {"diameter": 106.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}}
    json.dump(info, open(os.path.join(base, "models_eval", "models_info.json"), "w"))
    H, W = hw
    K = [100.0, 0.0, 40.0, 0.0, 100.0, 30.0, 0.0, 0.0, 1.0]
    sdir = os.path.join(base, split, "000003")
    os.makedirs(os.path.join(sdir, "depth"))
    gt, cams, targets, poses = {}, {}, [], {}
    for im in range(3):
        rows = []
        for obj, t in ((1, (-60.0 + 10 * im, 20.0, 700.0)), (2, (70.0, -30.0 + 5 * im, 650.0))):
            T = rr.pose_at(t, axis=(0.3, 1.0, 0.2 + im), deg=25.0 + 10 * im)
            rows.append({"obj_id": obj, "cam_R_m2c": T[:3, :3].reshape(-1).tolist(), "cam_t_m2c": T[:3, 3].tolist()})
            targets.append({"scene_id": 3, "im_id": im, "obj_id": obj, "inst_count": 1})
            poses[(3, im, obj)] = T
        gt[str(im)], cams[str(im)] = rows, {"cam_K": K, "depth_scale": 0.5}
        Image.fromarray(np.full((H, W), 1800, dtype=np.uint16)).save(os.path.join(sdir, "depth", "%06d.png" % im))
    json.dump(gt, open(os.path.join(sdir, "scene_gt.json"), "w"))
    json.dump(cams, open(os.path.join(sdir, "scene_camera.json"), "w"))
    json.dump(targets, open(os.path.join(base, "test_targets_bop19.json"), "w"))
    return targets, poses
