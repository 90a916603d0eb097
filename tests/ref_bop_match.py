"""Independent numpy restatement of SPEC.md 8.10-8.12 (BOP-19 targets with several instances: groups and kept estimates,
pair errors, the greedy matching, recall), the yardstick of ossid_bop_vsd_pairs / ossid_bop_match (csrc/bop_eval.hip) and
of bop_eval.vsd_pairs / match_instances / instance_recall / evaluate(..., multi_instance=True). Nothing here imports the
package's evaluation code. The pair errors are tests/ref_bop_eval.py's own functions on rows expanded one per pair; the
matching is the nested loop as 8.12 writes it. Like 8.1-8.9 this restates the published definition (bop_toolkit's
pose_matching and eval_calc_scores, which are in neither tree); parity with bop_toolkit is unpinned.
"""
import json
import os

import numpy as np

import ref_bop_eval as rb
import ref_raster as rr

MAX_INSTANCES = 64
THETAS = [k * 0.05 for k in range(1, 11)]
THETAS_PX = [5.0 * k for k in range(1, 11)]


# ---- 8.10 -------------------------------------------------------------------------------------------------------------------
def groups_of(targets):
    """[((scene_id, im_id, obj_id), inst_count)] in the targets' order."""
    out = []
    for t in targets:
        if isinstance(t, dict):
            out.append(((int(t["scene_id"]), int(t["im_id"]), int(t["obj_id"])), int(t.get("inst_count", 1))))
        else:
            out.append((tuple(int(v) for v in t), 1))
    for key, n in out:
        if n < 1 or n > MAX_INSTANCES:
            raise ValueError("target %r: inst_count %d" % (key, n))
    if len(set(k for k, _n in out)) != len(out) or not out:
        raise ValueError("a target is listed twice, or there is none")
    return out


def kept_estimates(rows, key, n):
    """The rows of `key` by score descending, ties by input order; the first n."""
    mine = [(i, r) for i, r in enumerate(rows) if (int(r["scene_id"]), int(r["im_id"]), int(r["obj_id"])) == key]
    order = []
    while mine:                                                  # selection by hand: the best remaining, the earliest among equals
        best = 0
        for j in range(1, len(mine)):
            if float(mine[j][1]["score"]) > float(mine[best][1]["score"]):
                best = j
        order.append(mine.pop(best)[1])
    return order[:n]


# ---- 8.11 -------------------------------------------------------------------------------------------------------------------
def pair_errors(V, F, info, depth, cam_K, poses_est, poses_gt, delta, z_near, taus=None):
    """One image: every (e, g) pair expanded into a row of its own -> vsd [E][G][T], mssd [E][G], mspd [E][G]. Each pose is
    rendered once here too -- rb.vsd would render the same pose again for every pair, with the same image."""
    E, G = len(poses_est), len(poses_gt)
    hw = np.asarray(depth).shape
    ze = [rr.render(V, F, p, cam_K, hw, pixel_offset=0.0, z_near=z_near)[0] for p in poses_est]
    zg = [rr.render(V, F, p, cam_K, hw, pixel_offset=0.0, z_near=z_near)[0] for p in poses_gt]
    cam = rb.cam4(cam_K)
    vsd = np.array([[rb.vsd_from_renders(depth, cam, ze[e], zg[g], info["diameter"], delta, taus)[1] for g in range(G)]
                    for e in range(E)]).reshape(E, G, len(rb.DEFAULT_TAUS if taus is None else taus))
    pe = np.array([poses_est[e] for e in range(E) for _g in range(G)]).reshape(-1, 4, 4)
    pg = np.array([poses_gt[g] for _e in range(E) for g in range(G)]).reshape(-1, 4, 4)
    if E:
        m3, m2 = rb.mssd_mspd(V, rb.symmetry_transformations(info), pe, pg, cam_K)
    else:
        m3, m2 = np.zeros(0), np.zeros(0)
    return vsd, m3.reshape(E, G), m2.reshape(E, G)


# ---- 8.12 -------------------------------------------------------------------------------------------------------------------
def match_group(err, thr):
    """err [E][G][K], thr [K][10] -> match int [E][K][10]."""
    E, G, K = err.shape
    match = -np.ones((E, K, 10), dtype=np.int32)
    for k in range(K):
        errs = np.asarray(err[:, :, k], dtype=np.float64).tolist()      # Python floats are the same doubles
        for j in range(10):
            th = float(thr[k][j])
            taken = [False] * G
            for e in range(E):
                best = -1
                for g in range(G):
                    if taken[g] or not errs[e][g] < th:                  # a NaN is never below
                        continue
                    if best < 0 or errs[e][g] < errs[e][best]:           # equal errors: the lower g stays
                        best = g
                if best >= 0:
                    taken[best] = True
                    match[e, k, j] = best
    return match


def match_instances(err, E, G, valid, thr):
    """The flat tables of bop_eval.match_instances -> (match int32 [sum E][K][10], tp int32 [K][10])."""
    thr = np.asarray(thr, dtype=np.float64)
    K = thr.shape[1]
    err = np.asarray(err, dtype=np.float64).reshape(-1, K)
    valid = np.asarray(valid).reshape(-1) != 0
    out, tp, p0, i0 = [], np.zeros((K, 10), dtype=np.int32), 0, 0
    for i in range(len(E)):
        e, g = int(E[i]), int(G[i])
        m = match_group(err[p0:p0 + e * g].reshape(e, g, K), thr[i])
        for row in m.reshape(-1, K, 10):
            for k in range(K):
                for j in range(10):
                    if row[k, j] >= 0 and valid[i0 + row[k, j]]:
                        tp[k, j] += 1
        out.append(m)
        p0, i0 = p0 + e * g, i0 + g
    return np.concatenate(out).astype(np.int32), tp


def instance_recall(rows, targets, diameters, image_width, valid=None):
    """rows: dicts scene_id, im_id, obj_id, score, vsd [G][T], mssd [G], mspd [G] -> the scores and the match table."""
    groups = groups_of(targets)
    total = float(sum(n for _k, n in groups))
    T = None
    for key, n in groups:
        for r in kept_estimates(rows, key, n):
            T = np.atleast_2d(r["vsd"]).shape[1]
    if T is None:
        zero = [0.0] * 10
        return {"AR_VSD": 0.0, "AR_MSSD": 0.0, "AR_MSPD": 0.0, "AR": 0.0, "recall_vsd": [], "recall_mssd": zero, "recall_mspd": zero,
                "match": np.zeros((0, 2, 10), np.int32)}
    tp, matches = np.zeros((T + 2, 10), dtype=np.int64), []
    ratio = float(image_width) / 640.0
    for key, n in groups:
        kept = kept_estimates(rows, key, n)
        if not kept:
            continue
        err = np.array([np.concatenate([np.atleast_2d(r["vsd"]), np.atleast_1d(r["mssd"])[:, None], np.atleast_1d(r["mspd"])[:, None]], 1)
                        for r in kept], dtype=np.float64)                       # [E][G][T+2]
        G = err.shape[1]
        if G > MAX_INSTANCES:
            raise ValueError("target %r: %d instances" % (key, G))
        ok = np.ones(G, bool) if valid is None or key not in valid else np.asarray(valid[key]).reshape(-1) != 0
        thr = np.array([THETAS] * T + [[th * float(diameters[key[2]]) for th in THETAS]] + [[px * ratio for px in THETAS_PX]])
        m = match_group(err, thr)
        matches.append(m)
        tp += ((m >= 0) & ok[np.maximum(m, 0)]).sum(0)
    rec = tp / total
    rec_vsd, rec_mssd, rec_mspd = [list(map(float, rec[t])) for t in range(T)], list(map(float, rec[T])), list(map(float, rec[T + 1]))
    ar_vsd, ar_mssd, ar_mspd = float(np.mean(rec_vsd)), float(np.mean(rec_mssd)), float(np.mean(rec_mspd))
    return {"AR_VSD": ar_vsd, "AR_MSSD": ar_mssd, "AR_MSPD": ar_mspd, "AR": (ar_vsd + ar_mssd + ar_mspd) / 3.0,
            "recall_vsd": rec_vsd, "recall_mssd": rec_mssd, "recall_mspd": rec_mspd, "match": np.concatenate(matches)}


def evaluate(ds, results, delta, z_near, visib_gt_min=0.1):
    """ds: mesh, model_info, frame, gt_poses, optional gt_visib, targets -> (rows with their pair errors, the scores)."""
    groups = groups_of(ds.targets)
    rows, valid, diameters, width = [], {}, {}, None
    for key, n in groups:
        V, F = ds.mesh(key[2])
        info = ds.model_info(key[2])
        diameters[key[2]] = float(info["diameter"])
        depth, K = ds.frame(key[0], key[1])
        width = np.asarray(depth).shape[1]
        gts = np.asarray(ds.gt_poses(*key), dtype=np.float64).reshape(-1, 4, 4)
        visib = ds.gt_visib(*key) if hasattr(ds, "gt_visib") else None
        valid[key] = np.ones(len(gts), bool) if visib is None else np.asarray(visib) >= visib_gt_min
        kept = kept_estimates(results, key, n)
        vsd, m3, m2 = pair_errors(V, F, info, depth, K, [r["pose"] for r in kept], gts, delta, z_near)
        for e, r in enumerate(kept):
            rows.append({"scene_id": key[0], "im_id": key[1], "obj_id": key[2], "score": r["score"], "vsd": vsd[e].tolist(),
                         "mssd": m3[e].tolist(), "mspd": m2[e].tolist()})
    return rows, instance_recall(rows, ds.targets, diameters, width, valid)


# ---- a BOP folder whose targets have several instances -----------------------------------------------------------------------------
def write_bop_folder(root, V, F, diameter, scenes, cam_K, name="multi", split="test", with_gt_info=True):
    """One object (obj 1, vertices in millimetres) in the layout of ref_bop_eval.write_bop_folder. scenes: {scene_id:
    (depth u16 [H,W] at depth_scale 1, [pose_gt ...], [visib_fract ...])}; every scene holds image 0 and one target with
    inst_count = its number of instances -> targets."""
    from PIL import Image
    base = os.path.join(root, name)
    os.makedirs(os.path.join(base, "models_eval"))
    rb.write_ply_ascii(os.path.join(base, "models_eval", "obj_000001.ply"), V, F)
    json.dump({"1": {"diameter": float(diameter)}}, open(os.path.join(base, "models_eval", "models_info.json"), "w"))
    targets = []
    for sid, (depth, poses, visib) in scenes.items():
        sdir = os.path.join(base, split, "%06d" % sid)
        os.makedirs(os.path.join(sdir, "depth"))
        Image.fromarray(np.asarray(depth, dtype=np.uint16)).save(os.path.join(sdir, "depth", "%06d.png" % 0))
        gt = [{"obj_id": 1, "cam_R_m2c": T[:3, :3].reshape(-1).tolist(), "cam_t_m2c": T[:3, 3].tolist()} for T in poses]
        json.dump({"0": gt}, open(os.path.join(sdir, "scene_gt.json"), "w"))
        json.dump({"0": {"cam_K": np.asarray(cam_K).reshape(-1).tolist(), "depth_scale": 1.0}}, open(os.path.join(sdir, "scene_camera.json"), "w"))
        if with_gt_info:
            json.dump({"0": [{"visib_fract": float(v)} for v in visib]}, open(os.path.join(sdir, "scene_gt_info.json"), "w"))
        targets.append({"scene_id": sid, "im_id": 0, "obj_id": 1, "inst_count": len(poses)})
    json.dump(targets, open(os.path.join(base, "test_targets_bop19.json"), "w"))
    return targets
