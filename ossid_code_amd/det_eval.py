"""Detection mAP on the device (csrc/det_eval.hip, SPEC.md section 10): the second figure the reference's run ends with --

    evalFinetuneResults(save_path, DATASET_NAME, tmp_root)                           scripts/online_learning.py:615-618
    runMapEval: subprocess.run(['python', 'main.py', '--no-animation', '--no-plot'])  utils/detection.py:97-135

The script the reference shells out to is in neither tree; the metric's arithmetic that IS in the reference tree is
DetectionMetric.calculate_mAP (utils/detection_metrics.py:20-156), an 11-point AP, and the recorded fixture
tests/golden/det_map.npz pins this module to it. The all-point AP (SPEC 10.8) is what the external script is understood to
report; parity with it is unpinned.

match is the device path on device tensors; evaluate validates (SPEC 10.1), uploads and reads back; DetectionMetric has the
reference class's signature; read_det_folder / runMapEval / evalFinetuneResults work on the text files
pipeline.save_det_results writes; summary gives the three recall figures the run prints; tools/eval_det_map.py is the
command line.
"""
import os
import pickle
import re

import numpy as np
import torch

from . import _lib

N_MAX, G_MAX, I_MAX, C_MAX = 1 << 22, 1 << 20, 1 << 20, 4096          # SPEC 10.1
ST_FP, ST_TP, ST_IGNORED, ST_DUP = 0, 1, 2, 3                         # status codes of ossid_det_match
REC_THR = tuple(float(np.float32(float(j) * 0.1)) for j in range(11))  # 10.1: t_j = f32((double) j * 0.1)


def _as_tensor(a, dtype, device=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if device is not None:
        t = t.to(device)
    return t.to(dtype).contiguous()


def _thresholds(iou_thresholds):
    thr = np.ascontiguousarray(iou_thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= len(thr) <= _lib.DET_MAX_THRESHOLDS or not np.isfinite(thr).all():
        raise ValueError("iou_thresholds must be 1 to %d finite values, got %r" % (_lib.DET_MAX_THRESHOLDS, iou_thresholds))
    return thr


def _check_sizes(N, G, I, C):
    if not 1 <= C <= C_MAX:
        raise ValueError("%d classes (1 to %d)" % (C, C_MAX))
    if not 1 <= I <= I_MAX:
        raise ValueError("%d images (1 to %d)" % (I, I_MAX))
    if N > N_MAX or G > G_MAX:
        raise ValueError("%d detections (at most %d), %d ground truths (at most %d)" % (N, N_MAX, G, G_MAX))


def validate(det_box, det_score, det_cls, det_image, gt_box, gt_cls, gt_image, n_images, n_classes):
    """The refusals of SPEC 10.1, on tensors wherever they live (host tensors never touch the device). ValueError."""
    N, G = int(det_cls.shape[0]), int(gt_cls.shape[0])
    _check_sizes(N, G, n_images, n_classes)
    if tuple(det_box.shape) != (N, 4) or tuple(det_score.shape) != (N,) or tuple(det_image.shape) != (N,):
        raise ValueError("detections: boxes [N,4], scores [N], classes [N], images [N] with one N")
    if tuple(gt_box.shape) != (G, 4) or tuple(gt_image.shape) != (G,):
        raise ValueError("ground truths: boxes [G,4], classes [G], images [G] with one G")
    if N and not (bool(torch.isfinite(det_box).all()) and bool(torch.isfinite(det_score).all())):
        raise ValueError("a detection has a non-finite coordinate or score")
    if G and not bool(torch.isfinite(gt_box).all()):
        raise ValueError("a ground truth has a non-finite coordinate")
    for what, t, hi in (("detection class", det_cls, n_classes), ("detection image", det_image, n_images),
                        ("ground-truth class", gt_cls, n_classes), ("ground-truth image", gt_image, n_images)):
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= hi):
            raise ValueError("a %s is outside [0, %d)" % (what, hi))
    if G > 1 and bool((gt_image[1:] < gt_image[:-1]).any()):
        raise ValueError("ground truths are not grouped by image (their image indices must not decrease)")


def class_offsets(det_cls, n_classes):
    """int32 [C+1]: class c owns the ranks [out[c], out[c+1]) of the sorted keys. scatter_add_, not bincount: bincount reads
    the input's maximum back to the host to size its output, which synchronises and cannot be captured."""
    counts = torch.zeros(n_classes, dtype=torch.int64, device=det_cls.device)
    if det_cls.numel():
        idx = det_cls.to(torch.int64).clamp(0, n_classes - 1)
        counts.scatter_add_(0, idx, torch.ones_like(idx))
    out = torch.zeros(n_classes + 1, dtype=torch.int32, device=det_cls.device)
    out[1:] = torch.cumsum(counts, 0)
    return out


def match(det_box, det_score, det_cls, det_image, gt_box, gt_cls, gt_offset, n_classes, gt_difficult=None,
          iou_thresholds=(0.5,), curves=False):
    """Device tensors in (f32 [N,4], f32 [N], int32 [N], int32 [N]; f32 [G,4], int32 [G], int32 [I+1] CSR by image, u8 [G]
    or None), device tensors out: a dict with best_gt int32 [N], best_iou f32 [N], order int32 [N] (the rank permutation of
    10.4), class_offset int32 [C+1], status u8 [T,N] by input index, n_easy int32 [C], p11 f32 [T,C,11], ap11 f32 [T,C], apa
    f64 [T,C], map11 f32 [T], mapa f64 [T]; with curves=True also ctp, cfp int32 and prec, rec, env f32, [T,N] in rank
    order. Shapes, dtypes and the device are checked; the CONTENTS are not (validate does that). Nothing is read back and
    nothing synchronises: the claim launch, the library's sort, a scatter_add_ and the match launches."""
    _lib.require_cuda(det_box, det_score, det_cls, det_image, gt_box, gt_cls, gt_offset, gt_difficult)
    thr = _thresholds(iou_thresholds)
    N, G, I, C, T = int(det_cls.shape[0]), int(gt_cls.shape[0]), int(gt_offset.shape[0]) - 1, int(n_classes), len(thr)
    _check_sizes(N, G, I, C)
    dev = det_box.device
    want = ((det_box, torch.float32), (det_score, torch.float32), (det_cls, torch.int32), (det_image, torch.int32),
            (gt_box, torch.float32), (gt_cls, torch.int32), (gt_offset, torch.int32))
    if any(t.dtype != d or t.device != dev for t, d in want) or (gt_difficult is not None and gt_difficult.dtype != torch.uint8):
        raise ValueError("match takes f32 boxes and scores, int32 indices and u8 difficult flags on one device")
    shapes = ((det_box, (N, 4)), (det_score, (N,)), (det_cls, (N,)), (det_image, (N,)), (gt_box, (G, 4)), (gt_cls, (G,)),
              (gt_offset, (I + 1,))) + (() if gt_difficult is None else ((gt_difficult, (G,)),))
    if any(tuple(t.shape) != sh for t, sh in shapes) or (gt_difficult is not None and gt_difficult.device != dev):
        raise ValueError("match takes boxes [N,4] / [G,4], scores, classes and images [N], classes and difficult flags [G] and "
                         "gt_offset [I+1], got %s" % ([tuple(t.shape) for t, _sh in shapes],))
    best_gt = torch.empty(N, dtype=torch.int32, device=dev)
    best_iou = torch.empty(N, dtype=torch.float32, device=dev)
    key = torch.empty(N, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_det_claim")(_lib.ptr(det_box), _lib.ptr(det_score), _lib.ptr(det_cls), _lib.ptr(det_image), N,
                                        _lib.ptr(gt_box), _lib.ptr(gt_cls), _lib.ptr(gt_offset), G, I, C, best_gt.data_ptr(),
                                        best_iou.data_ptr(), key.data_ptr(), _lib.stream())
        _lib.check(rc, "ossid_det_claim")
        # plumbing, not the metric: the library's stable sort of the kernel's keys, and the classes' offsets in it
        order = torch.sort(key, stable=True)[1].to(torch.int32)
        class_offset = class_offsets(det_cls, C)
        out = {"best_gt": best_gt, "best_iou": best_iou, "order": order, "class_offset": class_offset,
               "status": torch.empty(T, N, dtype=torch.uint8, device=dev), "n_easy": torch.empty(C, dtype=torch.int32, device=dev),
               "p11": torch.empty(T, C, 11, dtype=torch.float32, device=dev), "ap11": torch.empty(T, C, dtype=torch.float32, device=dev),
               "apa": torch.empty(T, C, dtype=torch.float64, device=dev), "map11": torch.empty(T, dtype=torch.float32, device=dev),
               "mapa": torch.empty(T, dtype=torch.float64, device=dev)}
        cur = [None] * 5
        if curves:
            for i, (name, dt) in enumerate((("ctp", torch.int32), ("cfp", torch.int32), ("prec", torch.float32),
                                            ("rec", torch.float32), ("env", torch.float32))):
                out[name] = cur[i] = torch.empty(T, N, dtype=dt, device=dev)
        nbytes = _lib.fn("ossid_det_eval_workspace_bytes")(N, G, C, T)
        ws = torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=dev)
        rc = _lib.fn("ossid_det_match")(best_gt.data_ptr(), best_iou.data_ptr(), order.data_ptr(), class_offset.data_ptr(), N,
                                        _lib.ptr(gt_cls), _lib.ptr(gt_difficult), G, C, thr.ctypes.data, T, ws.data_ptr(), int(nbytes),
                                        out["status"].data_ptr(), out["n_easy"].data_ptr(), out["p11"].data_ptr(),
                                        out["ap11"].data_ptr(), out["apa"].data_ptr(), out["map11"].data_ptr(), out["mapa"].data_ptr(),
                                        *[_lib.ptr(t) for t in cur], _lib.stream())
        _lib.check(rc, "ossid_det_match")
    return out


def _top_filter(det_cls, det_image, n_classes, top):
    """Rows kept by top=k: each (image, class)'s first k detections in input order (host)."""
    grp = det_image.astype(np.int64) * n_classes + det_cls.astype(np.int64)
    o = np.argsort(grp, kind="stable")
    g = grp[o]
    start = np.r_[True, g[1:] != g[:-1]] if len(g) else np.zeros(0, bool)
    first = np.maximum.accumulate(np.where(start, np.arange(len(g)), 0)) if len(g) else np.zeros(0, np.int64)
    keep = np.zeros(len(g), bool)
    keep[o] = (np.arange(len(g)) - first) < top
    return keep


def evaluate(det, gt, classes, iou_thresholds=(0.5,), top=None, curves=False, n_images=None, device=None):
    """det: {"boxes" [N,4] x1 y1 x2 y2, "scores" [N], "classes" [N] (indices into `classes`), "images" [N]}; gt: {"boxes"
    [G,4], "classes" [G], "images" [G] (not decreasing), optional "difficult" [G]}; numpy arrays or tensors. classes: the
    caller's list of names, in its order. Checks SPEC 10.1 (ValueError before any device work for host inputs), runs match
    and reads back -> {"classes", "iou_thresholds", "AP11" f32 [T,C], "APa" f64 [T,C], "mAP11" [T], "mAPa" [T], "p11"
    [T,C,11], "n_easy" [C], "n_det" [C]}, numpy; with curves=True also "curves": best_gt, best_iou, status, order,
    class_offset, ctp, cfp, prec, rec, env. top=k keeps each (image, class)'s first k detections in input order (top=1 is
    what the reference's evalFinetuneResults does)."""
    classes = list(classes)
    C = len(classes)
    thr = _thresholds(iou_thresholds)
    if top is not None and int(top) < 1:
        raise ValueError("top must be >= 1, got %r" % (top,))
    db, ds = _as_tensor(det["boxes"], torch.float32).reshape(-1, 4), _as_tensor(det["scores"], torch.float32)
    dc, di = _as_tensor(det["classes"], torch.int64), _as_tensor(det["images"], torch.int64)
    gb, gc, gi = _as_tensor(gt["boxes"], torch.float32).reshape(-1, 4), _as_tensor(gt["classes"], torch.int64), _as_tensor(gt["images"], torch.int64)
    gd = gt.get("difficult")
    gd = None if gd is None else _as_tensor(gd, torch.uint8)
    if gd is not None and tuple(gd.shape) != tuple(gc.shape):
        raise ValueError("difficult must be one flag per ground truth")
    if n_images is None:
        n_images = 1 + max([int(t.max()) for t in (di, gi) if t.numel()] + [0])
    validate(db, ds, dc, di, gb, gc, gi, int(n_images), C)
    if top is not None:
        keep = torch.from_numpy(_top_filter(dc.cpu().numpy(), di.cpu().numpy(), C, int(top))).to(dc.device)
        db, ds, dc, di = db[keep], ds[keep], dc[keep], di[keep]
    if device is None:
        device = db.device if db.is_cuda else torch.device("cuda", torch.cuda.current_device())
    off = torch.zeros(int(n_images) + 1, dtype=torch.int64, device=gi.device)
    off[1:] = torch.cumsum(torch.bincount(gi, minlength=int(n_images)), 0) if gi.numel() else 0
    to = lambda t, dt: t.to(device=device, dtype=dt).contiguous()
    m = match(to(db, torch.float32), to(ds, torch.float32), to(dc, torch.int32), to(di, torch.int32), to(gb, torch.float32),
              to(gc, torch.int32), to(off, torch.int32), C, None if gd is None else to(gd, torch.uint8), thr, curves=curves)
    host = {k: v.cpu().numpy() for k, v in m.items()}
    out = {"classes": classes, "iou_thresholds": thr, "AP11": host["ap11"], "APa": host["apa"], "mAP11": host["map11"],
           "mAPa": host["mapa"], "p11": host["p11"], "n_easy": host["n_easy"], "n_det": np.diff(host["class_offset"])}
    if curves:
        out["curves"] = {k: host[k] for k in ("best_gt", "best_iou", "status", "order", "class_offset", "ctp", "cfp", "prec", "rec", "env")}
    return out


class DetectionMetric:
    """The reference class's interface (utils/detection_metrics.py:7-156) on the device: lists of per-image tensors, labels
    from 1 (0 is the background and is dropped, as the reference's loop from 1 never looks at it), the 11-point AP at
    IoU > 0.5 -> ({name: AP}, mAP)."""

    def __init__(self, classes, device=None):
        self.classes = list(classes)
        self.label_map = {k: v + 1 for v, k in enumerate(self.classes)}
        self.label_map["bg"] = 0
        self.rev_label_map = {v: k for k, v in self.label_map.items()}
        self.device = device

    def calculate_mAP(self, det_boxes, det_labels, det_scores, true_boxes, true_labels, true_difficulties=None):
        n = len(det_boxes)
        if not (len(det_labels) == len(det_scores) == len(true_boxes) == len(true_labels) == n) or \
                (true_difficulties is not None and len(true_difficulties) != n):
            raise ValueError("calculate_mAP takes one tensor per image in every list")
        cat = lambda xs, dt, shape: (torch.cat([torch.as_tensor(x).reshape(shape).cpu() for x in xs]) if n else torch.zeros([0 if v < 0 else v for v in shape])).to(dt)
        images = lambda xs: torch.cat([torch.full((int(torch.as_tensor(x).reshape(-1).shape[0]),), i, dtype=torch.int64)
                                       for i, x in enumerate(xs)]) if n else torch.zeros(0, dtype=torch.int64)
        dl, tl = cat(det_labels, torch.int64, (-1,)), cat(true_labels, torch.int64, (-1,))
        kd, kt = dl != 0, tl != 0
        det = {"boxes": cat(det_boxes, torch.float32, (-1, 4))[kd], "scores": cat(det_scores, torch.float32, (-1,))[kd],
               "classes": dl[kd] - 1, "images": images(det_labels)[kd]}
        gt = {"boxes": cat(true_boxes, torch.float32, (-1, 4))[kt], "classes": tl[kt] - 1, "images": images(true_labels)[kt]}
        if true_difficulties is not None:
            gt["difficult"] = (cat(true_difficulties, torch.int64, (-1,))[kt] != 0).to(torch.uint8)
        r = evaluate(det, gt, self.classes, n_images=max(n, 1), device=self.device)
        return {name: float(r["AP11"][0, c]) for c, name in enumerate(self.classes)}, float(r["mAP11"][0])


# ---- the text files of pipeline.save_det_results -------------------------------------------------------------------------------
_FILE = re.compile(r"^s(\d+)_i(\d+)\.txt$")


def read_det_folder(path):
    """{(scene_id, im_id): rows} of a folder of s%06d_i%06d.txt files, files in sorted name order and rows in line order (the
    input order of SPEC 10.4). A 5-field row `name x1 y1 x2 y2` is a ground truth -> (name, x1, y1, x2, y2); a 6-field row
    `name score x1 y1 x2 y2` is a detection -> (name, x1, y1, x2, y2, score). Names stay strings (obj_%06d)."""
    out = {}
    for fn in sorted(os.listdir(path)):
        m = _FILE.match(fn)
        if not m:
            continue
        rows = []
        with open(os.path.join(path, fn)) as f:
            for ln, line in enumerate(f):
                p = line.split()
                if not p:
                    continue
                if len(p) == 5:
                    rows.append((p[0],) + tuple(float(v) for v in p[1:]))
                elif len(p) == 6:
                    rows.append((p[0],) + tuple(float(v) for v in p[2:]) + (float(p[1]),))
                else:
                    raise ValueError("%s line %d: %d fields (5 = ground truth, 6 = detection)" % (fn, ln + 1, len(p)))
        out[(int(m.group(1)), int(m.group(2)))] = rows
    return out


def eval_folders(gt_folder, det_folder, iou_thresholds=(0.5,), top=None):
    """evaluate over two folders of text files. Images: the union of both folders' files in sorted order; classes: the sorted
    union of the names in both."""
    gts, dets = read_det_folder(gt_folder), read_det_folder(det_folder)
    keys = sorted(set(gts) | set(dets))
    index = {k: i for i, k in enumerate(keys)}
    names = sorted(set(r[0] for rows in gts.values() for r in rows) | set(r[0] for rows in dets.values() for r in rows))
    if not names or not keys:
        raise ValueError("no rows in %s and %s" % (gt_folder, det_folder))
    cid = {nm: c for c, nm in enumerate(names)}
    if any(len(r) != 5 for rows in gts.values() for r in rows) or any(len(r) != 6 for rows in dets.values() for r in rows):
        raise ValueError("ground-truth rows have 5 fields and detection rows 6")
    g = [(index[k], cid[r[0]]) + r[1:5] for k in keys for r in gts.get(k, ())]
    d = [(index[k], cid[r[0]]) + r[1:6] for k in keys for r in dets.get(k, ())]
    ga, da = np.asarray(g, dtype=np.float64).reshape(-1, 6), np.asarray(d, dtype=np.float64).reshape(-1, 7)
    det = {"boxes": da[:, 2:6].astype(np.float32), "scores": da[:, 6].astype(np.float32), "classes": da[:, 1].astype(np.int64),
           "images": da[:, 0].astype(np.int64)}
    gt = {"boxes": ga[:, 2:6].astype(np.float32), "classes": ga[:, 1].astype(np.int64), "images": ga[:, 0].astype(np.int64)}
    return evaluate(det, gt, names, iou_thresholds=iou_thresholds, top=top, n_images=len(keys))


def runMapEval(gt_folder, det_folder):
    """utils/detection.py:97-135 without the external script: {obj_name: AP * 100, 'mAP': mean * 100} by the all-point
    method (SPEC 10.8) at IoU > 0.5. The values are unrounded; the reference parses two-decimal percentages from the
    script's stdout."""
    r = eval_folders(gt_folder, det_folder)
    out = {name: float(r["APa"][0, c]) * 100.0 for c, name in enumerate(r["classes"])}
    out["mAP"] = float(r["mAPa"][0]) * 100.0
    return out


def evalFinetuneResults(result_or_path, dataset_name, tmp_root="./DetResults"):
    """utils/detection.py:137-187: the FIRST box of every result row (`for i in range(1)`, :165) goes to
    <tmp_root>/tmp-<dataset_name>, the ground truth is expected in <tmp_root>/gt-<dataset_name> (lmo or ycbv), and the mAP
    of runMapEval is printed and returned. result: a list of dicts, a DataFrame, or the path of the run's pickle."""
    from . import pipeline
    result = result_or_path
    if isinstance(result, (str, os.PathLike)):
        with open(result, "rb") as f:
            result = pickle.load(f)
        if isinstance(result, dict) and "test_results" in result:
            result = result["test_results"]
    rows = (r for _i, r in result.iterrows()) if hasattr(result, "iterrows") else result
    if dataset_name not in ("lmo", "ycbv"):
        raise ValueError("Unknown dataset name: %r" % (dataset_name,))
    det = {}
    for r in rows:
        x1, y1, x2, y2 = r["dtoid_bbox"][0]
        det.setdefault((int(r["scene_id"]), int(r["im_id"])), []).append((int(r["obj_id"]), x1, y1, x2, y2, r["dtoid_score"][0]))
    save = os.path.join(str(tmp_root), "tmp-%s" % dataset_name)
    if os.path.isdir(save):
        for fn in os.listdir(save):                       # a stale file of an earlier run would count as detections
            if _FILE.match(fn):
                os.remove(os.path.join(save, fn))
    pipeline.save_det_results(det, save)
    res = runMapEval(os.path.join(str(tmp_root), "gt-%s" % dataset_name), save)
    print("Detection mAP metrics:")
    print("Per-object detection AP", res)
    print("Detection mAP:", res["mAP"])
    print()
    return res["mAP"]


def summary(results):
    """The three figures scripts/online_learning.py:611-613 prints, from the list of result rows (dicts) or a dict of
    columns: {"dtoid_iou_mean", "dtoid_iou_recall" (dtoid_iou > 0.5), "pred_iou_visib_recall" (pred_iou_visib > 0.5)}. Host."""
    col = (lambda k: results[k]) if isinstance(results, dict) else (lambda k: [r[k] for r in results])
    a, b = np.asarray(col("dtoid_iou"), dtype=np.float64), np.asarray(col("pred_iou_visib"), dtype=np.float64)
    if a.size == 0:
        raise ValueError("no results")
    return {"dtoid_iou_mean": float(a.mean()), "dtoid_iou_recall": float((a > 0.5).astype(np.float64).mean()),
            "pred_iou_visib_recall": float((b > 0.5).astype(np.float64).mean())}
