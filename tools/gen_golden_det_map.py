"""Writes tests/golden/det_map.npz: seeded detection sets with the per-class APs and the mAP that the REFERENCE class
DetectionMetric.calculate_mAP (utils/detection_metrics.py, loaded from the reference tree at generation time, on the CPU)
gives for them. Only the recorded inputs and results are committed; no reference source is copied. The fixture pins
ossid_code_amd/det_eval.py and tests/ref_det_eval.py (SPEC.md section 10) to the reference's own numbers. Run from the repo
root, in the build container:
    python tools/gen_golden_det_map.py

The generator refuses to write a fixture on which the comparison would rest on an unspecified choice of the reference
(torch.sort among equal scores, torch.max among equal IoUs) or would say little (APs at 0 or 1)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ref_import import REF  # noqa: E402
import ref_det_eval as rde  # noqa: E402

W, H = 640.0, 480.0


def reference_module():
    spec = importlib.util.spec_from_file_location("ref_detection_metrics", os.path.join(REF, "ossid", "utils", "detection_metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(seed, n_images=40, n_classes=3, per_image=6, sigma=15.0, p_difficult=0.0, p_relabel=0.2, one_per_object=False,
              silent_class=False, empty_images=0):
    """Ground truths: 0-3 per image (none in the first `empty_images`), random class and box. Detections: jittered copies of
    ground truths of their image (random boxes where it has none), 20 % relabelled at random; with one_per_object exactly one
    per ground truth. silent_class: no detection carries the last class."""
    rng = np.random.RandomState(seed)
    gb, gc, gi, db, dc, di = [], [], [], [], [], []
    for i in range(n_images):
        boxes = []
        for _ in range(0 if i < empty_images else rng.randint(0, 4)):
            w, h = rng.uniform(40, 160), rng.uniform(40, 160)
            x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
            boxes.append(((x, y, x + w, y + h), rng.randint(0, n_classes)))
        for b, c in boxes:
            gb.append(b), gc.append(c), gi.append(i)
        picks = list(range(len(boxes))) if one_per_object else [rng.randint(0, len(boxes)) if boxes else -1 for _ in range(per_image)]
        for p in picks:
            if p >= 0:
                b, c = np.asarray(boxes[p][0]) + rng.normal(0.0, sigma, 4), boxes[p][1]
            else:
                w, h = rng.uniform(40, 160), rng.uniform(40, 160)
                x, y = rng.uniform(0, W - w), rng.uniform(0, H - h)
                b, c = np.array([x, y, x + w, y + h]), rng.randint(0, n_classes)
            if rng.uniform() < p_relabel:
                c = rng.randint(0, n_classes)
            if silent_class and c == n_classes - 1:
                c = rng.randint(0, n_classes - 1)
            b = np.array([min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])])
            db.append(b), dc.append(c), di.append(i)
    N, G = len(dc), len(gc)
    score = (rng.permutation(N).astype(np.float64) + 0.5) / N            # pairwise distinct, also as f32: check_case asserts it
    return {"det_box": np.asarray(db, np.float32).reshape(N, 4), "det_score": score.astype(np.float32),
            "det_cls": np.asarray(dc, np.int32), "det_image": np.asarray(di, np.int32),
            "gt_box": np.asarray(gb, np.float32).reshape(G, 4), "gt_cls": np.asarray(gc, np.int32), "gt_image": np.asarray(gi, np.int32),
            "gt_difficult": (rng.uniform(size=G) < p_difficult).astype(np.uint8), "n_images": n_images, "n_classes": n_classes}


def run_reference(mod, case):
    I, C = case["n_images"], case["n_classes"]
    metric = mod.DetectionMetric(["c%d" % c for c in range(C)], device=torch.device("cpu"))
    sel = lambda a, idx, i: torch.from_numpy(a[idx == i])
    args = [[sel(case["det_box"], case["det_image"], i) for i in range(I)],
            [sel(case["det_cls"].astype(np.int64) + 1, case["det_image"], i) for i in range(I)],
            [sel(case["det_score"], case["det_image"], i) for i in range(I)],
            [sel(case["gt_box"], case["gt_image"], i) for i in range(I)],
            [sel(case["gt_cls"].astype(np.int64) + 1, case["gt_image"], i) for i in range(I)],
            [sel(case["gt_difficult"].astype(np.int64), case["gt_image"], i) for i in range(I)]]
    aps, mean = metric.calculate_mAP(*args)
    return np.array([aps["c%d" % c] for c in range(C)], np.float64), float(mean)


def check_case(name, case, ap):
    assert len(np.unique(case["det_score"])) == len(case["det_score"]), "%s: equal scores" % name
    off = np.concatenate([[0], np.cumsum(np.bincount(case["gt_image"], minlength=case["n_images"]))])
    for n in range(len(case["det_cls"])):
        g = [k for k in range(off[case["det_image"][n]], off[case["det_image"][n] + 1]) if case["gt_cls"][k] == case["det_cls"][n]]
        v = rde.iou(case["det_box"][n], case["gt_box"][g]) if g else np.zeros(0)
        nz = v[v != 0]                                          # candidates that do not overlap at all tie at 0 and are misses either way
        assert len(np.unique(nz)) == len(nz), "%s: detection %d has two candidates of equal IoU" % (name, n)
        assert not np.isnan(v).any(), "%s: NaN IoU" % name
    inside = int(((ap > 0.05) & (ap < 0.95)).sum())
    assert inside >= 2, "%s: only %d classes with 0.05 < AP < 0.95: %s" % (name, inside, ap)


def main():
    mod = reference_module()
    thr = torch.arange(start=0, end=1.1, step=.1)
    assert thr.numpy().tolist() == rde.REC_THR.tolist(), "recall thresholds differ from torch.arange(0, 1.1, .1)"
    cases = {"a": make_case(101), "b": make_case(102, p_difficult=0.3), "c": make_case(103, sigma=8.0, p_difficult=0.3),
             "d": make_case(104, sigma=25.0), "e": make_case(105, one_per_object=True, sigma=20.0, p_relabel=0.3),
             "f": make_case(106, n_classes=4, silent_class=True, empty_images=6)}
    out = {"rec_thr": rde.REC_THR}
    for name, case in cases.items():
        ap, mean = run_reference(mod, case)
        check_case(name, case, ap)
        if name == "f":
            assert not (case["det_cls"] == 3).any() and (case["gt_cls"] == 3).any() and ap[3] == 0.0
        print(name, "N", len(case["det_cls"]), "G", len(case["gt_cls"]), "AP", ap, "mAP", mean)
        for k, v in case.items():
            out["%s_%s" % (name, k)] = v
        out["%s_ap" % name], out["%s_map" % name] = ap, mean
    path = os.path.join(ROOT, "tests", "golden", "det_map.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
