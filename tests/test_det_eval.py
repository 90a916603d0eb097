"""Host checks of the detection mAP (SPEC.md section 10): the restatement tests/ref_det_eval.py against the recorded numbers of
the reference class (tests/golden/det_map.npz, written by tools/gen_golden_det_map.py), its two forms of the status rule
against each other, and the host side of ossid_code_amd/det_eval.py: text files, refusals, summary, compat."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_det_eval as rde
from ossid_code_amd import det_eval, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = "abcdef"
# |AP11 - ref| <= 2e-6: ten additions of partial sums below 16, each rounding <= 2^-21, then a division by 11, on each side
# (< 4.4e-7 per side). mAP11 within 3e-6: C <= 8, seven additions below 8, each <= 2^-22, divided by C, on top of that.
AP_TOL, MAP_TOL = 2e-6, 3e-6


def load_case(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "det_map.npz"))
    c = {k[2:]: z[k] for k in z.files if k.startswith(name + "_")}
    c["n_images"], c["n_classes"] = int(c["n_images"]), int(c["n_classes"])
    c["gt_offset"] = np.concatenate([[0], np.cumsum(np.bincount(c["gt_image"], minlength=c["n_images"]))]).astype(np.int32)
    return c


def ref_eval(c, iou_thr=(0.5,), sequential=False):
    return rde.evaluate(c["det_box"], c["det_score"], c["det_cls"], c["det_image"], c["gt_box"], c["gt_cls"], c["gt_offset"],
                        c["gt_difficult"], c["n_classes"], iou_thr, sequential=sequential)


def tied_case():
    """Tied scores, duplicate detections, two identical ground truths, a difficult one, the exact-0.5 pair and zero-area boxes."""
    gt_box = np.array([[10, 10, 50, 50], [10, 10, 50, 50], [100, 100, 160, 140], [0, 0, 1, 1], [5, 5, 5, 5], [200, 200, 240, 260]], np.float32)
    gt_cls = np.array([0, 0, 1, 0, 1, 0], np.int32)
    gt_image = np.array([0, 0, 0, 1, 1, 2], np.int32)
    difficult = np.array([0, 0, 0, 0, 0, 1], np.uint8)
    det_box = np.array([[10, 10, 50, 50], [10, 10, 50, 50], [10, 10, 50, 50], [12, 11, 50, 52], [100, 100, 160, 140], [101, 100, 160, 140],
                        [0, 0, 2, 1], [5, 5, 5, 5], [200, 200, 240, 260], [200, 200, 240, 258], [300, 300, 340, 340]], np.float32)
    det_cls = np.array([0, 0, 0, 0, 1, 1, 0, 1, 0, 0, 1], np.int32)
    det_image = np.array([0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2], np.int32)
    det_score = np.array([0.5, 0.5, 0.5, 0.4, 0.25, 0.25, 0.75, 0.75, 0.0, -0.0, 0.125], np.float32)
    return {"det_box": det_box, "det_score": det_score, "det_cls": det_cls, "det_image": det_image, "gt_box": gt_box, "gt_cls": gt_cls,
            "gt_image": gt_image, "gt_difficult": difficult, "n_images": 3, "n_classes": 2,
            "gt_offset": np.array([0, 3, 5, 6], np.int32)}


@pytest.mark.parametrize("name", CASES)
def test_restatement_gives_the_reference_class_aps(name):
    c = load_case(name)
    r = ref_eval(c)
    err = np.abs(r["ap11"][0].astype(np.float64) - c["ap"])
    print(name, "AP11", r["ap11"][0], "ref", c["ap"], "max |d|", err.max(), "mAP d", abs(float(r["map11"][0]) - float(c["map"])))
    assert (err <= AP_TOL).all()
    assert abs(float(r["map11"][0]) - float(c["map"])) <= MAP_TOL


def test_recall_thresholds_are_the_recorded_table():
    z = np.load(os.path.join(ROOT, "tests", "golden", "det_map.npz"))
    assert z["rec_thr"].tobytes() == rde.REC_THR.tobytes() == np.asarray(det_eval.REC_THR, np.float32).tobytes()


@pytest.mark.parametrize("name", CASES + "t")
def test_sequential_loop_equals_claim_winner_form(name):
    c = tied_case() if name == "t" else load_case(name)
    thr = (0.3, 0.5, 0.75)
    a, b = ref_eval(c, thr), ref_eval(c, thr, sequential=True)
    assert np.array_equal(a["status"], b["status"])
    assert a["ap11"].tobytes() == b["ap11"].tobytes() and a["apa"].tobytes() == b["apa"].tobytes()
    if name == "t":
        st = a["status"][1]
        assert list(st[:4]) == [rde.ST_TP, rde.ST_DUP, rde.ST_DUP, rde.ST_DUP]      # equal boxes: the score decides; ties by input index
        assert int(a["best_gt"][0]) == 0                                             # two identical ground truths: the lowest g
        assert list(st[4:6]) == [rde.ST_TP, rde.ST_DUP]
        assert float(a["best_iou"][6]) == 0.5 and st[6] == rde.ST_FP                 # exactly 0.5 is not > 0.5
        assert int(a["best_gt"][7]) == -1 and float(a["best_iou"][7]) == 0.0         # NaN never beats a number
        assert list(st[8:10]) == [rde.ST_IGNORED, rde.ST_IGNORED]
        assert list(a["order"]) == [6, 0, 1, 2, 3, 8, 9, 7, 4, 5, 10]              # class, score descending, input index; -0 = +0


def test_rank_ties_by_input_index_and_signed_zero():
    order, off = rde.rank_order(np.array([0.0, -0.0, 0.5, 0.5, -1.0], np.float32), np.array([0, 0, 0, 0, 0]), 1)
    assert list(order) == [2, 3, 0, 1, 4] and list(off) == [0, 5]


def test_read_det_folder_round_trips_save_det_results(tmp_path):
    gt = {(2, 13): [(5, 10, 20, 110, 220), (8, 1, 2, 3, 4)], (1, 7): [(5, 0, 0, 64, 48)], (2, 2): []}
    det = {(2, 13): [(5, 11, 19, 111, 223, 0.5), (5, 300, 20, 400, 220, 0.25)], (1, 7): [(8, 0, 0, 64, 48, 0.125)]}
    pipeline.save_det_results(gt, str(tmp_path / "gt"))
    pipeline.save_det_results(det, str(tmp_path / "det"))
    g, d = det_eval.read_det_folder(str(tmp_path / "gt")), det_eval.read_det_folder(str(tmp_path / "det"))
    assert list(g) == [(1, 7), (2, 2), (2, 13)] and list(d) == [(1, 7), (2, 13)]           # sorted file names
    for back, src in ((g, gt), (d, det)):
        for key, rows in src.items():
            assert back[key] == [("obj_%06d" % r[0],) + tuple(float(v) for v in r[1:]) for r in rows]
    (tmp_path / "det" / "s000009_i000001.txt").write_text("obj_000001 1 2 3\n")
    with pytest.raises(ValueError):
        det_eval.read_det_folder(str(tmp_path / "det"))


def _good():
    det = {"boxes": np.array([[0, 0, 2, 2], [1, 1, 3, 3]], np.float32), "scores": np.array([0.5, 0.25], np.float32),
           "classes": np.array([0, 1]), "images": np.array([0, 1])}
    gt = {"boxes": np.array([[0, 0, 2, 2], [1, 1, 3, 3]], np.float32), "classes": np.array([0, 1]), "images": np.array([0, 1])}
    return det, gt


@pytest.mark.parametrize("what", ["nan_box", "inf_score", "inf_gt", "det_class", "det_class_neg", "det_image", "gt_class", "gt_image",
                                  "ungrouped", "T0", "T17", "thr_nan", "C0", "C4097", "top0"])
def test_refusals_raise_before_the_device_is_touched(what, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device path was reached")
    monkeypatch.setattr(det_eval, "match", no_device)
    monkeypatch.setattr(det_eval._lib, "fn", no_device)
    det, gt = _good()
    classes, kw = ["a", "b"], {}
    if what == "nan_box":
        det["boxes"][1, 2] = np.nan
    elif what == "inf_score":
        det["scores"][0] = np.inf
    elif what == "inf_gt":
        gt["boxes"][0, 0] = -np.inf
    elif what == "det_class":
        det["classes"][1] = 2
    elif what == "det_class_neg":
        det["classes"][0] = -1
    elif what == "det_image":
        det["images"][1], kw["n_images"] = 2, 2
    elif what == "gt_class":
        gt["classes"][0] = 5
    elif what == "gt_image":
        gt["images"][1], kw["n_images"] = 7, 2
    elif what == "ungrouped":
        gt["images"] = np.array([1, 0])
    elif what == "T0":
        kw["iou_thresholds"] = ()
    elif what == "T17":
        kw["iou_thresholds"] = tuple(0.05 * k for k in range(17))
    elif what == "thr_nan":
        kw["iou_thresholds"] = (0.5, float("nan"))
    elif what == "C0":
        classes = []
    elif what == "C4097":
        classes = ["c%d" % k for k in range(4097)]
    elif what == "top0":
        kw["top"] = 0
    with pytest.raises(ValueError):
        det_eval.evaluate(det, gt, classes, **kw)


def test_top_filter_keeps_the_first_k_of_each_image_and_class():
    cls = np.array([0, 0, 1, 0, 1, 0, 0])
    img = np.array([0, 0, 0, 1, 0, 0, 1])
    assert list(det_eval._top_filter(cls, img, 2, 1)) == [True, False, True, True, False, False, False]
    assert list(det_eval._top_filter(cls, img, 2, 2)) == [True, True, True, True, True, False, True]


def test_summary_on_a_made_up_result_list():
    rows = [{"dtoid_iou": 0.8, "pred_iou_visib": 0.9}, {"dtoid_iou": 0.5, "pred_iou_visib": 0.2},
            {"dtoid_iou": 0.2, "pred_iou_visib": 0.6}, {"dtoid_iou": 0.7, "pred_iou_visib": 0.51}]
    s = det_eval.summary(rows)
    assert s == {"dtoid_iou_mean": float(np.mean([0.8, 0.5, 0.2, 0.7])), "dtoid_iou_recall": 0.5, "pred_iou_visib_recall": 0.75}
    assert det_eval.summary({"dtoid_iou": [0.8, 0.5, 0.2, 0.7], "pred_iou_visib": [0.9, 0.2, 0.6, 0.51]}) == s
    with pytest.raises(ValueError):
        det_eval.summary([])


def test_compat_install_det_eval_resolves_the_three_names():
    code = ("import ossid_code_amd.compat as c; c.install(det_eval=True);"
            "from ossid.utils.detection import runMapEval, evalFinetuneResults;"
            "from ossid.utils.detection_metrics import DetectionMetric;"
            "print('ok', runMapEval.__module__, evalFinetuneResults.__module__, DetectionMetric.__module__)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "ok ossid_code_amd.det_eval ossid_code_amd.det_eval ossid_code_amd.det_eval" in out.stdout
    off = ("import sys, ossid_code_amd.compat as c; c.install();"
           "print('off', 'ossid.utils.detection_metrics' in sys.modules)")
    out = subprocess.run([sys.executable, "-c", off], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "off False" in out.stdout, out.stderr


def test_workspace_query_refuses_sizes_outside_the_caps(hiplib):
    q = hiplib.lib().ossid_det_eval_workspace_bytes
    assert q(1000, 10, 3, 1) > 0 and q(0, 0, 1, 16) > 0
    for bad in ((-1, 0, 1, 1), ((1 << 22) + 1, 0, 1, 1), (1, (1 << 20) + 1, 1, 1), (1, 1, 0, 1), (1, 1, 4097, 1), (1, 1, 1, 0), (1, 1, 1, 17)):
        assert q(*bad) == 0, bad
