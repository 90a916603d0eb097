"""Detection mAP of two folders of per-image text files on the GPU (ossid_code_amd/det_eval.py, SPEC.md section 10): what the
reference's run ends with (utils/detection.py:97-135 hands the same two folders to an external script):

    python3 tools/eval_det_map.py GT_FOLDER DET_FOLDER [--method area|voc11] [--iou 0.5 ...] [--top K]

Files are s%06d_i%06d.txt as pipeline.save_det_results writes them: `name x1 y1 x2 y2` per ground truth, `name score x1 y1
x2 y2` per detection. --method area is the all-point AP (SPEC 10.8, the default; what the external script is understood to
report, parity unpinned), voc11 the 11-point AP of the reference's DetectionMetric (10.7, pinned to it by a recorded
fixture). --top K keeps each (image, object)'s first K detections. Prints, per IoU threshold, `AP% = name AP` per object and
`mAP = AP%`, unrounded.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    from ossid_code_amd import det_eval
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("gt_folder")
    ap.add_argument("det_folder")
    ap.add_argument("--method", choices=("area", "voc11"), default="area")
    ap.add_argument("--iou", type=float, nargs="+", default=[0.5])
    ap.add_argument("--top", type=int, default=None)
    args = ap.parse_args(argv)
    r = det_eval.eval_folders(args.gt_folder, args.det_folder, iou_thresholds=args.iou, top=args.top)
    per, mean = (r["APa"], r["mAPa"]) if args.method == "area" else (r["AP11"], r["mAP11"])
    for k, thr in enumerate(r["iou_thresholds"]):
        if len(args.iou) > 1:
            print("IoU > %g" % float(thr))
        for c, name in enumerate(r["classes"]):
            print("%.6f%% = %s AP" % (100.0 * float(per[k, c]), name))
        print("mAP = %.6f%%" % (100.0 * float(mean[k])))
    return r


if __name__ == "__main__":
    main()
