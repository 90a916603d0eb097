"""BOP-19 evaluation of a results csv on the GPU (ossid_code_amd/bop_eval.py, SPEC.md section 8), under the command line the
reference issues (utils/bop_utils.py:51-53):

    cd BOP_TOOLKIT_PATH; python scripts/eval_bop19.py --renderer_type=cpp --result_filenames=NAME.csv

    python3 tools/eval_bop19.py --result_filenames=method_lmo-test.csv[,more.csv] --datasets_path=/data/bop
                                [--results_path=DIR] [--targets_filename=test_targets_bop19.json] [--renderer_type=ANY]
                                [--multi_instance [--visib_gt_min=0.1]]

--multi_instance (off by default: then every target must have one instance, as before) scores targets with inst_count > 1,
e.g. a folder tools/make_scenes.py wrote with more objects per scene than models: the inst_count best-scored rows of a
target against all its instances, matched greedily per threshold (SPEC 8.10-8.12). Not BOP-19 even then: no per-object
averaging variants, no time limits.

A file is `<method>_<dataset>-<split>.csv` as pipeline.save_results_bop writes it (looked up under --results_path unless
the path exists as given). --renderer_type is accepted and ignored: there is one renderer, the device rasteriser. Prints
AR_VSD, AR_MSSD, AR_MSPD and AR per file and writes `<result>_scores.json` beside the csv. The reference passes neither
folder: as with bop_toolkit (whose config reads the same variables) --datasets_path defaults to the environment variable
BOP_PATH and --results_path to BOP_RESULTS_PATH -- the folder saveResultsBop wrote into, ossid.config.BOP_RESULTS_FOLDER --
and only then to the working directory. The script may be reached through a symbolic link (BOP_TOOLKIT_PATH/scripts/
eval_bop19.py -> this file): the package is found beside the link's target, whatever PYTHONPATH says. The definitions are
this build's own; parity with bop_toolkit is unpinned (SPEC 8).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.realpath(__file__)))       # through a link: the repository, not the link's folder
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_result_name(path):
    """`<method>_<dataset>-<split>.csv` -> (method, dataset, split)."""
    base = os.path.basename(path)
    if not base.endswith(".csv") or "_" not in base or "-" not in base.rsplit("_", 1)[1]:
        raise ValueError("%s: a results file is named <method>_<dataset>-<split>.csv" % base)
    method, rest = base[:-4].rsplit("_", 1)
    dataset, split = rest.split("-", 1)
    return method, dataset, split


def main(argv=None):
    from ossid_code_amd import bop_eval
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--result_filenames", required=True, help="comma-separated csv files")
    ap.add_argument("--datasets_path", default=os.environ.get("BOP_PATH"), help="folder that holds lmo/, ycbv/, ...")
    ap.add_argument("--results_path", default=os.environ.get("BOP_RESULTS_PATH") or ".", help="where the csv files are looked up")
    ap.add_argument("--targets_filename", default="test_targets_bop19.json")
    ap.add_argument("--renderer_type", default=None, help="accepted and ignored")
    ap.add_argument("--multi_instance", action="store_true",
                    help="targets may have inst_count > 1: pair errors and BOP's greedy matching (SPEC 8.10-8.12)")
    ap.add_argument("--visib_gt_min", type=float, default=0.1,
                    help="with --multi_instance: an instance counts iff its visib_fract is at least this")
    args, unknown = ap.parse_known_args(argv)
    if unknown:
        print("eval_bop19: ignoring %s" % " ".join(unknown), file=sys.stderr)
    if not args.datasets_path:
        ap.error("--datasets_path (or the environment variable BOP_PATH) is required")
    out = {}
    for name in [n for n in args.result_filenames.split(",") if n]:
        path = name if os.path.exists(name) else os.path.join(args.results_path, name)
        if not os.path.exists(path):
            raise SystemExit("eval_bop19: %s is neither a file nor in %s (--results_path, or the environment variable "
                             "BOP_RESULTS_PATH)" % (name, os.path.abspath(args.results_path)))
        method, dataset_name, split = parse_result_name(path)
        dataset = bop_eval.BopFolder(args.datasets_path, dataset_name, split, targets_filename=args.targets_filename)
        if args.multi_instance:
            scores = bop_eval.evaluate(bop_eval.read_results_csv(path), dataset, multi_instance=True,
                                       visib_gt_min=args.visib_gt_min)
        else:
            scores = bop_eval.evaluate(bop_eval.read_results_csv(path), dataset)
        keep = {k: v for k, v in scores.items() if k not in ("rows", "match")}
        keep.update(method=method, dataset=dataset_name, split=split)
        tail = "(%d estimates kept for %d targets)" if args.multi_instance else "(%d of %d targets have an estimate)"
        print(("%s: AR_VSD %.6f  AR_MSSD %.6f  AR_MSPD %.6f  AR %.6f  " + tail)
              % (os.path.basename(path), keep["AR_VSD"], keep["AR_MSSD"], keep["AR_MSPD"], keep["AR"], keep["estimates"],
                 keep["targets"]))
        with open(path[:-4] + "_scores.json", "w") as f:
            json.dump(keep, f, indent=1)
        out[path] = keep
    return out


if __name__ == "__main__":
    main()
