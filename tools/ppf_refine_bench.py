"""Dense pose refinement of PPF hypotheses (csrc/ppf_refine.hip, SPEC.md 6.9) on the asymmetric test scene of
tests/ref_ppf.py: the model build time it adds (refinement sampling and grids), and the per-frame device form (depth +
mask -> poses, one launch chain) with and without DensePoseRefinement at the LM-O defaults (SceneSamplingDist 0.05) and
at the YCB-V parameters (0.03), RefPtRate 0.2 and NumResult 100 either way. Device-event timing of >= 200 calls after a
warm-up; one JSON line per case. Beside it, the numpy restatement tests/ref_ppf_refine.py per refined hypothesis.

    python tools/ppf_refine_bench.py [--calls 200] [--out profiles/r07_ppf_refine_bench.json]
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_ppf as rp  # noqa: E402
import ref_ppf_refine as rr  # noqa: E402
from ossid_code_amd import _build, ppf  # noqa: E402


def _timed(fn, calls):
    for _ in range(10):
        out = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _build.build_lib()
    P, N = rp.object_model()
    depth, K, mask, _T = rp.scene(0)
    rows = []
    ppf.PPFModel(P, normals=N)                                 # warm-up (module load, first launches)
    Pd, Nd = ppf._f32(P, torch.device("cuda", 0)), ppf._f32(N, torch.device("cuda", 0))
    model = ppf.PPFModel(P, normals=N)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        model._refine_surface(Pd, Nd)
    torch.cuda.synchronize()
    rows.append({"metric": "ppf_refine_model_build", "vertices": int(len(P)), "RefineSamplingRel": ppf.REFINE_SAMPLING_REL,
                 "refine_points": model.refine["Mr"], "grid_bytes": int(model.refine["grid"].numel()),
                 "ms": round((time.perf_counter() - t0) * 1e3 / 20, 3)})
    d = torch.from_numpy(depth).cuda()
    m = torch.from_numpy(mask.astype(np.uint8)).cuda()
    for name, ssd in (("lmo", 0.05), ("ycbv", 0.03)):
        base, ms0 = _timed(lambda: model.find_hypotheses(d, m, K, SceneSamplingDist=ssd, RefPtRate=0.2), args.calls)
        out, ms1 = _timed(lambda: model.find_hypotheses(d, m, K, SceneSamplingDist=ssd, RefPtRate=0.2,
                                                        DensePoseRefinement=True), args.calls)
        info, st = ppf.check_info(out[2], ssd), ppf.check_refine(out[3])
        rows.append({"metric": "ppf_find_hypotheses_refined", "params": name, "SceneSamplingDist": ssd, "RefPtRate": 0.2,
                     "results": info[0], "refine_scene_points": st[1], "calls": args.calls,
                     "ms_per_frame_unrefined": round(ms0, 4), "ms_per_frame_refined": round(ms1, 4),
                     "ms_added": round(ms1 - ms0, 4)})
    rm = rr.RefineModel(P, N)
    C = rp.depth2cloud(depth, mask, K)
    poses, _s = rp.find(rp.Model(P, N, 0.03), C)
    _idx, S = rr.scene_points(C, rm.D)
    t0 = time.perf_counter()
    for T in poses[:4]:
        rr.refine_one(T, S, rm)
    rows.append({"metric": "numpy_restatement_refine (tests/ref_ppf_refine.py)", "SceneSamplingDist": 0.05,
                 "threads": int(os.environ["OMP_NUM_THREADS"]), "refine_scene_points": int(len(S)),
                 "ms_per_hypothesis": round((time.perf_counter() - t0) * 1e3 / 4, 1)})
    text = "\n".join(json.dumps(r) for r in rows)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
