"""PPF hypotheses throughput (csrc/ppf.hip, SPEC.md section 6) on the asymmetric test scene of tests/ref_ppf.py: model build
time, and the per-frame device form (depth + mask -> poses, one launch chain) at the LM-O defaults (SceneSamplingDist
0.05, RefPtRate 0.2) and at the YCB-V parameters (0.03 / 0.2, model at 0.03 either way). Device-event timing of >= 200
calls after a warm-up; one JSON line per case. Beside it, the numpy restatement tests/ref_ppf.py on the same frame.

    python tools/ppf_bench.py [--calls 200] [--out profiles/r06_ppf_bench.json]
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
from ossid_code_amd import _build, ppf  # noqa: E402


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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model = ppf.PPFModel(P, normals=N)
    torch.cuda.synchronize()
    rows.append({"metric": "ppf_model_build", "vertices": int(len(P)), "ModelSamplingDist": 0.03, "sampled": model.Ms,
                 "entries": int(model.offsets[-1].item()), "ms": round((time.perf_counter() - t0) * 1e3, 3)})
    d = torch.from_numpy(depth).cuda()
    m = torch.from_numpy(mask.astype(np.uint8)).cuda()
    for name, ssd in (("lmo", 0.05), ("ycbv", 0.03)):
        for _ in range(10):
            out = model.find_hypotheses(d, m, K, SceneSamplingDist=ssd, RefPtRate=0.2)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            out = model.find_hypotheses(d, m, K, SceneSamplingDist=ssd, RefPtRate=0.2)
        e1.record()
        torch.cuda.synchronize()
        info = ppf.check_info(out[2], ssd)
        rows.append({"metric": "ppf_find_hypotheses", "params": name, "SceneSamplingDist": ssd, "RefPtRate": 0.2,
                     "pixels_in_mask": int(mask.sum()), "scene_sampled": info[1], "candidates": info[2],
                     "clusters": info[3], "results": info[0], "calls": args.calls,
                     "ms_per_frame": round(e0.elapsed_time(e1) / args.calls, 4)})
    model_ref = rp.Model(P, N, 0.03)
    C = rp.depth2cloud(depth, mask, K)
    for ssd in (0.05, 0.03):
        t0 = time.perf_counter()
        rp.find(model_ref, C, rel=ssd)
        rows.append({"metric": "numpy_restatement_ppf (tests/ref_ppf.py)", "SceneSamplingDist": ssd,
                     "threads": int(os.environ["OMP_NUM_THREADS"]), "ms_per_frame": round((time.perf_counter() - t0) * 1e3, 1)})
    text = "\n".join(json.dumps(r) for r in rows)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
