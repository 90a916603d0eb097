"""ICP refinement throughput (csrc/icp.hip, SPEC.md section 5): M = 2048 on the asymmetric test scene of tests/ref_icp.py,
K = 1 (the caller's case) and K = 1000 (top-k hypotheses in one launch), plus K = 1 with max_iter = 0 (staging and one
correspondence pass: the rest of a K = 1 call is its updates). Device-event timing of >= 200 calls after a warm-up; one
JSON line per case. Beside it, the numpy restatement tests/ref_icp.py (brute force, 16 threads) on one pose:
a restatement of the same algorithm, not open3d.

    python tools/icp_bench.py [--calls 200] [--out profiles/r05_icp_bench.json]
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

import ref_icp as ri  # noqa: E402
from ossid_code_amd import _build, pipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _build.build_lib()
    depth, K, T_gt, P = ri.scene()
    rows = []
    for n_pose, max_iter in ((1, 0), (1, 30), (1000, 30)):
        rng = np.random.default_rng(5)                      # the K = 1 cases refine the same pose
        poses = np.stack([ri.perturb(T_gt, rng.normal(size=3), rng.uniform(2, 3), rng.normal(0, 0.0025, 3))
                          for _ in range(n_pose)])
        uv = torch.from_numpy(np.stack([ri.project_uv(T, P, K) for T in poses])).cuda()
        d = torch.from_numpy(depth).cuda()
        Tt = torch.from_numpy(poses).cuda()
        Pt = torch.from_numpy(P.astype(np.float32)).cuda()
        for _ in range(10):
            out = pipeline.icp_refine(d, uv, Tt, K, Pt, max_iter=max_iter)
        torch.cuda.synchronize()
        calls = args.calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = pipeline.icp_refine(d, uv, Tt, K, Pt, max_iter=max_iter)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / calls
        its = out[3].cpu().numpy()
        rows.append({"metric": "icp_refine", "M": int(len(P)), "K": n_pose, "max_iter": max_iter, "calls": calls, "ms_per_call": round(ms, 4),
                     "poses_per_s": round(n_pose * 1000.0 / ms, 1), "iterations_mean": float(its.mean()),
                     "iterations_max": int(its.max()), "kernel_launches_per_call": 1,
                     "fitness_mean": float(out[1].cpu().numpy().mean())})
    t0 = time.perf_counter()
    n_ref = 3
    for k in range(n_ref):
        ri.icp(depth, ri.project_uv(ri.perturb(T_gt, [1, 0, 0], 2.5, [0.003, 0, 0]), P, K),
               ri.perturb(T_gt, [1, 0, 0], 2.5, [0.003, 0, 0]), K, P)
    ref_ms = (time.perf_counter() - t0) * 1000.0 / n_ref
    rows.append({"metric": "numpy_restatement_icp (tests/ref_icp.py, brute force, not open3d)", "M": int(len(P)), "K": 1,
                 "threads": int(os.environ["OMP_NUM_THREADS"]), "ms_per_pose": round(ref_ms, 2)})
    text = "\n".join(json.dumps(r) for r in rows)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.join(ROOT, args.out)), exist_ok=True)
        with open(os.path.join(ROOT, args.out), "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
