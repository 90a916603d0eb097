"""Times distinct-pose selection (csrc/pose_select.hip, SPEC.md section 16) -> one JSON line and profiles/pose_select.json:

  ossid_pose_select at N = 1000 scored hypotheses and M = 2048 model points, for K in {1, 4, 16} picks and S in {1, 315}
  symmetry transforms (315: one continuous symmetry at 8.6's default step). The hypotheses are 16 clouds of perturbations
  (synth.perturb_pose: N(0, 0.2) rad, N(0, 0.01) m per axis) around 16 poses 0.15 m apart, of an ellipsoid of diameter
  0.1 m, sep = 0.2 x the diameter as OnlineStream's default has it -- so every one of the K rounds picks;
  beside it, in the same run, the scoring of one 1000 x 2048 frame (scoring.networkInference on synth's frame with the
  random-weight scorer), so that the selection's share of a frame can be read off: `share_of_scoring` = select / score.

    python3 tools/bench_pose_select.py [--out profiles/pose_select.json] [--commit ID]
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/bench_pose_select.py --trace

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows; the windows
of the shapes alternate round by round. Device-resident inputs: the times are the 1 + 2 K launches, no upload.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_pose_select as rp   # noqa: E402
from ossid_code_amd import _lib, bop_eval, scoring, synth, zephyr  # noqa: E402

N, M, CLOUDS, DIAMETER, SEP_REL = 1000, 2048, 16, 0.1, 0.2


def frame_of_clouds(seed=0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(M, 3))
    points = (0.5 * DIAMETER * d / np.linalg.norm(d, axis=1, keepdims=True) * np.array([1.0, 0.8, 0.6])).astype(np.float32)
    poses = []
    for c in range(CLOUDS):
        T = np.eye(4)
        T[:3, :3] = synth._rodrigues(np.array([0.6, 0.0, 0.8]), 0.4 * c)
        T[:3, 3] = [0.15 * (c % 4 - 1.5), 0.15 * (c // 4 - 1.5), 0.8]
        poses.append(synth.perturb_pose(T, (N + CLOUDS - 1) // CLOUDS, seed=seed + c))
    every = np.concatenate(poses)
    return every[rng.permutation(len(every))[:N]], rng.random(N).astype(np.float32), points


def alternating_ms(fns, reps, rounds):
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / reps)
    return {k: {"ms": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "reps": reps, "rounds": rounds}
            for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_select.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--trace", action="store_true", help="a few untimed calls per shape, for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_select.py needs the GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    poses, scores, points = frame_of_clouds()
    lathe = {"symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [0.0, 0.0, 0.0]}]}
    syms = {1: bop_eval.symmetry_transformations({}), 315: bop_eval.symmetry_transformations(lathe)}
    T, sc, P = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (poses, scores, points))
    Sd = {S: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for S, v in syms.items()}
    sep = SEP_REL * DIAMETER
    out = torch.empty(64 + 1 + N, dtype=torch.int32, device=dev)
    keys = torch.empty(64, dtype=torch.int64, device=dev)
    fn = _lib.fn("ossid_pose_select")

    def call(K, S):
        def run():
            rc = fn(T.data_ptr(), sc.data_ptr(), N, P.data_ptr(), M, Sd[S].data_ptr(), S, K, sep, float("-inf"), out.data_ptr(),
                    out.data_ptr() + 256, out.data_ptr() + 260, keys.data_ptr(), _lib.stream())
            assert rc == 0, rc
        return run
    shapes = [(K, S) for S in (1, 315) for K in (1, 4, 16)]
    if args.trace:
        for K, S in shapes:
            for _ in range(3):
                call(K, S)()
        torch.cuda.synchronize()
        return
    res = {"metric": "distinct-pose selection, ms per frame", "N": N, "M": M, "clouds": CLOUDS, "sep": sep, "select": {}}
    # what the shapes select, and S = 1 against the restatement
    for K, S in shapes:
        call(K, S)()
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        res["select"]["K%d_S%d" % (K, S)] = {"picks": int(o[64]), "owned": int((o[65:] >= 0).sum())}
        if S == 1:
            want = rp.select(poses, scores, points, K, sep)
            assert np.array_equal(o[:K], want[0]) and o[64] == want[1][0] and np.array_equal(o[65:], want[2]), (K, S)
    times = alternating_ms({"K%d_S%d" % ks: call(*ks) for ks in shapes}, reps=10, rounds=7)
    for k, v in times.items():
        res["select"][k].update(v)

    class Args:
        dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0
    dataset = zephyr.ScoreDataset([], "", "lmo", Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(dataset.dim_point, Args(), num_class=1), 0).to(0).eval()
    data = synth.make_scoring_inputs(N, M, seed=42)
    res["score_1000x2048"] = alternating_ms({"score": lambda: scoring.networkInference(scorer, dataset, data)}, reps=3, rounds=7)["score"]
    for k in times:
        res["select"][k]["share_of_scoring"] = res["select"][k]["ms"] / res["score_1000x2048"]["ms"]
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    res.update(commit=commit, box={"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
