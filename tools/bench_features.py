"""Times the keypoint-feature pose hypotheses (csrc/features.hip, SPEC.md section 11) -> profiles/features_bench.json:

  one 640 x 480 frame of the level-5 textured test mesh against its 162-view model (view_grid level 2, S = 256), per
  stage: pyramid, detect, describe, match, hypotheses, cluster, and the whole find_hypotheses call;
  the matcher alone at Ns = 4096, Nm = 65536 with random descriptors, and the i8 TOP/s (2 Ns Nm 128 operations) it implies.

    python3 tools/bench_features.py [--out profiles/features_bench.json] [--commit ID]

Times are HIP events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_features as rf  # noqa: E402
import ref_ppf as rp       # noqa: E402
from ossid_code_amd import _lib, features, render, synth  # noqa: E402


def event_ms(fn, reps=20, rounds=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return {"ms": float(np.median(out)), "ms_min": float(min(out)), "ms_max": float(max(out)), "reps": reps, "rounds": rounds}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.json"))
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    V, F, C = rf.textured_mesh(5)
    mesh = render.Mesh(V, F, colors=C)
    K = synth.CAM_K
    model = features.FeatureModel.from_mesh(mesh, K, level=2, view_size=256)
    img, dep = render.render_color(mesh, rp.gt_pose(0), K, (480, 640))
    mask = (dep > 0).to(torch.uint8)
    H, W = 480, 640
    fx, fy, cx, cy = features._intrinsics(K)
    f = features.featurize(img, dep, mask, K)
    n = features.check_count(f)
    st, cap = _lib.stream(), f["cap"]
    pyr, kps, count = f["pyramid"], f["keypoints"], f["count"]
    pb = pyr.numel() * 4
    wb = int(_lib.fn("ossid_feat_detect_workspace_bytes")(H, W, 3))
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    r = model._hypotheses(f["descriptors"], f["frames"], f["ok"], count)
    peaks, cand = r["peaks"], r["cand_poses"]
    poses, scores, info = r["poses"], r["scores"], r["info"]
    stages = {
        "pyramid": lambda: _lib.fn("ossid_feat_pyramid")(img.data_ptr(), H, W, 3, pyr.data_ptr(), pb, st),
        "detect": lambda: _lib.fn("ossid_feat_detect")(pyr.data_ptr(), H, W, 3, dep.data_ptr(), mask.data_ptr(), features.CONTRAST,
                                                       cap, ws.data_ptr(), wb, kps.data_ptr(), count.data_ptr(), st),
        "describe": lambda: _lib.fn("ossid_feat_describe")(pyr.data_ptr(), H, W, 3, dep.data_ptr(), fx, fy, cx, cy, kps.data_ptr(),
                                                           count.data_ptr(), cap, f["bins"].data_ptr(), f["descriptors"].data_ptr(),
                                                           f["frames"].data_ptr(), f["ok"].data_ptr(), st),
        "match": lambda: features.match_descriptors(f["descriptors"], f["ok"], count, model.descriptors),
        "hypotheses": lambda: _lib.fn("ossid_feat_hypotheses")(r["match"].data_ptr(), f["frames"].data_ptr(), count.data_ptr(), cap,
                                                               model.frames.data_ptr(), len(model), peaks.data_ptr(),
                                                               cand.data_ptr(), st),
        "cluster": lambda: _lib.fn("ossid_ppf_cluster")(peaks.data_ptr(), cand.data_ptr(), count.data_ptr(), cap, 1, 1024,
                                                        float(model.D), 0.1, 100, poses.data_ptr(), scores.data_ptr(),
                                                        info.data_ptr(), st),
        "find_hypotheses": lambda: model.find_hypotheses(dep, img, mask, K),
    }
    out = {"commit": args.commit, "device": torch.cuda.get_device_name(0), "frame": [H, W], "keypoints": n,
           "scene_features": int(f["ok"][:n].sum()), "model_features": len(model), "model_views": len(model.view_poses),
           "hypotheses": int(info[0]), "stages": {k: event_ms(fn) for k, fn in stages.items()}}
    rng = np.random.default_rng(0)
    Ns, Nm = _lib.FEAT_MAX_KEYPOINTS, _lib.FEAT_MAX_MODEL_FEATURES
    A = torch.from_numpy(rng.integers(0, 128, (Ns, 128), dtype=np.uint8)).cuda()
    B = torch.from_numpy(rng.integers(0, 128, (Nm, 128), dtype=np.uint8)).cuda()
    ok = torch.ones(Ns, dtype=torch.uint8, device="cuda")
    cnt = torch.tensor([Ns, 0], dtype=torch.int32, device="cuda")
    t = event_ms(lambda: features.match_descriptors(A, ok, cnt, B), reps=10)
    t["tops"] = 2.0 * Ns * Nm * 128 / (t["ms"] * 1e-3) / 1e12
    out["matcher_full"] = {"Ns": Ns, "Nm": Nm, **t}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
