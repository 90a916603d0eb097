"""Times the model cloud from a mesh (csrc/model_cloud.hip, SPEC.md section 9) -> profiles/model_cloud.json:

  sample_model_cloud at all defaults on the level-5 test mesh (40 960 triangles; 162 views at 512 x 512, K = 32 768
  candidates, M = 2048), stage by stage: the views' render, the votes, the weights, the candidates, the thinning, the
  diameter; the whole call, which adds the framing, the host checks and the read-back of Wt;
  the farthest-point sampling alone at K = 32 768 for M = 2048 and M = 4096 and at K = 2048 for M = 2048: the time per round.

    python3 tools/model_cloud_bench.py [--out profiles/model_cloud.json] [--commit ID]
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/model_cloud_bench.py --trace

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_raster as rr            # noqa: E402
import ref_raster_color as rc      # noqa: E402
from ossid_code_amd import model_cloud, render  # noqa: E402


def event_ms(fn, reps, rounds):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_cloud.json"))
    ap.add_argument("--commit", default="")
    ap.add_argument("--trace", action="store_true", help="one pass of every stage and nothing else (for rocprofv3)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("model_cloud_bench.py measures on the GPU: there is no CPU path")
    V, F = rr.bump_mesh(5)
    mesh = render.Mesh(V, F, colors=rc.axis_colors(V)[0])
    cloud, info = model_cloud.sample_model_cloud(mesh, return_info=True)
    torch.cuda.synchronize()
    if a.trace:
        return
    S, per = 512, 32
    R, cams, centres = info["rotations"], info["intrinsics"], info["centres"]
    poses = np.tile(np.eye(4), (len(R), 1, 1))
    poses[:, :3, :3], poses[:, 2, 3] = R, info["distance"]
    chunks = [(lo, min(len(R), lo + per)) for lo in range(0, len(R), per)]
    ids = {}

    def render_all():
        for lo, hi in chunks:
            ids[lo] = render.render_color(mesh, poses[lo:hi], None, (S, S), 0.5, info["z_near"], intrinsics=cams[lo:hi],
                                          return_face_id=True)[2]

    votes = torch.zeros_like(info["votes"])

    def votes_all():
        for lo, hi in chunks:
            model_cloud.face_votes(mesh, ids[lo], centres[lo:hi], votes)

    pts = info["candidates"]["points"]
    small = pts[:2048].contiguous()
    stages = {
        "render_162_views_512": event_ms(render_all, 3, 5),
        "votes_162_views_512": event_ms(votes_all, 3, 5),
        "weights_F40960": event_ms(lambda: model_cloud.face_weights(mesh, info["votes"]), 10, 5),
        "candidates_K32768": event_ms(lambda: model_cloud.face_candidates(mesh, info["votes"], info["prefix"],
                                                                          info["face_normals"], 32768), 10, 5),
        "fps_K32768_M2048": event_ms(lambda: model_cloud.fps(pts, 2048), 5, 5),
        "diameter_V20484": event_ms(lambda: model_cloud.mesh_diameter(mesh), 5, 5),
    }
    t0 = time.perf_counter()
    for _ in range(3):
        model_cloud.sample_model_cloud(mesh)
    torch.cuda.synchronize()
    whole = (time.perf_counter() - t0) / 3.0 * 1e3
    fps = {"K32768_M4096": event_ms(lambda: model_cloud.fps(pts, 4096), 5, 5), "K32768_M2048": stages["fps_K32768_M2048"],
           "K2048_M2048": event_ms(lambda: model_cloud.fps(small, 2048), 5, 5)}
    for key, rounds in (("K32768_M4096", 4095), ("K32768_M2048", 2047), ("K2048_M2048", 2047)):
        fps[key] = dict(fps[key], us_per_round=fps[key]["ms"] * 1e3 / rounds)
    out = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "mesh": {"vertices": len(V), "faces": len(F)},
           "defaults": {"n_points": 2048, "oversample": 16, "level": 2, "view_size": 512, "views_per_call": per},
           "stages_ms": stages, "sample_model_cloud_ms_host_clock": whole, "fps": fps,
           "seen_faces": int((info["votes"].sum(1) > 0).sum()), "diameter": cloud.diameter}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
