"""Times the mesh depth renderer (csrc/raster.hip, SPEC.md section 7) -> profiles/render_mesh.json:

  render_depth at level 5 (40 960 triangles) and level 7 (655 360) of the test mesh at ref_ppf.POSES[0], and level 0
  (40 triangles) at the near pose, each at N = 1 and N = 32, with the statistics of the first pose;
  the point-splat stand-in (pipeline.render_depth_points, 2048 points, radius 1) on the same box in the same run;
  the pseudo_label stage of OnlineStream per frame with the splat and with the mesh.

    python3 tools/bench_render.py [--out profiles/render_mesh.json] [--commit ID]
    python3 tools/bench_render.py --color [--out profiles/render_color.json]      render_color against render_depth, see below
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/bench_render.py --trace     (a few untimed calls per workload)

Times are HIP events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows.
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

import ref_ppf as rp      # noqa: E402
import ref_raster as rr   # noqa: E402
from ossid_code_amd import pipeline, render, synth  # noqa: E402

HW = (480, 640)


def event_ms(fn, reps, rounds):
    """Median over `rounds` of the mean milliseconds of `reps` back-to-back calls (device events); also min and max."""
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


def batch_of(T, n):
    poses = np.repeat(np.asarray(T)[None], n, 0).copy()
    for k in range(n):                       # the top-k hypotheses of a frame: the same object, a little apart
        poses[k, :3, 3] += [0.002 * (k % 8), 0.002 * (k // 8), 0.001 * k]
    return poses


def workloads():
    return [("level5_far", 5, rp.gt_pose(0)), ("level7_far", 7, rp.gt_pose(0)), ("level0_near", 0, rr.pose_at((0.03, 0.02, 0.12)))]


def stream_stage_ms(meshes, n_warm=2, n_timed=8):
    """times["pseudo_label"] of OnlineStream per frame (host clock around synchronised work, as the stream reports it)."""
    from ossid_code_amd import dtoid, zephyr
    from ossid_code_amd.stream import OnlineStream

    class _Args:
        dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0

    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", _Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, _Args(), num_class=1), 0).to(0).eval()
    g = torch.Generator().manual_seed(1)
    limg = torch.rand(3, 3, 124, 124, generator=g)
    lmask = (torch.rand(3, 1, 124, 124, generator=g) > 0.5).float()
    frames = []
    for f in range(n_warm + n_timed):
        d = synth.make_scoring_inputs(64, 2048, seed=200 + f)
        d.update(limg=limg, lmask=lmask, obj_id=1, pose_gt=d["pose_hypos"][0].copy())
        frames.append(d)
    stream = OnlineStream(det, scorer, ds, confident_threshold=1e30, meshes=meshes)
    for fr in frames[:n_warm]:
        stream.process(fr)
    stream.times = {k: 0.0 for k in stream.times}
    for fr in frames[n_warm:]:
        stream.process(fr)
    return {k: 1e3 * v / n_timed for k, v in stream.times.items()}


def per_call_ms(fn, warm=3, calls=20):
    """Median, min and max of `calls` single calls, each between its own pair of device events, after `warm` untimed ones."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms": float(np.median(out)), "ms_min": float(min(out)), "ms_max": float(max(out)), "calls": calls, "warm": warm}


def color_against_depth(trace):
    """render_color against render_depth (the depth-only entry) on the same call (SPEC 7.11-7.12): level 5 and level 7 of
    the coloured test mesh, 32 poses at 640 x 480 and the 162 template views at 496 x 496. The depth-only entry has one
    camera per call, so for the template views both sides use the first view's virtual camera. Also the wall time of
    render_templates for the 162-view grid (host clock around synchronised work)."""
    import time

    import ref_raster_color as rc
    K = synth.CAM_K
    res = {}
    for level in (5, 7):
        V, F = rr.bump_mesh(level)
        mesh = render.Mesh(V, F, colors=rc.axis_colors(V)[0])
        R = render.view_grid(2)
        cams, _tz = render._frame_views(mesh.vertices, R, 0.8, K, 496, 124, 1.1, 0.05)
        Kv = rc.cam_matrix(*[float(np.float32(x)) for x in cams[0]])
        views = np.tile(np.eye(4), (len(R), 1, 1))
        views[:, :3, :3], views[:, 2, 3] = R, 0.8
        for name, poses, cam, hw in (("frames_32x640x480", batch_of(rp.gt_pose(0), 32), K, HW), ("views_162x496x496", views, Kv, (496, 496))):
            T = torch.from_numpy(poses).to("cuda", torch.float32)
            depth_fn = lambda: render.render_depth(mesh, T, cam, hw)  # noqa: E731
            color_fn = lambda: render.render_color(mesh, T, cam, hw)  # noqa: E731
            if trace:
                for _ in range(3):
                    depth_fn(), color_fn()
                torch.cuda.synchronize()
                continue
            assert torch.equal(depth_fn(), color_fn()[1])
            row = {"depth": per_call_ms(depth_fn), "color": per_call_ms(color_fn), "triangles": mesh.n_faces, "poses": len(poses),
                   "frame": list(hw)}
            row["ratio"] = row["color"]["ms"] / row["depth"]["ms"]
            res["level%d_%s" % (level, name)] = row
            print("level", level, name, row, flush=True)
        if not trace:
            walls = []
            for _ in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                render.render_templates(mesh, cam_K=K)
                torch.cuda.synchronize()
                walls.append(1e3 * (time.perf_counter() - t0))
            res["level%d_render_templates_162_wall_ms" % level] = {"first": walls[0], "median_of_next_3": float(np.median(walls[1:]))}
            print("level", level, "render_templates", walls, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="profiles/render_mesh.json, or profiles/render_color.json with --color")
    ap.add_argument("--color", action="store_true", help="time render_color against render_depth and render_templates")
    ap.add_argument("--commit", default=None)
    ap.add_argument("--trace", action="store_true", help="a few untimed calls per workload, for a kernel trace")
    ap.add_argument("--no-stream", action="store_true", help="skip the OnlineStream stage timing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs the GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    args.out = args.out or os.path.join(ROOT, "profiles", "render_color.json" if args.color else "render_mesh.json")
    if args.color:
        res = {"render_color_against_render_depth": color_against_depth(args.trace)}
        if not args.trace:
            write(res, args)
        return
    K = synth.CAM_K
    res = {"render_depth": {}, "frame": list(HW)}
    for name, level, T in workloads():
        mesh = render.Mesh(*rr.bump_mesh(level))
        for n in (1, 32):
            poses = torch.from_numpy(batch_of(T, n) if n > 1 else np.asarray(T)).cuda()
            fn = lambda: render.render_depth(mesh, poses, K, HW)  # noqa: E731
            if args.trace:
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                continue
            _d, st = render.render_depth(mesh, poses, K, HW, return_stats=True)
            row = event_ms(fn, reps=50 if n == 1 else 10, rounds=7)
            row.update(triangles=mesh.n_faces, vertices=mesh.n_vertices, poses=n, pixels_covered=int((_d.reshape(-1, *HW)[0] > 0).sum()),
                       stats_pose0=st.reshape(-1, 4)[0].tolist(), us_per_pose=1e3 * row["ms"] / n)
            res["render_depth"]["%s_N%d" % (name, n)] = row
            print(name, n, row, flush=True)
    pts = synth.make_scoring_inputs(8, 2048, seed=5)["model_points"]
    splat = lambda: pipeline.render_depth_points(rp.gt_pose(0), pts, K, HW, radius=1)  # noqa: E731
    if args.trace:
        for _ in range(5):
            splat()
        torch.cuda.synchronize()
        return
    res["render_depth_points_2048_r1"] = event_ms(splat, reps=50, rounds=7)
    print("splat", res["render_depth_points_2048_r1"], flush=True)
    if not args.no_stream:
        res["pseudo_label_stage_ms_per_frame"] = {
            "splat": stream_stage_ms(None)["pseudo_label"],
            "mesh_level5": stream_stage_ms({1: render.Mesh(*rr.bump_mesh(5))})["pseudo_label"],
            "mesh_level7": stream_stage_ms({1: render.Mesh(*rr.bump_mesh(7))})["pseudo_label"]}
        print("pseudo_label", res["pseudo_label_stage_ms_per_frame"], flush=True)
    write(res, args)


def write(res, args):
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    res.update(commit=commit, box={"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__,
                                   "hip": torch.version.hip})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
