"""Times the BOP-19 pose errors (csrc/bop_eval.hip, SPEC.md section 8) -> profiles/bop_eval.json:

  VSD per estimate at 480 x 640 on the level-5 test mesh (40 960 triangles), a batch of N estimates near the scene's true pose,
  split into its three parts: the estimates' render, the ground truths' render, the cost launches (ossid_bop_vsd);
  MSSD / MSPD at N = 1024 on the level-5 vertices (20 484) for S = 1 and S = 315 symmetry transformations;
  beside each the numpy restatement (tests/ref_bop_eval.py) timed in the same run on the box's CPUs -- a baseline for
  orientation, not a target (VSD: the cost pass alone on the device's renders, and one ref_raster render; MSSD / MSPD: a few
  estimates, scaled to N).

  --multi: the multi-instance leg alone -> profiles/bop_eval_multi.json: groups of 4 and of 12 estimates and instances
  through the pair table (n + n renders, ossid_bop_vsd_pairs; SPEC 8.11) against every pair as a row of bop_eval.vsd (2 n n
  renders, ossid_bop_vsd), the two forms' windows alternating round by round: renders, cost launches, the whole Python calls.

    python3 tools/bop_eval_bench.py [--out profiles/bop_eval.json] [--commit ID] [--n 64]
    python3 tools/bop_eval_bench.py --multi [--out profiles/bop_eval_multi.json]
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/bop_eval_bench.py --trace

Times are device events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_bop_eval as rb   # noqa: E402
import ref_icp as ri        # noqa: E402
import ref_raster as rr     # noqa: E402
from ossid_code_amd import _lib, bop_eval, render  # noqa: E402

HW = (480, 640)
DIAMETER = 0.1


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


def estimates(T, n, seed=0):
    """n poses around T: up to 5 degrees and 10 mm off, as a refined hypothesis list is."""
    rng = np.random.default_rng(seed)
    return np.stack([ri.perturb(T, rng.normal(size=3), 5.0 * rng.random(), rng.normal(size=3) * 0.01 * rng.random()) for _ in range(n)])


def vsd_parts(mesh, depth, K, est, gt, trace):
    dev = mesh.device
    N = len(est)
    O = torch.from_numpy(depth[None]).to(dev)
    cams = torch.from_numpy(bop_eval._cameras(K, 1)).to(dev)
    # f32 on the device already: render_depth then adds no cast kernel, the window holds the rasteriser's three launches
    Te, Tg = torch.from_numpy(est).to(dev, torch.float32), torch.from_numpy(gt).to(dev, torch.float32)
    frame, taus = np.zeros(N, dtype=np.int32), np.asarray(bop_eval.VSD_TAUS)
    counts = torch.empty(N, 12, dtype=torch.int32, device=dev)
    errors = torch.empty(N, 10, dtype=torch.float64, device=dev)
    z_est = render.render_depth(mesh, Te, K, HW, pixel_offset=0.0)
    z_gt = render.render_depth(mesh, Tg, K, HW, pixel_offset=0.0)
    fn = _lib.fn("ossid_bop_vsd")

    def cost():
        rc = fn(O.data_ptr(), cams.data_ptr(), 1, HW[0], HW[1], z_est.data_ptr(), z_gt.data_ptr(), frame.ctypes.data, N, DIAMETER,
                0.015, taus.ctypes.data, 10, counts.data_ptr(), errors.data_ptr(), _lib.stream())
        assert rc == 0, rc
    parts = {"render_est": lambda: render.render_depth(mesh, Te, K, HW, pixel_offset=0.0),
             "render_gt": lambda: render.render_depth(mesh, Tg, K, HW, pixel_offset=0.0), "cost": cost}
    if trace:
        for f in parts.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        return None
    row = {"estimates": N, "triangles": mesh.n_faces, "frame": list(HW)}
    for name, f in parts.items():
        row[name] = event_ms(f, reps=10, rounds=7)
        row[name]["us_per_estimate"] = 1e3 * row[name]["ms"] / N
    row["us_per_estimate"] = sum(row[k]["us_per_estimate"] for k in parts)
    cost()
    torch.cuda.synchronize()
    c = counts.cpu().numpy()
    row["mean_n_U"], row["mean_n_I"] = float(c[:, 0].mean()), float(c[:, 1].mean())
    # the restatement's cost pass on the same renders, and one render of its own
    k = min(4, N)
    ze, zg = z_est[:k].cpu().numpy(), z_gt[:k].cpu().numpy()
    t0 = time.perf_counter()
    for i in range(k):
        wc, _e = rb.vsd_from_renders(depth, rb.cam4(K), ze[i], zg[i], DIAMETER)
        assert wc.tolist() == c[i].tolist()
    row["numpy_cost_ms_per_estimate"] = 1e3 * (time.perf_counter() - t0) / k
    return row


def alternating_ms(fns, reps, rounds):
    """event_ms for several callables whose windows alternate round by round (a, b, a, b ...), so that a drift of the
    clocks meets all of them alike."""
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


def multi_instance_leg(mesh, depth, K, T, n):
    """A group of n kept estimates and n instances at 480 x 640 (SPEC 8.11): vsd_pairs' form -- n + n renders and one
    ossid_bop_vsd_pairs over the n x n table -- against the only way the single-instance entry has to the same numbers, every
    pair a row of its own: n x n + n x n renders and ossid_bop_vsd over n x n rows. Device parts on device-resident inputs
    as in vsd_parts, then the two Python calls whole (uploads, read-back and host work included)."""
    dev = mesh.device
    rng = np.random.default_rng(n)
    gt = np.stack([ri.perturb(T, rng.normal(size=3), 40.0 * rng.random(), np.array([0.12, 0.08, 0.05]) * rng.uniform(-1, 1, 3))
                   for _ in range(n)])
    est = np.stack([ri.perturb(g, rng.normal(size=3), 5.0 * rng.random(), rng.normal(size=3) * 0.01 * rng.random()) for g in gt])
    pairs = np.array([(e, g, 0) for e in range(n) for g in range(n)], dtype=np.int32)
    P = len(pairs)
    O = torch.from_numpy(depth[None]).to(dev)
    cams = torch.from_numpy(bop_eval._cameras(K, 1)).to(dev)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, torch.float32)  # noqa: E731
    Te, Tg, Tex, Tgx = f32(est), f32(gt), f32(est[pairs[:, 0]]), f32(gt[pairs[:, 1]])
    tab = torch.from_numpy(pairs).to(dev)
    frame, taus = np.zeros(P, dtype=np.int32), np.asarray(bop_eval.VSD_TAUS)
    rd = lambda poses: render.render_depth(mesh, poses, K, HW, pixel_offset=0.0)  # noqa: E731
    z_est, z_gt, z_estx, z_gtx = rd(Te), rd(Tg), rd(Tex), rd(Tgx)
    out = {k: (torch.empty(P, 12, dtype=torch.int32, device=dev), torch.empty(P, 10, dtype=torch.float64, device=dev))
           for k in ("pairs", "expanded")}
    fn_p, fn_x = _lib.fn("ossid_bop_vsd_pairs"), _lib.fn("ossid_bop_vsd")

    def cost_pairs():
        rc = fn_p(O.data_ptr(), cams.data_ptr(), 1, HW[0], HW[1], z_est.data_ptr(), n, z_gt.data_ptr(), n, tab.data_ptr(), P, DIAMETER,
                  0.015, taus.ctypes.data, 10, out["pairs"][0].data_ptr(), out["pairs"][1].data_ptr(), _lib.stream())
        assert rc == 0, rc

    def cost_expanded():
        rc = fn_x(O.data_ptr(), cams.data_ptr(), 1, HW[0], HW[1], z_estx.data_ptr(), z_gtx.data_ptr(), frame.ctypes.data, P, DIAMETER,
                  0.015, taus.ctypes.data, 10, out["expanded"][0].data_ptr(), out["expanded"][1].data_ptr(), _lib.stream())
        assert rc == 0, rc
    row = {"estimates": n, "instances": n, "pairs": P, "triangles": mesh.n_faces, "frame": list(HW),
           "renders": {"pairs": 2 * n, "expanded": 2 * P}, "expected_render_ratio": (n + n) / (2.0 * n * n)}
    row["render"] = alternating_ms({"pairs": lambda: (rd(Te), rd(Tg)), "expanded": lambda: (rd(Tex), rd(Tgx))}, reps=10, rounds=7)
    row["cost"] = alternating_ms({"pairs": cost_pairs, "expanded": cost_expanded}, reps=10, rounds=7)
    cost_pairs(), cost_expanded()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out["pairs"], out["expanded"])), "the two forms disagree"
    c = out["pairs"][0].cpu().numpy()
    row["mean_n_U"], row["pairs_with_overlap"] = float(c[:, 0].mean()), int((c[:, 1] > 0).sum())
    got = {}

    def call_pairs():
        got["pairs"] = bop_eval.vsd_pairs(mesh, DIAMETER, O, K, est, gt, pairs)

    def call_expanded():
        got["expanded"] = bop_eval.vsd(mesh, DIAMETER, O, K, est[pairs[:, 0]], gt[pairs[:, 1]], chunk=_lib.RASTER_MAX_POSES)
    row["python_call"] = alternating_ms({"pairs": call_pairs, "expanded": call_expanded}, reps=3, rounds=7)
    assert np.array_equal(got["pairs"], got["expanded"])
    for part in ("render", "cost", "python_call"):
        row[part]["ratio"] = row[part]["pairs"]["ms"] / row[part]["expanded"]["ms"]
    dev_p, dev_x = (row["render"][k]["ms"] + row["cost"][k]["ms"] for k in ("pairs", "expanded"))
    row["device_ms"] = {"pairs": dev_p, "expanded": dev_x, "ratio": dev_p / dev_x}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multi", action="store_true",
                    help="the multi-instance leg alone (groups of 4 and 12) -> profiles/bop_eval_multi.json unless --out is given")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--n", type=int, default=64, help="estimates per VSD batch")
    ap.add_argument("--trace", action="store_true", help="a few untimed calls per workload, for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bop_eval_bench.py needs the GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    depth, K, T, _pts = ri.scene()
    V, F = rr.bump_mesh(5)
    mesh = render.Mesh(V, F)
    args.out = args.out or os.path.join(ROOT, "profiles", "bop_eval_multi.json" if args.multi else "bop_eval.json")
    if args.multi:
        res = {"vsd_pairs_level5_480x640": {}}
        for n in (4, 12):
            res["vsd_pairs_level5_480x640"]["E%d_G%d" % (n, n)] = row = multi_instance_leg(mesh, depth, K, T, n)
            print("vsd_pairs", n, row, flush=True)
        write(res, args)
        return
    res = {"vsd_level5_480x640": {}, "mssd_mspd_level5_N1024": {}}
    for n in sorted(set((1, args.n))):
        row = vsd_parts(mesh, depth, K, estimates(T, n), np.stack([T] * n), args.trace)
        if row is not None:
            res["vsd_level5_480x640"]["N%d" % n] = row
            print("vsd N", n, row, flush=True)
    if not args.trace:
        t0 = time.perf_counter()
        rr.render(V, F, T, K, HW, pixel_offset=0.0)
        res["vsd_level5_480x640"]["numpy_render_ms_per_pose"] = 1e3 * (time.perf_counter() - t0)
    N = 1024
    gt = estimates(T, N, seed=1)
    est = np.stack([ri.perturb(g, [0.2, 1.0, 0.4], 3.0, [0.002, -0.001, 0.004]) for g in gt])
    lathe = {"symmetries_continuous": [{"axis": [0.0, 0.0, 1.0], "offset": [0.0, 0.0, 0.0]}]}
    for S, info in ((1, {}), (315, lathe)):
        syms = bop_eval.symmetry_transformations(info)
        dev = mesh.device
        Sd, ped, pgd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (syms, est, gt))
        cams = torch.from_numpy(bop_eval._cameras(K, 1)).to(dev)
        frame = np.zeros(N, dtype=np.int32)
        out = torch.empty(2, N, dtype=torch.float64, device=dev)
        fn = _lib.fn("ossid_bop_mssd_mspd")

        def run():
            rc = fn(mesh.vertices.data_ptr(), mesh.n_vertices, Sd.data_ptr(), S, ped.data_ptr(), pgd.data_ptr(), cams.data_ptr(), 1,
                    frame.ctypes.data, N, out[0].data_ptr(), out[1].data_ptr(), _lib.stream())
            assert rc == 0, rc
        if args.trace:
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            continue
        row = event_ms(run, reps=10 if S == 1 else 3, rounds=7)
        row.update(estimates=N, vertices=mesh.n_vertices, symmetries=S, us_per_estimate=1e3 * row["ms"] / N,
                   vertex_transform_pairs_per_s=N * S * mesh.n_vertices / (1e-3 * row["ms"]))
        k = 4 if S == 1 else 1
        t0 = time.perf_counter()
        wm, wp = rb.mssd_mspd(V, syms, est[:k], gt[:k], K)
        row["numpy_ms_per_estimate"] = 1e3 * (time.perf_counter() - t0) / k
        got = out.cpu().numpy()
        assert np.array_equal(got[0, :k], wm) and np.array_equal(got[1, :k], wp)
        res["mssd_mspd_level5_N1024"]["S%d" % S] = row
        print("mssd_mspd S", S, row, flush=True)
    if args.trace:
        return
    write(res, args)


def write(res, args):
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    res.update(commit=commit, cpus=int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
               box={"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
