"""Times the detection mAP (csrc/det_eval.hip, SPEC.md section 10) -> profiles/det_eval.json:

  det_eval.evaluate from host arrays (validation, upload, match, read-back; a host clock around a call that ends in the
  read-back) and det_eval.match on device tensors (device events) at N = 2^16, 2^20, 2^22 detections (LM-O-like: 8 classes, 5
  ground truths and 20 detections per image, so that G = N / 4 stays within the cap of 2^20), T = 1 and T = 10 IoU
  thresholds; match split into its three parts -- the claim launch, the sort (the library's stable sort of the keys plus the
  classes' offsets: plumbing), and the rest (ossid_det_match);
  beside it the numpy restatement (tests/ref_det_eval.py, vectorised) on the same inputs, timed in the same run on the box's
  CPUs (the median of three runs after a warm-up up to 2^20; one run at 2^22), and at N = 2^12 also its sequential loop, the
  reference class's algorithm -- baselines for orientation, not targets.

    python3 tools/det_eval_bench.py [--out profiles/det_eval.json] [--commit ID] [--sizes 16 20 22]

Device times are events around `reps` back-to-back calls after a warm-up, the median of `rounds` such windows. The file is
rewritten after every row, with the date and the device's clocks as the runtime reports them.
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

import ref_det_eval as rde  # noqa: E402
from ossid_code_amd import _lib, det_eval  # noqa: E402

C, GT_PER_IMAGE, DET_PER_IMAGE = 8, 5, 20


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


def host_ms(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return {"ms": float(np.median(out)), "ms_min": float(min(out)), "ms_max": float(max(out)), "runs": runs}


def current_clock_mhz():
    """The engine clock as the management library reports it, None where it is not installed (the clocks are left at the
    machine's defaults either way: the tool sets nothing)."""
    try:
        return float(torch.cuda.clock_rate(0))
    except Exception:
        return None


def make(N, seed=0):
    rng = np.random.RandomState(seed)
    I = max(1, N // DET_PER_IMAGE)
    G = I * GT_PER_IMAGE
    assert G <= det_eval.G_MAX and I <= det_eval.I_MAX, (N, G, I)
    gt_image = np.repeat(np.arange(I), GT_PER_IMAGE).astype(np.int32)
    xy, wh = rng.uniform(0, 480, (G, 2)), rng.uniform(40, 160, (G, 2))
    gt_box = np.concatenate([xy, xy + wh], 1).astype(np.float32)
    gt_cls = rng.randint(0, C, G).astype(np.int32)
    det_image = rng.randint(0, I, N).astype(np.int32)
    pick = det_image * GT_PER_IMAGE + rng.randint(0, GT_PER_IMAGE, N)
    box = gt_box[pick] + rng.normal(0, 12.0, (N, 4))
    det_box = np.concatenate([np.minimum(box[:, :2], box[:, 2:]), np.maximum(box[:, :2], box[:, 2:])], 1).astype(np.float32)
    det_cls = np.where(rng.uniform(size=N) > 0.2, gt_cls[pick], rng.randint(0, C, N)).astype(np.int32)
    return {"det_box": det_box, "det_score": rng.uniform(size=N).astype(np.float32), "det_cls": det_cls, "det_image": det_image,
            "gt_box": gt_box, "gt_cls": gt_cls, "gt_image": gt_image, "gt_offset": (np.arange(I + 1) * GT_PER_IMAGE).astype(np.int32),
            "gt_difficult": (rng.uniform(size=G) < 0.1).astype(np.uint8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_eval.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[16, 20, 22])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    prop = torch.cuda.get_device_properties(0)
    res = {"classes": C, "gt_per_image": GT_PER_IMAGE, "det_per_image": DET_PER_IMAGE, "commit": commit, "date": time.strftime("%Y-%m-%d"),
           "cpus": int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
           "box": {"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
                   "compute_units": prop.multi_processor_count, "max_engine_clock_mhz": (getattr(prop, "clock_rate", 0) / 1e3) or None,
                   "max_memory_clock_mhz": (getattr(prop, "memory_clock_rate", 0) / 1e3) or None,
                   "engine_clock_mhz_now": current_clock_mhz()}, "rows": []}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for lg in args.sizes:
        N = 1 << lg
        c = make(N)
        d = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
        det = {"boxes": c["det_box"], "scores": c["det_score"], "classes": c["det_cls"], "images": c["det_image"]}
        gt = {"boxes": c["gt_box"], "classes": c["gt_cls"], "images": c["gt_image"], "difficult": c["gt_difficult"]}
        names = ["c%d" % k for k in range(C)]
        I, G = len(c["gt_offset"]) - 1, len(c["gt_cls"])
        for T in (1, 10):
            thr = tuple(float(np.float32(0.5 + 0.05 * k)) for k in range(T))
            full = lambda: det_eval.match(d["det_box"], d["det_score"], d["det_cls"], d["det_image"], d["gt_box"], d["gt_cls"],
                                          d["gt_offset"], C, d["gt_difficult"], thr)
            m = full()
            best_gt, best_iou, key = m["best_gt"], m["best_iou"], torch.empty(N, dtype=torch.int64, device=dev)
            claim = lambda: _lib.check(_lib.fn("ossid_det_claim")(
                d["det_box"].data_ptr(), d["det_score"].data_ptr(), d["det_cls"].data_ptr(), d["det_image"].data_ptr(), N,
                d["gt_box"].data_ptr(), d["gt_cls"].data_ptr(), d["gt_offset"].data_ptr(), G, I, C, best_gt.data_ptr(), best_iou.data_ptr(),
                key.data_ptr(), _lib.stream()), "ossid_det_claim")
            claim()

            def sort():
                order = torch.sort(key, stable=True)[1].to(torch.int32)
                return order, det_eval.class_offsets(d["det_cls"], C)
            order, off = sort()
            nbytes = _lib.fn("ossid_det_eval_workspace_bytes")(N, G, C, T)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            tarr = np.asarray(thr, np.float32)
            rest = lambda: _lib.check(_lib.fn("ossid_det_match")(
                best_gt.data_ptr(), best_iou.data_ptr(), order.data_ptr(), off.data_ptr(), N, d["gt_cls"].data_ptr(),
                d["gt_difficult"].data_ptr(), G, C, tarr.ctypes.data, T, ws.data_ptr(), nbytes, m["status"].data_ptr(),
                m["n_easy"].data_ptr(), m["p11"].data_ptr(), m["ap11"].data_ptr(), m["apa"].data_ptr(), m["map11"].data_ptr(),
                m["mapa"].data_ptr(), None, None, None, None, None, _lib.stream()), "ossid_det_match")
            reps = 10 if lg <= 20 else 3
            row = {"N": N, "G": G, "T": T, "workspace_bytes": int(nbytes), "match": event_ms(full, reps, 7), "claim": event_ms(claim, reps, 7),
                   "sort": event_ms(sort, reps, 7), "rest": event_ms(rest, reps, 7)}
            row["evaluate_host"] = host_ms(lambda: det_eval.evaluate(det, gt, names, thr, n_images=I), 5 if lg <= 20 else 3)
            ref = lambda: rde.evaluate(c["det_box"], c["det_score"], c["det_cls"], c["det_image"], c["gt_box"], c["gt_cls"], c["gt_offset"],
                                       c["gt_difficult"], C, thr)
            if lg <= 20:
                row["numpy"] = host_ms(ref, 3)
            else:
                t0 = time.perf_counter()
                ref()
                row["numpy"] = {"ms": 1e3 * (time.perf_counter() - t0), "runs": 1}
            r = ref() if lg <= 16 else None                # the comparison itself is the tests' business; a spot check here
            if r is not None:
                assert np.array_equal(m["status"].cpu().numpy(), r["status"]) and m["ap11"].cpu().numpy().tobytes() == r["ap11"].tobytes()
            res["rows"].append(row)
            write()
            print(row, flush=True)
    c = make(1 << 12)
    t0 = time.perf_counter()
    rde.evaluate(c["det_box"], c["det_score"], c["det_cls"], c["det_image"], c["gt_box"], c["gt_cls"], c["gt_offset"], c["gt_difficult"], C,
                 (0.5,), sequential=True)
    res["sequential_loop_N4096_T1_ms"] = 1e3 * (time.perf_counter() - t0)
    print("sequential loop, N = 4096:", res["sequential_loop_N4096_T1_ms"], "ms", flush=True)
    write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
