"""Measures the detector's pre-training loop on rendered scenes (SPEC.md 15) and writes two files to profiles/:

  pretrain_producer.json   one batch of 8 at 480x640, median of --reps after 3 warm-ups, HIP events: the device producer
                           (dtoid.pretrain.scene_batch + the template gather), the host route it replaces
                           (SceneBatch.frames -> pipeline.make_dtoid_sample x 8 -> collate), a refresh (backgrounds,
                           render_scenes, select_targets) amortised over its batches, and finetune_step of the same run
  pretrain_curve.json      tools/pretrain_dtoid.py for --steps steps on a models folder written by SceneBatch.write_bop:
                           the loss per step, validation seg_IoU and AP at the start and the end

    python tools/bench_pretrain.py [--reps 20] [--steps 200] [--skip-curve] [--lights [--shadows]] [--rest]

--lights and --shadows measure the producer with lit (SPEC 13.11-13.12) and shadowed (13.13-13.15) scenes; the producer's
file is then pretrain_producer_lit.json or pretrain_producer_shadow.json, and the curve is left alone. --rest rests the
objects on a table (SPEC 13.16-13.18) -> pretrain_producer_rest.json (with the other flags: ..._rest_lit / ..._rest_shadow),
no curve: `layouts_sensor` among the refresh's parts then holds the drop's launch and read-back.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _sphere(n_lat=12, n_lon=24):
    """A unit latitude / longitude sphere -> (V f64 [V,3], F int32 [F,3]), wound outwards."""
    V = [(0.0, 0.0, 1.0)]
    for a in range(1, n_lat):
        t = np.pi * a / n_lat
        V += [(np.sin(t) * np.cos(2 * np.pi * b / n_lon), np.sin(t) * np.sin(2 * np.pi * b / n_lon), np.cos(t)) for b in range(n_lon)]
    V.append((0.0, 0.0, -1.0))
    ring = lambda a, b: 1 + (a - 1) * n_lon + b % n_lon
    F = [(0, ring(1, b), ring(1, b + 1)) for b in range(n_lon)]
    for a in range(1, n_lat - 1):
        for b in range(n_lon):
            F += [(ring(a, b), ring(a + 1, b), ring(a + 1, b + 1)), (ring(a, b), ring(a + 1, b + 1), ring(a, b + 1))]
    F += [(len(V) - 1, ring(n_lat - 1, b + 1), ring(n_lat - 1, b)) for b in range(n_lon)]
    return np.asarray(V, dtype=np.float64), np.asarray(F, dtype=np.int32)


def write_models(root, seed=0):
    """Four small vertex-coloured objects -> the models folder of a BOP dataset written by SceneBatch.write_bop."""
    from ossid_code_amd import render, scenes, synth
    rng = np.random.default_rng(seed)
    V, F = _sphere()
    shapes = {1: V * 0.07, 2: V * (0.09, 0.05, 0.05), 3: V * (0.04, 0.04, 0.10), 4: np.sign(V) * np.abs(V) ** 0.4 * 0.06}
    meshes = {}
    for o, P in shapes.items():
        C = (np.clip(0.5 + 0.5 * np.sin(P * rng.uniform(40.0, 120.0, 3) + rng.uniform(0, 6, 3)), 0, 1) * 255).astype(np.uint8)
        meshes[o] = render.Mesh(P, F, colors=C)
    atlas = scenes.MeshAtlas(meshes)
    layout = scenes.sample_layouts(atlas, 1, 4, synth.CAM_K, (480, 640), rng)
    scenes.render_scenes(atlas, layout, (480, 640)).write_bop(root, "synth")
    return os.path.join(root, "synth", "models")


def _median_ms(fn, reps, warm=3, before=None):
    """Median over reps of (HIP-event ms, host wall ms) of fn(), each rep synchronised on its own."""
    ev, wall = [], []
    for k in range(warm + reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        if k >= warm:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall))


def refresh_parts(train, reps, warm=3):
    """Median host wall ms of each part of ScenePretrainSet._refresh, run one after the other with the device drained in
    between (so a part's figure holds its own device work too)."""
    from ossid_code_amd import scenes
    from ossid_code_amd.dtoid import pretrain
    parts = {k: [] for k in ("layouts_sensor", "backgrounds", "render_scenes", "select_targets", "plan", "uploads")}

    def timed(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        parts[name].append((time.perf_counter() - t0) * 1e3)
        return out
    for _ in range(warm + reps):
        layout, sensor = timed("layouts_sensor", train.draw_targets)
        bg = timed("backgrounds", lambda: train._backgrounds(train.n_scenes))
        lights = material = None
        if train.lights:
            lights, material = scenes.sample_lights(layout, np.random.default_rng(0))
        batch = timed("render_scenes", lambda: scenes.render_scenes(train.atlas, layout, train.hw, background=bg, sensor=sensor,
                                                                    lights=lights, material=material, shadows=train.shadows))
        targets = timed("select_targets", lambda: pretrain.select_targets(batch, train.obj_ids, train.min_visib, train.min_px))
        plan = timed("plan", lambda: train.plan(layout, targets))
        timed("uploads", lambda: [torch.from_numpy(a).to(train.atlas.device) for a in (plan[0], plan[1], plan[2], plan[4])])
    return {k: float(np.median(v[warm:])) for k, v in parts.items()}


def producer(models, reps, lights=False, shadows=False, rest=False):
    from ossid_code_amd import dtoid, pipeline
    from ossid_code_amd.dtoid import pretrain
    from pretrain_dtoid import build_sets
    train, _val, line = build_sets(models, 8, 8, 4, 0, 1.0, 0, lights=lights, shadows=shadows, rest=rest)
    print(line, flush=True)
    res = {"batch": 8, "hw": [480, 640], "scenes_per_refresh": 8, "objects_per_scene": 4, "reps": reps, "lights": bool(lights), "rest": bool(rest),
           "shadows": None if train.shadows is None else {"size": list(train.shadows.size), "beta": list(train.shadows.beta)}}

    # a refresh: layouts + sensor, backgrounds, render_scenes, select_targets (one read-back of gt_info), the plan, its uploads
    def refresh():
        train._queue.clear()
        train._refresh()
    ev, wall = _median_ms(refresh, reps)
    n_batches = len(train._queue)
    res["refresh_ms"], res["refresh_host_ms"], res["batches_per_refresh"] = ev, wall, n_batches
    res["render_amortised_ms_per_batch"] = max(ev, wall) / n_batches
    res["refresh_parts_host_ms"] = refresh_parts(train, reps)

    # the device producer: scene_batch + the template gather
    def refill():
        if not train._queue:
            train._refresh()
    res["device_producer_ms"], res["device_producer_host_ms"] = _median_ms(lambda: next(train), reps, before=refill)

    # the host route of the same targets: frames() -> make_dtoid_sample x 8 -> collate (the read-back included)
    batch = train.render_batch
    objects = [(s, i) for s, i, _k in batch._objects()]
    want = [objects.index((int(s), int(i))) for s, i in pretrain.select_targets(batch)[:8]]
    assert len(want) == 8

    def host_route():
        batch._host_cache = None
        frames = list(batch.frames())
        return pipeline.collate([pipeline.make_dtoid_sample(frames[k]["img"], frames[k]["depth"], frames[k]["mask_gt_visib"],
                                                            frames[k]["cam_K"]) for k in want])
    res["host_route_ms"], res["host_route_host_ms"] = _median_ms(host_route, reps)

    # the step of the same run
    torch.manual_seed(0)
    trainer = pretrain.DtoidPretrainer(dtoid.DtoidNet(dtoid.DtoidConfig()).cuda(), train)
    fixed = next(train)
    trainer.model.train()

    def step():
        pretrain.finetune.finetune_step(trainer.model, fixed, trainer.optimizer)
    res["finetune_step_ms"], res["finetune_step_host_ms"] = _median_ms(step, reps)
    # the loop as the tool runs it, the loss read every step
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 3 * n_batches
    for _ in range(n):
        float(trainer.step())
    res["loop_ms_per_step"] = (time.perf_counter() - t0) * 1e3 / n
    res["producer_plus_render_ms"] = res["device_producer_ms"] + res["render_amortised_ms_per_batch"]
    res["producer_plus_render_over_step"] = res["producer_plus_render_ms"] / res["finetune_step_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--skip-curve", action="store_true")
    ap.add_argument("--lights", action="store_true", help="light the scenes -> pretrain_producer_lit.json, no curve")
    ap.add_argument("--shadows", action="store_true", help="with --lights: cast shadows -> pretrain_producer_shadow.json")
    ap.add_argument("--rest", action="store_true", help="rest the objects on a table -> pretrain_producer_rest.json, no curve")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.shadows and not a.lights:
        raise SystemExit("--shadows needs --lights: shadows are cast by lights")
    if not torch.cuda.is_available():
        raise SystemExit("bench_pretrain.py measures on the GPU")
    os.makedirs(a.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        models = write_models(tmp)
        res = producer(models, a.reps, a.lights, a.shadows, a.rest)
        print(json.dumps(res), flush=True)
        name = "pretrain_producer%s%s.json" % ("_rest" if a.rest else "", "_shadow" if a.shadows else "_lit" if a.lights else "")
        with open(os.path.join(a.out, name), "w") as f:
            json.dump(res, f, indent=1)
        if not a.skip_curve and not a.lights and not a.rest:
            curve_path = os.path.join(tmp, "curve.json")
            cmd = [sys.executable, os.path.join(ROOT, "tools", "pretrain_dtoid.py"), "--models", models, "--steps", str(a.steps),
                   "--out", os.path.join(tmp, "ckpt.pt"), "--views", "1", "--val_every", str(a.steps), "--curve", curve_path]
            t0 = time.perf_counter()
            subprocess.run(cmd, check=True, timeout=900)
            with open(curve_path) as f:
                curve = json.load(f)
            curve.update(command="tools/pretrain_dtoid.py --models MODELS --steps %d --out ckpt.pt --views 1 --val_every %d" % (a.steps, a.steps),
                         wall_s=time.perf_counter() - t0, checkpoint_bytes=os.path.getsize(os.path.join(tmp, "ckpt.pt")))
            k = max(1, len(curve["loss"]) // 10)
            curve["loss_mean_first_tenth"], curve["loss_mean_last_tenth"] = float(np.mean(curve["loss"][:k])), float(np.mean(curve["loss"][-k:]))
            print(json.dumps({k2: v for k2, v in curve.items() if k2 != "loss"}), flush=True)
            with open(os.path.join(a.out, "pretrain_curve.json"), "w") as f:
                json.dump(curve, f, indent=1)


if __name__ == "__main__":
    main()
