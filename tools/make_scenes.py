"""Cluttered RGB-D scenes with BOP ground truth from a folder of BOP models, vertex-coloured or texture-mapped (a .ply
that names its texture in `comment TextureFile`, the image beside it) -> a standard BOP folder:

    python3 tools/make_scenes.py MODELS_DIR OUT_DIR --scenes 32 --objects 6 --seed 0 [--name synth] [--split test]
                                 [--hw 480 640] [--no-mm2m] [--clean] [--no-table] [--depth_scale 1.0] [--lights [--shadows]]
                                 [--rest] [--symmetries]

Every MODELS_DIR/*.ply (obj_XXXXXX.ply keeps its id; millimetres, as BOP stores them, unless --no-mm2m) goes into one
atlas; scenes.sample_layouts places the objects, scenes.render_scenes (csrc/scene.hip, SPEC.md section 13) draws them with
the depth corruption of scenes.sample_sensor (--clean: quantisation only), and SceneBatch.write_bop writes
OUT_DIR/<name>: what bop_eval.BopFolder, tools/eval_bop19.py and scenes.read_bop_frames read. The same seed gives the same
folder. At most 256 scenes per call. --lights lights the scenes (scenes.sample_lights, SPEC.md 13.11-13.12) from a
generator of its own: rgb/ is lit, every other file is the one written without the flag at the same seed. --shadows (with
--lights) lets the lights cast shadows (scenes.Shadows, SPEC.md 13.13-13.15): again rgb/ alone differs. --rest rests the
objects on the table (scenes.sample_layouts(placement="rest"), SPEC.md 13.16-13.18) instead of letting them float: other
layouts, so every file differs from the folder written without the flag. --symmetries finds each object's symmetries from
its mesh (symmetry.find_symmetries, SPEC.md section 17) and writes them into models_info.json, which alone differs.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ossid_code_amd import scenes, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--objects", type=int, default=6)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--name", default="synth")
    ap.add_argument("--split", default="test")
    ap.add_argument("--hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--depth_scale", type=float, default=1.0)
    ap.add_argument("--no-mm2m", action="store_true", help="the models are already in metres")
    ap.add_argument("--clean", action="store_true", help="no depth corruption: quantisation only")
    ap.add_argument("--no-table", action="store_true")
    ap.add_argument("--lights", action="store_true", help="light the scenes: sampled lights and materials (default: unlit)")
    ap.add_argument("--shadows", action="store_true", help="let the lights cast shadows; needs --lights")
    ap.add_argument("--rest", action="store_true", help="rest the objects on the table, stacked where they overlap (default: free poses)")
    ap.add_argument("--symmetries", action="store_true", help="find each object's symmetries and write them into models_info.json")
    a = ap.parse_args()
    if a.shadows and not a.lights:
        raise SystemExit("--shadows needs --lights: shadows are cast by lights")
    if not torch.cuda.is_available():
        raise SystemExit("make_scenes.py renders on the GPU: there is no CPU path")
    if a.scenes > 256:
        raise SystemExit("at most 256 scenes per folder and call; use several seeds and names for more")
    atlas = scenes.MeshAtlas(scenes.read_models_dir(a.models_dir, scale=1.0 if a.no_mm2m else 0.001))
    rng = np.random.default_rng(a.seed)
    K = synth.CAM_K * np.array([[a.hw[1] / 640.0], [a.hw[0] / 480.0], [1.0]])
    layout = scenes.sample_layouts(atlas, a.scenes, a.objects, K, a.hw, rng, table=not a.no_table,
                                   placement="rest" if a.rest else "free")
    sensor = None if a.clean else scenes.sample_sensor(a.scenes, a.hw, rng)
    lights = material = None
    if a.lights:
        lights, material = scenes.sample_lights(layout, np.random.default_rng(np.random.SeedSequence(a.seed, spawn_key=(0,))))
    batch = scenes.render_scenes(atlas, layout, a.hw, sensor=sensor, depth_scale=a.depth_scale, lights=lights,
                                 material=material, shadows=scenes.Shadows() if a.shadows else None)
    base = batch.write_bop(a.out_dir, a.name, split=a.split, depth_scale=a.depth_scale, symmetries=a.symmetries)
    g = batch.gt_info.cpu().numpy()
    print("%d scenes, %d instances (%d visible) of %d objects -> %s" % (a.scenes, layout.n_instances, int((g[:, 1] > 0).sum()),
                                                                       atlas.n_meshes - 1, base))


if __name__ == "__main__":
    main()
