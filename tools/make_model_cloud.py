"""Zephyr's model clouds from a BOP models folder -> the files scripts/online_learning.py:303-311 loads:

    python3 tools/make_model_cloud.py MODELS_DIR OUT_DIR [--n_points 2048] [--oversample 16] [--level 2] [--view_size 512]
                                      [--no-mm2m]

Every MODELS_DIR/obj_XXXXXX.ply (vertex-coloured, or texture-mapped with its image beside it; millimetres, as BOP stores them, scaled to metres unless --no-mm2m)
becomes OUT_DIR/model_cloud_XX.npz with model_points / model_colors / model_normals as float64 [n_points,3] and `diameter`.
model_cloud.sample_model_cloud (SPEC.md section 9) does the work. The clouds are in the BOP frame of the .ply: a YCB-V
run that uses them must not also apply modelPointsShiftYcbv2Bop. Parity with zephyr's own clouds is unpinned.
"""
import argparse
import glob
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ossid_code_amd import model_cloud, render  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--n_points", type=int, default=2048)
    ap.add_argument("--oversample", type=int, default=16)
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--view_size", type=int, default=512)
    ap.add_argument("--no-mm2m", action="store_true", help="the models are already in metres")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("make_model_cloud.py samples on the GPU: there is no CPU path")
    paths = sorted(p for p in glob.glob(os.path.join(a.models_dir, "obj_*.ply")) if re.fullmatch(r"obj_\d{6}\.ply", os.path.basename(p)))
    if not paths:
        raise SystemExit("no obj_XXXXXX.ply in %s" % a.models_dir)
    os.makedirs(a.out_dir, exist_ok=True)
    for p in paths:
        obj = int(os.path.basename(p)[4:10])
        mesh = render.load_mesh(p, scale=1.0 if a.no_mm2m else 0.001)
        cloud = model_cloud.sample_model_cloud(mesh, n_points=a.n_points, oversample=a.oversample, level=a.level,
                                               view_size=a.view_size)
        out = os.path.join(a.out_dir, "model_cloud_{:02d}.npz".format(obj))
        cloud.save(out)
        print("obj %d: %d triangles -> %d points, diameter %.6g -> %s" % (obj, mesh.n_faces, len(cloud), cloud.diameter, out))


if __name__ == "__main__":
    main()
