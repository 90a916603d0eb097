"""Templates of an object from its vertex-coloured or texture-mapped PLY model -> an .npz the detector's TemplateBank can be filled from:

    python3 tools/make_templates.py obj_000001.ply obj_000001_templates.npz [--mm2m] [--level 2] [--inplane 1]
                                    [--size 124] [--supersample 4] [--distance 0.8] [--fx 572.4 --fy 573.6 --cx 325.3 --cy 242.0]

The file holds numeric arrays only: img f32 [n,3,T,T], mask f32 [n,1,T,T], rotations f64 [n,3,3], quats f64 [n,4] (xyzw),
template_z f64 [n], intrinsics f32 [n,4]. render.load_mesh reads the model (vertex colours, or the texture its header names,
looked for beside the .ply; a model with both is rendered from its vertex colours); render.render_templates (SPEC.md 7.13-7.14) does the work;
`TemplateBank.add(obj_id, z["img"], z["mask"], z["quats"])` takes the result, and `TemplateBank.add_mesh` skips the file.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ossid_code_amd import render, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ply")
    ap.add_argument("out")
    ap.add_argument("--mm2m", action="store_true", help="the model is in millimetres (BOP): scale by 0.001")
    ap.add_argument("--level", type=int, default=2)
    ap.add_argument("--inplane", type=int, default=1)
    ap.add_argument("--size", type=int, default=124)
    ap.add_argument("--supersample", type=int, default=4)
    ap.add_argument("--distance", type=float, default=0.8)
    ap.add_argument("--views-per-call", type=int, default=32)
    for k, name in enumerate(("fx", "fy", "cx", "cy")):
        ap.add_argument("--" + name, type=float, default=float(synth.CAM_K[(0, 1, 0, 1)[k]][(0, 1, 2, 2)[k]]))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("make_templates.py renders on the GPU: there is no CPU path")
    mesh = render.load_mesh(a.ply, scale=0.001 if a.mm2m else 1.0)
    K = np.array([[a.fx, 0.0, a.cx], [0.0, a.fy, a.cy], [0.0, 0.0, 1.0]])
    img, mask, info = render.render_templates(mesh, rotations=render.view_grid(a.level, a.inplane), size=a.size,
                                              supersample=a.supersample, distance=a.distance, cam_K=K,
                                              views_per_call=a.views_per_call)
    np.savez_compressed(a.out, img=img.cpu().numpy(), mask=mask.cpu().numpy(), rotations=info["rotations"], quats=info["quats"],
                        template_z=info["template_z"], intrinsics=info["intrinsics"])
    print("%d views of %d triangles -> %s" % (len(img), mesh.n_faces, a.out))


if __name__ == "__main__":
    main()
