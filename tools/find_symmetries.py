"""Symmetries of the models of a BOP models folder, found from the meshes (symmetry.find_symmetries, SPEC.md section 17):

    python3 tools/find_symmetries.py MODELS_DIR [--write] [--tol_rel 0.05] [--max_miss 0] [--level 4] [--max_order 8]

Every MODELS_DIR/*.ply (obj_XXXXXX.ply keeps its id; vertex-coloured or texture-mapped) is read in the file's own unit
-- BOP's millimetres -- and its discrete and continuous symmetries are printed. --write merges them into
MODELS_DIR/models_info.json as `symmetries_discrete` / `symmetries_continuous`: every other key, and every object that has
no model in the folder, keeps what it had; an object found to have none loses the key. The definition is this build's
own: parity with BOP's published lists is unpinned.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("symmetries_discrete", "symmetries_continuous")


def merge(path, found):
    """found: dict obj_id -> find_symmetries' dict, in the file's unit. Rewrites models_info.json at `path`."""
    info = {}
    if os.path.exists(path):
        with open(path) as f:
            info = json.load(f)
    for obj, sym in found.items():
        entry = info.setdefault(str(obj), {})
        for k in KEYS:
            if sym.get(k):
                entry[k] = sym[k]
            else:
                entry.pop(k, None)
    with open(path, "w") as f:
        json.dump(info, f, indent=1)
    return info


def main():
    import torch

    from ossid_code_amd import scenes, symmetry
    ap = argparse.ArgumentParser()
    ap.add_argument("models_dir")
    ap.add_argument("--write", action="store_true", help="merge the findings into MODELS_DIR/models_info.json")
    ap.add_argument("--tol_rel", type=float, default=0.05)
    ap.add_argument("--max_miss", type=int, default=0)
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--max_order", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("find_symmetries.py scores on the GPU: there is no CPU path")
    found = {}
    for obj, mesh in sorted(scenes.read_models_dir(a.models_dir, scale=1.0).items()):
        sym, info = symmetry.find_symmetries(mesh, tol_rel=a.tol_rel, max_miss=a.max_miss, level=a.level, max_order=a.max_order,
                                             return_info=True)
        found[obj] = sym
        print("obj %d: diameter %.6g, tol %.6g, %d transforms scored -> %d discrete, %d continuous"
              % (obj, info["diameter"], info["tol"], info["n_scored"], len(sym["symmetries_discrete"]),
                 len(sym["symmetries_continuous"])))
        for m in sym["symmetries_discrete"]:
            print("   discrete  " + " ".join("%.6g" % v for v in m))
        for c in sym["symmetries_continuous"]:
            print("   continuous axis %s offset %s" % (" ".join("%.6g" % v for v in c["axis"]), " ".join("%.6g" % v for v in c["offset"])))
    if a.write:
        path = os.path.join(a.models_dir, "models_info.json")
        merge(path, found)
        print("merged into %s" % path)


if __name__ == "__main__":
    main()
