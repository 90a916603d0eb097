"""Pre-trains the DTOID detector on rendered scenes of a folder of BOP models (SPEC.md 15; the reference's python/ossid/train.py
over datasets/dtoid_dataset.py, whose BlenderProc renders are in neither tree) and writes the checkpoint
scripts/online_learning.py:153-167 starts from (--dtoid_weights_path; :161-162 loads ckpt['state_dict']).

    python tools/pretrain_dtoid.py --models MODELS_DIR --steps N --out ckpt.pt \
        [--batch 8] [--scenes 8] [--objects 4] [--views 2] [--jitter 1.0] [--val_every K] [--resume ckpt.pt] [--seed S]
        [--lights [--shadows]] [--rest]

MODELS_DIR holds .ply models, vertex-coloured or texture-mapped, in millimetres as BOP stores them (scenes.read_models_dir).
Every object's templates are rendered once (TemplateBank.add_mesh, the view grid of subdivision --views: 12, 42, 162 views);
the scenes are rendered --scenes at a time with --objects objects each, and every batch is made on the device
(dtoid.pretrain.ScenePretrainSet). Objects are split as the reference splits them (id % 4 == 0 validates); a folder that
leaves either side empty validates on the training objects, on scenes of another seed. One line per step. --lights
lights the scenes of both sets (scenes.sample_lights, SPEC.md 13.11-13.12); whether that helps on real frames is untested.
--rest rests the objects of both sets on a table (SPEC.md 13.16-13.18); the same holds for it.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_sets(models_dir, batch, n_scenes, n_objects, level, jitter, seed, hw=(480, 640), lights=False, shadows=False, rest=False):
    """-> (train set, validation set, the printed line about the split)."""
    from ossid_code_amd import pipeline, render, scenes, synth
    from ossid_code_amd.dtoid import pretrain
    meshes = scenes.read_models_dir(models_dir)
    atlas = scenes.MeshAtlas(meshes)
    bank = pipeline.TemplateBank()
    for o, m in meshes.items():
        bank.add_mesh(o, m, rotations=render.view_grid(level), cam_K=synth.CAM_K)
    train_ids, val_ids, shared = pretrain.split_objects(meshes)
    n_objects = min(n_objects, len(meshes))
    # a refresh is cut into whole batches: render enough scenes for about two batches of training targets
    per_scene = n_objects * len(train_ids) / float(len(meshes))
    n_scenes = min(256, max(n_scenes, int(-(-2 * batch // per_scene))))
    train = pretrain.ScenePretrainSet(atlas, bank, synth.CAM_K, hw, n_objects, n_scenes, batch, seed, obj_ids=train_ids, jitter=jitter,
                                      lights=lights, shadows=shadows, rest=rest)
    val = pretrain.ScenePretrainSet(atlas, bank, synth.CAM_K, hw, n_objects, n_scenes, batch, seed + 1000003, obj_ids=val_ids, jitter=None,
                                    drop_last=False, lights=lights, shadows=shadows, rest=rest)
    line = "%d objects, %d views each, %d scenes per refresh: train on %s, validate on %s%s" % (
        len(meshes), int(bank.img[train_ids[0]].shape[0]), n_scenes, train_ids, val_ids,
        " (the split by id %% 4 leaves one side empty: validating on the training objects, scenes of seed %d)" % (seed + 1000003)
        if shared else "")
    return train, val, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", required=True, help="a folder of .ply models, vertex-coloured or texture-mapped (millimetres)")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--scenes", type=int, default=8, help="scenes rendered per refresh")
    ap.add_argument("--objects", type=int, default=4, help="objects per scene")
    ap.add_argument("--views", type=int, default=2, help="subdivision level of the template view grid (0: 12 views, 2: 162)")
    ap.add_argument("--jitter", type=float, default=1.0, help="strength of the photometric jitter, 0 for none")
    ap.add_argument("--val_every", type=int, default=0, help="validate every K steps (and at the start and the end); 0: never")
    ap.add_argument("--val_batches", type=int, default=4)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--lights", action="store_true", help="light the rendered scenes (default: unlit)")
    ap.add_argument("--shadows", action="store_true", help="let the lights cast shadows (SPEC.md 13.13-13.15); needs --lights")
    ap.add_argument("--rest", action="store_true", help="rest the objects on a table (SPEC.md 13.16-13.18; default: free poses)")
    ap.add_argument("--curve", default=None, help="also write the losses and validation numbers to this JSON file")
    a = ap.parse_args()
    if a.shadows and not a.lights:
        raise SystemExit("--shadows needs --lights: shadows are cast by lights")
    if not torch.cuda.is_available():
        raise SystemExit("pretrain_dtoid.py trains on the GPU: there is no CPU path")
    from ossid_code_amd import dtoid
    from ossid_code_amd.dtoid import pretrain
    torch.manual_seed(a.seed)
    model = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda()
    trainer = pretrain.DtoidPretrainer(model, None, lr=a.lr)
    if a.resume:
        trainer.load(a.resume)
        print("resumed %s at iteration %d" % (a.resume, trainer.iteration), flush=True)
    # a resumed run draws new scenes: the sets' seed moves on with the iteration it starts from
    train, val, line = build_sets(a.models, a.batch, a.scenes, a.objects, a.views, a.jitter, a.seed + trainer.iteration,
                                   lights=a.lights, shadows=a.shadows, rest=a.rest)
    print(line, flush=True)
    trainer.train_set, trainer.val_set = train, val if a.val_every > 0 else None
    curve = {"loss": [], "val": [], "first_iteration": trainer.iteration}

    def validate():
        v = trainer.validate(a.val_batches)
        curve["val"].append(dict(v, iteration=trainer.iteration))
        print("iteration %5d  validation seg_IoU %.4f  AP@0.5 %.4f  (%d targets)" % (trainer.iteration, v["seg_IoU"], v["AP"], v["n"]), flush=True)
    if a.val_every > 0:
        validate()
    for k in range(a.steps):
        loss = float(trainer.step())
        curve["loss"].append(loss)
        print("iteration %5d  loss %.6f" % (trainer.iteration, loss), flush=True)
        if a.val_every > 0 and ((k + 1) % a.val_every == 0 or k + 1 == a.steps):
            validate()
    trainer.save(a.out)
    print("saved", a.out)
    if a.curve:
        with open(a.curve, "w") as f:
            json.dump(curve, f, indent=1)


if __name__ == "__main__":
    main()
