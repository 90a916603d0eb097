"""Smoke driver of the scorer's training path (SPEC.md 12): fits PointNet2SSG on the synthetic cfg-2 frame of SURVEY 8d with
ScorerTrainer and prints the loss per step. --out saves {'state_dict': ...}, the form scripts/online_learning.py:213-214
loads (ckpt = torch.load(path); model.load_state_dict(ckpt['state_dict'])).

    python tools/train_scorer.py --steps 20 --hypotheses 64 --out ckpt.pt
    python tools/train_scorer.py --models MODELS_DIR --scenes 8 --objects 4 --steps 200 --out ckpt.pt [--lights [--shadows]] [--rest]

With --models the frames are rendered scenes (scenes.render_scenes, SPEC.md 13) of the .ply models of MODELS_DIR,
vertex-coloured or texture-mapped (millimetres, as BOP stores them), with the sampled depth corruption; every step takes the next (scene, object)
frame whose object is at least --min_visib visible, scores synth.perturb_pose hypotheses around its pose_gt against the
object's own model cloud (model_cloud.sample_model_cloud), with pp_err from scoring.pose_errors. --lights lights the
scenes (scenes.sample_lights, SPEC.md 13.11-13.12), so that the true pose no longer has dS = dV = 0; --shadows (with
--lights) lets those lights cast shadows (scenes.Shadows, SPEC.md 13.13-13.15). --rest rests the objects on a table
(scenes.sample_layouts(placement="rest"), SPEC.md 13.16-13.18).

The loss and the recipe are this build's own (zephyr's are in neither tree): unpinned.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene_frames(a):
    """-> (frames of rendered scenes whose object is visible enough, {obj_id: the object's model cloud as host arrays})."""
    import numpy as np

    from ossid_code_amd import model_cloud, scenes, synth
    meshes = scenes.read_models_dir(a.models)
    atlas = scenes.MeshAtlas(meshes)
    rng = np.random.default_rng(a.seed)
    hw = (480, 640)
    layout = scenes.sample_layouts(atlas, a.scenes, a.objects, synth.CAM_K, hw, rng, placement="rest" if a.rest else "free")
    sensor = scenes.sample_sensor(a.scenes, hw, rng)
    lights = material = None
    if a.lights:                                             # a generator of its own: the layouts and the sensor do not move
        lights, material = scenes.sample_lights(layout, np.random.default_rng(np.random.SeedSequence(a.seed, spawn_key=(0,))))
    batch = scenes.render_scenes(atlas, layout, hw, sensor=sensor, lights=lights, material=material,
                                 shadows=scenes.Shadows() if a.shadows else None)
    frames = [f for f in batch.frames() if f["visib_fract"] >= a.min_visib]
    if not frames:
        raise SystemExit("no object is at least %g visible in the %d scenes" % (a.min_visib, a.scenes))
    clouds = {o: {k: v.cpu().numpy() for k, v in model_cloud.sample_model_cloud(m, n_points=a.points).as_dict().items()}
              for o, m in meshes.items()}
    print("%d frames of %d scenes, %d objects" % (len(frames), a.scenes, len(meshes)), flush=True)
    return frames, clouds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default=None, help="a folder of .ply models, vertex-coloured or texture-mapped: train on rendered scenes of them")
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--objects", type=int, default=4, help="objects per scene (with --models)")
    ap.add_argument("--min_visib", type=float, default=0.25)
    ap.add_argument("--lights", action="store_true", help="light the rendered scenes (with --models; default: unlit)")
    ap.add_argument("--shadows", action="store_true", help="let the lights cast shadows (with --models; needs --lights)")
    ap.add_argument("--rest", action="store_true", help="rest the objects on a table (with --models; default: free poses)")
    a = ap.parse_args()
    if a.shadows and not a.lights:
        raise SystemExit("--shadows needs --lights: shadows are cast by lights")

    from ossid_code_amd import scoring, synth, zephyr
    from ossid_code_amd.zephyr.train import ScorerTrainer

    class Args:
        pass
    torch.manual_seed(a.seed)
    dataset = zephyr.ScoreDataset([], "", "", Args(), mode="train")
    model = synth.random_pn2_state(zephyr.PointNet2SSG(dataset.dim_point, Args(), num_class=1), a.seed).to(0)
    trainer = ScorerTrainer(model, dataset, torch.optim.Adam(model.parameters(), lr=a.lr),
                            generator=torch.Generator().manual_seed(a.seed))
    if a.models is None:
        data = synth.make_scoring_inputs(N=a.hypotheses, M=a.points)
        data["pp_err"] = scoring.pose_errors(data["pose_hypos"], data["pose_hypos"][0], data["model_points"])
        for step in range(a.steps):
            print("step %3d  loss %.6f" % (step, trainer.step(data)), flush=True)
    else:
        frames, clouds = scene_frames(a)
        for step in range(a.steps):
            fr = frames[step % len(frames)]
            data = {k: fr[k] for k in ("img", "depth", "cam_K")}
            data.update(clouds[fr["obj_id"]])
            data["pose_hypos"] = synth.perturb_pose(fr["pose_gt"], a.hypotheses, a.seed + step)
            data["pp_err"] = scoring.pose_errors(data["pose_hypos"], fr["pose_gt"], data["model_points"])
            print("step %3d  scene %d object %d  loss %.6f" % (step, fr["scene_id"], fr["obj_id"], trainer.step(data)), flush=True)
    if a.out:
        torch.save({"state_dict": model.state_dict()}, a.out)
        print("saved", a.out)


if __name__ == "__main__":
    main()
