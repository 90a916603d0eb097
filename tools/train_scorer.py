"""Smoke driver of the scorer's training path (SPEC.md 12): fits PointNet2SSG on the synthetic cfg-2 frame of SURVEY 8d with
ScorerTrainer and prints the loss per step. --out saves {'state_dict': ...}, the form scripts/online_learning.py:213-214
loads (ckpt = torch.load(path); model.load_state_dict(ckpt['state_dict'])).

    python tools/train_scorer.py --steps 20 --hypotheses 64 --out ckpt.pt

The loss and the recipe are this build's own (zephyr's are in neither tree): unpinned.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from ossid_code_amd import scoring, synth, zephyr
    from ossid_code_amd.zephyr.train import ScorerTrainer

    class Args:
        pass
    torch.manual_seed(a.seed)
    dataset = zephyr.ScoreDataset([], "", "", Args(), mode="train")
    model = synth.random_pn2_state(zephyr.PointNet2SSG(dataset.dim_point, Args(), num_class=1), a.seed).to(0)
    data = synth.make_scoring_inputs(N=a.hypotheses, M=a.points)
    data["pp_err"] = scoring.pose_errors(data["pose_hypos"], data["pose_hypos"][0], data["model_points"])
    trainer = ScorerTrainer(model, dataset, torch.optim.Adam(model.parameters(), lr=a.lr),
                            generator=torch.Generator().manual_seed(a.seed))
    for step in range(a.steps):
        print("step %3d  loss %.6f" % (step, trainer.step(data)), flush=True)
    if a.out:
        torch.save({"state_dict": model.state_dict()}, a.out)
        print("saved", a.out)


if __name__ == "__main__":
    main()
