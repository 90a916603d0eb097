"""One training step of the scorer (forward + backward, SPEC.md 12) at B = 256, M = 2048, npoint 512/128: the hand-written
path (csrc/pn2_train.hip) next to the same step in plain torch modules and autograd on the same device and the same
sampling indices, alternating the two. 3 warm-ups, median of --reps (>= 10), a device synchronise inside the timed window.
No pass / fail threshold; the measured pair goes into DESIGN.md.

    python tools/bench_scorer_train.py [--B 256] [--M 2048] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MATRIX = 155e12


def flops(B, np1, np2):
    """Algorithmic multiply-adds x 2 of one hypothesis: forward, and a step (forward + data gradient + weight gradient; the
    first layer of SA1 has no data gradient)."""
    rows = [np1 * 64] * 3 + [np2 * 64] * 3 + [np2] * 3 + [1] * 3
    k = [8, 64, 64, 131, 128, 128, 259, 256, 512, 1024, 512, 256]
    c = [64, 64, 128, 128, 128, 256, 256, 512, 1024, 512, 256, 1]
    fwd = sum(2.0 * r * kk * cc for r, kk, cc in zip(rows, k, c))
    return fwd, 3 * fwd - 2.0 * rows[0] * k[0] * c[0]


def torch_step(model, x, idx, keep, p_drop, dsc):
    """The same step with torch modules: gather by the given indices, Conv2d / BatchNorm2d / ReLU, max-pool, the head."""
    B = x.shape[0]
    xyz, feats = x[..., 0:3], x[..., 3:]

    def take(t, i):
        S, K = i.shape[1:]
        return t.gather(1, i.reshape(B, S * K, 1).expand(-1, -1, t.shape[2])).reshape(B, S, K, t.shape[2])
    xyz1 = xyz.gather(1, idx["fps1"][..., None].expand(-1, -1, 3))
    xyz2 = xyz1.gather(1, idx["fps2"][..., None].expand(-1, -1, 3))
    g = torch.cat([take(xyz, idx["ball1"]) - xyz1[:, :, None, :], take(feats, idx["ball1"])], -1).permute(0, 3, 1, 2)
    f1 = model.SA_modules[0].mlps[0](g).max(3).values.transpose(1, 2)
    g = torch.cat([take(xyz1, idx["ball2"]) - xyz2[:, :, None, :], take(f1, idx["ball2"])], -1).permute(0, 3, 1, 2)
    f2 = model.SA_modules[1].mlps[0](g).max(3).values.transpose(1, 2)
    g = torch.cat([xyz2, f2], -1).transpose(1, 2)[:, :, None, :]
    f3 = model.SA_modules[2].mlps[0](g).max(3).values.squeeze(-1)
    fc = model.fc_layer
    a = fc[5](fc[4](fc[3](fc[2](fc[1](fc[0](f3))))))
    s = fc[7](a * (keep.float() * (1.0 / (1.0 - p_drop))))
    s.backward(dsc)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--M", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from ossid_code_amd import _lib, synth, zephyr

    dev = torch.device("cuda", 0)
    model = synth.random_pn2_state(zephyr.PointNet2SSG(8, None, 1), 0).to(dev).train()
    np1, np2 = model.SA_modules[0].npoint, model.SA_modules[1].npoint
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(a.B, a.M, 8)
    x[..., 0:2] = torch.rand(a.B, a.M, 2, generator=g) - 0.5
    x[..., 3:] = torch.randn(a.B, a.M, 5, generator=g)
    x = x.to(dev)
    keep = model.draw_keep_mask(a.B, g).to(dev)
    dsc = torch.randn(a.B, 1, generator=g).to(dev)
    p_drop = float(model.fc_layer[6].p)
    dbg = {}
    model({"point_x": x}, keep_mask=keep, debug=dbg).backward(dsc)
    idx = {k: dbg[k].long() for k in ("fps1", "ball1", "fps2", "ball2")}
    del dbg

    def hip():
        model.zero_grad(set_to_none=True)
        model({"point_x": x}, keep_mask=keep).backward(dsc)

    def plain():
        model.zero_grad(set_to_none=True)
        torch_step(model, x, idx, keep, p_drop, dsc)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        hip()
        plain()
    t_hip, t_torch = [], []
    for _ in range(max(10, a.reps)):
        t_hip.append(timed(hip))
        t_torch.append(timed(plain))
    fwd, step = flops(a.B, np1, np2)
    ms_hip, ms_torch = statistics.median(t_hip), statistics.median(t_torch)
    print(json.dumps({
        "B": a.B, "M": a.M, "npoint": [np1, np2], "ms_hip": round(ms_hip, 3), "ms_torch": round(ms_torch, 3),
        "workspace_bytes": int(_lib.fn("ossid_pn2_train_workspace_bytes")(a.B, a.M, np1, np2)),
        "gflop_fwd_per_hypothesis": round(fwd / 1e9, 3), "gflop_step_per_hypothesis": round(step / 1e9, 3),
        "frac_f32_matrix_peak_hip": round(step * a.B / (ms_hip * 1e-3) / PEAK_F32_MATRIX, 4),
        "frac_f32_matrix_peak_torch": round(step * a.B / (ms_torch * 1e-3) / PEAK_F32_MATRIX, 4)}))


if __name__ == "__main__":
    main()
