"""CPU anchor of the float64 head restatement (tests/ref_dtoid_head.py): held to the reference's own float32 run at the
finetune step's real sizes (tests/golden/dtoid_head_train_full.npz) within the float32 noise that
test_dtoid_train_full_fixture.py::test_module_path_matches_full_size_training_fixture already allows. This pins the
restatement -- modules, the four-term loss restated in float64, the anchor assignment -- to the reference's semantics, so
the GPU tests can hold the product to it elementwise (tests/test_head_train_gpu.py)."""
import os

import numpy as np
import pytest
import torch

import ref_dtoid_head as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.load(os.path.join(ROOT, "tests", "golden", "dtoid_head_train_full.npz"))


@pytest.fixture(scope="module")
def ref():
    """One float64 forward + backward at B = 8 (~15 s on 8 CPUs)."""
    assert int(F["batch"]) == R.gen.B and int(F["seed"]) == R.gen.SEED
    net = R.build_head()[0]
    return net, R.reference(net, *R.gen.seeded_inputs(R.gen.SEED + 10))


def test_ref_dtoid_head_matches_full_size_reference_fixture(ref):
    """rtol 2e-4 / atol 2e-5 elementwise and 2e-4 of each tensor's scale: the bounds of the module-path fixture test (the
    golden itself is float32). Measured: 1.3e-4 of scale at most (g.corr.s5.bias, a sum over 2.46 M float32 terms in the
    golden), 1e-5 or less on every output and loss."""
    _, out = ref
    got = R.sampled(out)
    stored = [k for k in F.files if k not in ("seed", "batch")]
    bad = []
    for k in stored:
        want = F[k].astype(np.float64)
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        err = float(np.abs(got[k] - want).max())
        scale = max(float(np.abs(want).max()), 1e-12)
        if not np.allclose(got[k], want, rtol=2e-4, atol=2e-5) or err > 2e-4 * scale:
            bad.append((k, "%.2e of scale %.2e" % (err / scale, scale)))
    assert not bad, bad
    # every parameter has a gradient and every running statistic was stored: nothing of the head went unchecked
    assert sorted(k for k in got if k.startswith(("g.", "b."))) == sorted(k for k in stored if k.startswith(("g.", "b.")))


def test_ref_dtoid_head_assignment_and_margins(ref):
    """The restated anchor assignment is the repo's tensor-form DetectionLoss' (same positives, same losses to 1e-12 in
    float64), every sample has positives, and the margins are finite and cover every decision of the loss."""
    from ossid_code_amd import dtoid
    net, out = ref
    info = out["info"]
    assert bool((info["npos"] > 0).all())
    lc, lr = dtoid.DetectionLoss()(out["cls"], out["reg"], R.anchors64(net), R.gen.seeded_inputs(R.gen.SEED + 10)[2].double())
    assert abs(float(lc) - float(out["loss_cls"])) <= 1e-12 * abs(float(lc))
    assert abs(float(lr) - float(out["loss_reg"])) <= 1e-12 * abs(float(lr))
    m = info["margins"]
    assert m["smooth_l1"].numel() == 4 * int(info["npos"].sum())
    assert m["p_clamp"].numel() == 2 * int(info["counted"].sum())
    assert m["seg_logit"].numel() == out["seg"].numel() and m["heat_l1"].numel() == out["heat"].numel()
    assert all(bool(torch.isfinite(v).all()) for v in m.values())
