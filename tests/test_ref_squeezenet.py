"""CPU tests of tests/ref_squeezenet.py, the float64 restatement the template-encoder training node is held to: with its own
decisions it is the nn.Module in float64, and decisions handed to it are followed."""
import copy

import pytest
import torch

import ref_squeezenet as R
from ossid_code_amd.dtoid import network


def _encoder(which, seed):
    torch.manual_seed(seed)
    mod = (network.TemplateFeatExtract() if which == "local" else network.TemplateFeatExtractGlobal()).double().train()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1, 0.2)
                m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
            elif isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                m.bias.normal_(0, 0.1)
    return mod


@pytest.mark.parametrize("which", ["local", "global"])
def test_restatement_equals_the_module_in_float64(which):
    mod = _encoder(which, 3)
    g = torch.Generator().manual_seed(11)
    img = torch.rand(2, 4, 124, 124, generator=g, dtype=torch.float64)
    ref = copy.deepcopy(mod)
    y = ref(img)
    gout = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gout)
    y = y.detach()
    got = R.encoder_train(mod, img, gout)
    scale = lambda t: float(t.abs().max())      # noqa: E731
    assert got["out"].shape == y.shape == ((2, 640, 7, 7) if which == "local" else (2, 64, 3, 3))
    assert float((got["out"] - y).abs().max()) <= 1e-12 * scale(y)
    n_used = 0
    for n, p in ref.named_parameters():
        if p.grad is None:
            assert n not in got["grads"], n                # the classifier / 3-channel stem of mod.backbone never run
            continue
        n_used += 1
        assert float((got["grads"][n] - p.grad).abs().max()) <= 1e-12 * scale(p.grad), n
    assert n_used == len(got["grads"]) == (54 if which == "local" else 62)
    for n, b in ref.named_buffers():
        if b.dtype.is_floating_point:
            assert float((got["running"][n] - b).abs().max()) <= 1e-12 * scale(b), n
    # every decision came back with a margin and a scale: stem + 8 Fire modules x 2 ReLU masks, 3 max-pools
    assert sorted(got["margin"]) == sorted(got["decisions"]) and len(got["decisions"]) == 1 + 16 + 3
    assert got["decisions"]["backbone_2.3"].shape == (2, 256, 7, 7)


def test_restatement_follows_its_own_decisions_bit_for_bit():
    mod = _encoder("global", 5)
    g = torch.Generator().manual_seed(2)
    img = torch.rand(2, 4, 124, 124, generator=g, dtype=torch.float64)
    gout = torch.randn(2, 64, 3, 3, generator=g, dtype=torch.float64)
    a = R.encoder_train(mod, img, gout)
    b = R.encoder_train(mod, img, gout, decisions=a["decisions"])
    assert torch.equal(a["out"], b["out"])
    assert a["grads"].keys() == b["grads"].keys() and all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])
    assert all(torch.equal(a["running"][n], b["running"][n]) for n in a["running"])


def test_a_changed_argmax_moves_the_gradient_to_the_other_input_position():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 30, 30, generator=g, dtype=torch.float64)
    go = torch.randn(2, 4, 15, 15, generator=g, dtype=torch.float64)
    xa = x.clone().requires_grad_(True)
    ya, _, own, margin = R.maxpool(xa, 3, 2, 0, True)
    ya.backward(go)
    xr = x.clone().requires_grad_(True)
    yr = torch.nn.functional.max_pool2d(xr, 3, 2, 0, ceil_mode=True)
    yr.backward(go)
    assert torch.equal(ya, yr) and float((xa.grad - xr.grad).abs().max()) <= 1e-12 and bool((margin > 0).all())
    # window (b 1, c 2, row 14 -- the partial last one, rows 28..29 -- column 5) chooses another element of its window
    b, c, yo, xo = 1, 2, 14, 5
    a0 = int(own[b, c, yo, xo])
    a1 = next(p for p in range(6) if p != a0)              # (positions 6..8 lie below the input)
    am = own.clone()
    am[b, c, yo, xo] = a1
    xb = x.clone().requires_grad_(True)
    yb, used, _, _ = R.maxpool(xb, 3, 2, 0, True, argmax=am)
    yb.backward(go)
    pos = lambda p: (yo * 2 + p // 3, xo * 2 + p % 3)      # noqa: E731
    (r0, c0), (r1, c1) = pos(a0), pos(a1)
    assert float(yb.detach()[b, c, yo, xo]) == float(x[b, c, r1, c1])
    d = xb.grad - xa.grad
    gv = float(go[b, c, yo, xo])
    assert abs(float(d[b, c, r1, c1]) - gv) <= 1e-12 and abs(float(d[b, c, r0, c0]) + gv) <= 1e-12
    d[b, c, r1, c1] = d[b, c, r0, c0] = 0
    assert float(d.abs().max()) == 0.0                      # nothing else moved
    # and through a whole encoder: the changed decision changes the gradients in front of that pool
    mod = _encoder("local", 9)
    img = torch.rand(2, 4, 124, 124, generator=g, dtype=torch.float64)
    gout = torch.randn(2, 640, 7, 7, generator=g, dtype=torch.float64)
    base = R.encoder_train(mod, img, gout)
    dec = dict(base["decisions"])
    am = dec["backbone_2.0"].clone()
    am[0, 0, 3, 3] = (int(am[0, 0, 3, 3]) + 1) % 9
    dec["backbone_2.0"] = am
    moved = R.encoder_train(mod, img, gout, decisions=dec)
    assert not torch.equal(moved["grads"]["backbone_0.0.weight"], base["grads"]["backbone_0.0.weight"])
    assert torch.equal(moved["grads"]["norm_1.weight"], base["grads"]["norm_1.weight"])      # behind the pool: untouched
