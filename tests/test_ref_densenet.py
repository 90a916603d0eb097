"""tests/ref_densenet.py against torch autograd of the module itself, in float64 on the CPU: with free decisions the
restatement IS ImageFeatExtract(...).double().train(); imposing its own decisions changes nothing; imposing another one does."""
import copy

import pytest
import torch

import backbone_train_cases as bc
import ref_densenet as rd
from ossid_code_amd.dtoid import ops

B, H, W = 2, 38, 54


def _close(name, a, b, tol=1e-10):
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= tol * max(scale, 1e-300), (name, err, scale)


@pytest.mark.parametrize("Bx,kb", [(2, 2), (3, 1), (1, 1)])
def test_dw_xcorr_is_the_per_channel_cross_correlation(Bx, kb):
    """rd.dw_xcorr stands in for the device kernel in the module comparison below, so it is pinned by itself: explicit
    float64 loops over a 2-channel 3 x 4 map, k per image and k shared by the batch (whose gradient is the sum over it)."""
    gen = torch.Generator().manual_seed(Bx + kb)
    C, H, W = 2, 3, 4
    x = torch.randn(Bx, C, H, W, generator=gen, dtype=torch.float64)
    k = torch.randn(kb, C, 3, 3, generator=gen, dtype=torch.float64).requires_grad_(True)
    go = torch.randn(Bx, C, H, W, generator=gen, dtype=torch.float64)
    out = rd.dw_xcorr(x, k)
    out.backward(go)
    want, dk = torch.zeros(Bx, C, H, W, dtype=torch.float64), torch.zeros(kb, C, 3, 3, dtype=torch.float64)
    for b in range(Bx):
        for c in range(C):
            for y in range(H):
                for xx in range(W):
                    for dy in range(3):
                        for dx in range(3):
                            yy, xs = y + dy - 1, xx + dx - 1
                            if 0 <= yy < H and 0 <= xs < W:
                                want[b, c, y, xx] += float(k.detach()[b % kb, c, dy, dx]) * x[b, c, yy, xs]
                                dk[b % kb, c, dy, dx] += go[b, c, y, xx] * x[b, c, yy, xs]
    assert float((out.detach() - want).abs().max()) < 1e-13 and float((k.grad - dk).abs().max()) < 1e-13


@pytest.fixture(scope="module")
def setup():
    ife = bc.make_backbone(5)
    gen = torch.Generator().manual_seed(6)
    image = torch.randn(B, 3, H, W, generator=gen)
    h, w = bc.maps(H, W)[-1]
    gout = torch.randn(B, 640, h, w, generator=gen)
    gs = {gb: 0.3 * torch.randn(gb, 64, 3, 3, generator=gen) for gb in (B, 1)}
    res = {gb: rd.backbone_train(ife, image, g, gout) for gb, g in gs.items()}
    return ife, image, gout, gs, res


@pytest.mark.parametrize("gb", [B, 1], ids=["g-per-image", "g-shared"])
def test_free_decisions_equal_torch_autograd_of_the_module(setup, monkeypatch, gb):
    """Output, all 366 parameter gradients, the gradient with respect to g and the 244 running statistics, each to 1e-10 of
    its own scale. (ops.dw_xcorr is a device kernel; the module runs here with the plain grouped convolution in its place.)"""
    ife, image, gout, gs, res = setup
    monkeypatch.setattr(ops, "dw_xcorr", lambda x, k: rd.dw_xcorr(x, k))
    mod = copy.deepcopy(ife).double().train()
    g = gs[gb].double().requires_grad_(True)
    out = mod(image.double(), g)
    out.backward(gout.double())
    r = res[gb]
    _close("out", r["out"], out.detach())
    names = [n for n, _ in mod.named_parameters()]
    assert len(names) == 366 and set(r["grads"]) == set(names) | {"g"}
    for n, p in mod.named_parameters():
        _close(n, r["grads"][n], p.grad)
    assert r["grads"]["g"].shape == g.shape
    _close("g", r["grads"]["g"], g.grad)
    bufs = {n: b for n, b in mod.named_buffers() if b.dtype.is_floating_point}
    assert len(bufs) == 244 and set(r["running"]) == set(bufs)
    for n, b in bufs.items():
        _close(n, r["running"][n], b)
        assert not torch.equal(b, ife.get_buffer(n).double())                 # (they moved)
    assert list(r["decisions"]) == rd.decision_names() and len(r["decisions"]) == 2 + 2 * 58 + 3
    for n in r["decisions"]:
        assert r["margin"][n].shape == r["decisions"][n].shape and r["scale"][n] > 0
        assert r["pre"][n].shape[:2] == r["decisions"][n].shape[:2]


def test_imposing_its_own_decisions_changes_nothing(setup):
    ife, image, gout, gs, res = setup
    r = res[B]
    again = rd.backbone_train(ife, image, gs[B], gout, decisions=r["decisions"])
    assert torch.equal(again["out"], r["out"])
    for n, gr in r["grads"].items():
        assert torch.equal(again["grads"][n], gr), n
    for n, b in r["running"].items():
        assert torch.equal(again["running"][n], b), n


@pytest.mark.parametrize("name", ["norm0", "denseblock2.denselayer5.norm2", "transition3.norm"])
def test_one_flipped_relu_element_changes_the_gradients(setup, name):
    ife, image, gout, gs, res = setup
    r = res[B]
    flipped = r["decisions"][name].clone()
    # the element that was on by the widest margin: switching it off is no rounding matter (every other decision is left free)
    on = torch.where(flipped.reshape(-1), r["margin"][name].reshape(-1), torch.zeros(()).double())
    flipped.view(-1)[int(on.argmax())] = False
    other = rd.backbone_train(ife, image, gs[B], gout, decisions={name: flipped})
    conv0 = "backdense_0.0.weight"
    assert not torch.equal(other["grads"][conv0], r["grads"][conv0])
    assert float((other["grads"][conv0] - r["grads"][conv0]).abs().max()) > 1e-8 * float(r["grads"][conv0].abs().max())
    assert torch.equal(other["decisions"][name], r["decisions"][name])         # `decisions` reports the pass's own


def test_float32_runs_the_same_code_on_the_same_decisions(setup):
    """dtype=torch.float32: every tensor of the pass is float32, the imposed decisions are followed (the pass's own may
    differ), the result is finite and is not the float64 one. Its distance from float64 is the yardstick of the GPU tests;
    printed here, not bounded: it depends on the batch statistics' conditioning (four samples per channel in n1 here)."""
    ife, image, gout, gs, res = setup
    r = res[B]
    r32 = rd.backbone_train(ife, image, gs[B], gout, decisions=r["decisions"], dtype=torch.float32)
    assert r32["out"].dtype == torch.float32 and all(v.dtype == torch.float32 for v in r32["running"].values())
    worst = ("", 0.0)
    for n, gr in r["grads"].items():
        g32 = r32["grads"][n]
        assert g32.dtype == torch.float32 and bool(torch.isfinite(g32).all()), n
        e = float((g32.double() - gr).abs().max() / gr.abs().max())
        worst = max(worst, (n, e), key=lambda t: t[1])
    print("float32 restatement vs float64, worst gradient: %.3e (%s)" % (worst[1], worst[0]))
    assert worst[1] > 0
