"""GPU tests (pytest -m gpu) of the DTOID head's TRAINING path (Network._head_train_hip and the fused losses behind it) at
the finetune step's own shapes -- batch 8, image features [8, 640, 29, 39], template features [8, 640, 7, 7], decoder
29x39 -> 58x78 -> 116x156 -> 232x312 -> 480x640 -- against float64.

Pieces: train_ops.FusedConv forward and backward for every head layer shape (ELU epilogue, column sums, weight gradient,
data gradient with the up-sampling window sum and the prologue's (d scale, d shift) sums) in the form the dispatcher
picks and in the other one; BNFold forward / backward and the running statistics at every n of the head, with channels
whose mean is large against their spread; dw_xcorr; the two one-output-channel convolutions; the ELU epilogue itself;
the fused detection loss with inputs placed at known margins from every kink and clamp.
Whole head: every element of every output, loss, gradient and running buffer against tests/ref_dtoid_head.py after the
test has checked that every decision of the loss has a float64 margin above its tau; bit-equality of two runs, of side
streams on / off, of weight gradients on / off the side stream, and of self-packed against PackPlan-packed weights.

Bounds are max |got - float64| over the whole tensor relative to max |float64| of that tensor; the measured maximum is
noted beside each, every bound is at most 3x it."""
import ctypes

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import ref_dtoid_head as R
from oracle import dtoid_oracle
from ossid_code_amd import _lib
from ossid_code_amd.dtoid import ops
from ossid_code_amd.dtoid import train_ops as T
from ossid_code_amd.dtoid.loss import DetectionLoss, SegBceIou, _FusedDetectionLoss

pytestmark = pytest.mark.gpu

gen = R.gen
B = gen.B
GH, GW = gen.GRID


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


# ---- 1. FusedConv at every head layer shape -------------------------------------------------------------------------------
# name, cin, cout, source grid, output grid, prologue (folded BatchNorm in front), column sums, ELU, (fwd, dgrad) on Winograd
# at B = 8 as train_ops.wino_fits decides. Trunk conv2..conv4 of both trunks share one shape (and conv1 of both another).
LAYERS = [
    ("tmpl_c1", 640, 640, (7, 7), (7, 7), False, False, True, (False, False)),
    ("tmpl_c2", 640, 640, (5, 5), (5, 5), False, False, True, (False, False)),
    ("corr_conv_dot/sub/dot3x3", 640, 256, (GH, GW), (GH, GW), False, True, True, (True, True)),
    ("cf", 768, 512, (GH, GW), (GH, GW), True, True, True, (True, True)),
    ("trunk conv1", 512, 256, (GH, GW), (GH, GW), True, False, True, (True, True)),
    ("trunk conv2-4", 256, 256, (GH, GW), (GH, GW), False, False, True, (True, True)),
    ("cls output", 256, 48, (GH, GW), (GH, GW), False, False, False, (False, True)),
    ("reg output", 256, 96, (GH, GW), (GH, GW), False, False, False, (True, True)),
    ("s1", 512, 256, (GH, GW), (GH, GW), True, True, True, (True, True)),
    ("s2", 256, 128, (GH, GW), (58, 78), True, True, True, (False, True)),
    ("s3", 128, 64, (58, 78), (116, 156), True, True, True, (False, True)),
    ("s4", 64, 32, (116, 156), (232, 312), True, True, True, (False, True)),
    ("s5", 32, 16, (232, 312), (480, 640), True, True, True, (False, False)),
]


def _fewch_takes(cin, cout):
    """csrc/wgrad_fc.hip's own dispatch predicate (internal symbol of the library)."""
    f = getattr(_lib.lib(), "_Z23ossid_wgrad_fewch_takesiiiii")
    f.restype, f.argtypes = ctypes.c_bool, [ctypes.c_int] * 5
    return bool(f(cin, cout, 9, cin, cout))


def _up_index(n_src, n_dst):
    """The product's nearest index: min(floor(dst * (float)in / (float)out), in - 1), in float32."""
    scale = torch.tensor(n_src, dtype=torch.float32) / torch.tensor(n_dst, dtype=torch.float32)
    return torch.clamp(torch.floor(torch.arange(n_dst, dtype=torch.float32) * scale).long(), max=n_src - 1)


def _layer_inputs(cin, cout, src, dst, pre, stats, seed):
    g = torch.Generator().manual_seed(seed)
    x = F.elu(torch.randn(B, cin, *src, generator=g)) if pre else torch.randn(B, cin, *src, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    ps = (1.0 + 0.2 * torch.randn(cin, generator=g)) if pre else None
    pt = (0.1 * torch.randn(cin, generator=g)) if pre else None
    du = torch.randn(B, cout, *dst, generator=g)
    dsums = torch.zeros(3, cout)
    if stats:
        dsums[0] = 1e-3 * torch.randn(cout, generator=g)
        dsums[1] = 1e-3 * torch.randn(cout, generator=g)
    return x, w, b, ps, pt, du, dsums


def _layer_f64(x, w, b, ps, pt, du, dsums, dst, act, stats):
    x, w, b = (t.double().requires_grad_(True) for t in (x, w, b))
    leaves = [x, w, b]
    h = x
    if ps is not None:
        ps, pt = ps.double().requires_grad_(True), pt.double().requires_grad_(True)
        leaves += [ps, pt]
        h = x * ps.view(1, -1, 1, 1) + pt.view(1, -1, 1, 1)
    if tuple(dst) != tuple(x.shape[2:]):
        h = h[:, :, _up_index(x.shape[2], dst[0])][:, :, :, _up_index(x.shape[3], dst[1])]
    u = F.conv2d(h, w, b, padding=1)
    if act:
        u = F.elu(u)
    L = (du.double() * u).sum()
    if stats:
        L = L + (dsums[0].double().view(1, -1, 1, 1) * u).sum() + 0.5 * (dsums[1].double().view(1, -1, 1, 1) * u * u).sum()
    L.backward()
    ud = u.detach()
    return dict(u=ud, mean=ud.mean((0, 2, 3)), var=ud.var((0, 2, 3), unbiased=False), dx=x.grad, dw=w.grad, db=b.grad,
                dps=None if ps is None else ps.grad, dpt=None if pt is None else pt.grad)


def _layer_gpu(x, w, b, ps, pt, du, dsums, dst, act, stats):
    xg = cl(x).requires_grad_(True)
    wg, bg = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    psg = None if ps is None else ps.cuda().requires_grad_(True)
    ptg = None if pt is None else pt.cuda().requires_grad_(True)
    size = None if tuple(dst) == tuple(x.shape[2:]) else tuple(dst)
    res = T.FusedConv.apply(xg, wg, bg, psg, ptg, False, int(act), size, bool(stats))
    if stats:
        u, sums = res
        torch.autograd.backward([u, sums], [cl(du), dsums.cuda()])
        n = B * dst[0] * dst[1]
        s = sums.detach().double().cpu()
        mean = s[2] + s[0] / n
        var = s[1] / n - (s[0] / n) ** 2
    else:
        u = res
        u.backward(cl(du))
        mean = var = None
    torch.cuda.synchronize()
    return dict(u=u.detach(), mean=mean, var=var, dx=xg.grad, dw=wg.grad, db=bg.grad,
                dps=None if psg is None else psg.grad, dpt=None if ptg is None else ptg.grad)


def _dispatch(monkeypatch):
    seen = []
    real = T.conv_raw

    def spy(*a, **k):
        seen.append(bool(k.get("wino", False)))
        return real(*a, **k)
    monkeypatch.setattr(T, "conv_raw", spy)
    return seen


# measured maxima over every layer, both forms: u 8.6e-6, mean 2.1e-6, var 1.0e-6, dx 1.12e-5, dw 7.7e-6, db 5.0e-6,
# dps 1.13e-5, dpt 9.8e-6
LAYER_BOUND = dict(u=2.5e-5, mean=6e-6, var=3e-6, dx=3.3e-5, dw=2.3e-5, db=1.5e-5, dps=3.3e-5, dpt=2.9e-5)


@pytest.mark.parametrize("layer", LAYERS, ids=[l[0] for l in LAYERS])
def test_fused_conv_every_head_layer_against_float64(hiplib, layer, monkeypatch):
    """One launch set per layer shape in the dispatcher's own form, then the same with WINO_MIN_WGS forcing the other form
    (Winograd <-> direct) where the layer can take it. Both against one float64 restatement (prologue, the product's
    float32 nearest index, convolution, ELU, the column-sum gradient dv += dsums[1] * u + dsums[0])."""
    name, cin, cout, src, dst, pre, stats, act, (fwd_w, dgrad_w) = layer
    upsampled = tuple(src) != tuple(dst)
    assert T.wino_fits(B, dst[0], dst[1], cin, cout, 9, plain=not upsampled) == fwd_w
    assert T.wino_fits(B, dst[0], dst[1], cout, cin, 9) == dgrad_w
    # the decoder's two few-channel weight gradients run on csrc/wgrad_fc.hip, summing 8 x 480 x 640 pixels per tap for s5
    assert _fewch_takes(cin, cout) == (name in ("s4", "s5"))
    ins = _layer_inputs(cin, cout, src, dst, pre, stats, seed=cin * 7 + cout + dst[0])
    want = _layer_f64(*ins, dst, act, stats)
    forms = [None]
    if fwd_w or dgrad_w:
        forms.append(1 << 30)                            # everything direct
    elif cin % 16 == 0 and cout >= 64 and not upsampled or (cout % 16 == 0 and cin >= 64):
        forms.append(1)                                  # everything that can run on Winograd does
    for form in forms:
        if form is not None:
            monkeypatch.setattr(T, "WINO_MIN_WGS", form)
        seen = _dispatch(monkeypatch)
        got = _layer_gpu(*ins, dst, act, stats)
        if form is None:
            assert seen == [fwd_w, dgrad_w], (name, seen)
            again = _layer_gpu(*ins, dst, act, stats)
            for k in ("u", "dx", "dw", "db"):
                assert torch.equal(got[k], again[k]), k
        else:
            assert seen != [fwd_w, dgrad_w], (name, form, seen)
        monkeypatch.undo()
        for k, bound in LAYER_BOUND.items():
            if want.get(k) is None or (k in ("mean", "var") and not stats):
                continue
            assert got[k] is not None, k
            e = rel(got[k], want[k])
            print("MEASURE fused_conv %s form=%s %s %.3e" % (name, form, k, e))
            assert e < bound, (name, form, k, e)


# ---- 2. BNFold at every n of the head -----------------------------------------------------------------------------------------
BN_CASES = [(200, 640), (72, 640), (9048, 256), (9048, 512), (36192, 128), (144768, 64), (579072, 32), (2457600, 16)]


@pytest.mark.parametrize("n,C", BN_CASES)
def test_bn_fold_and_running_stats_against_float64(hiplib, n, C):
    """batch_stats (pivoted column sums) -> BNFold forward (scale, shift, running_mean / running_var with the UNBIASED
    variance) and backward (the sums' gradient in ColStats' dx = c1 + cx * x form, dgamma, dbeta). A quarter of the
    channels carry a mean 10^3 .. 10^4 times their spread, as ELU outputs in a saturated channel do. The variance is held
    per channel (relative to that channel's own variance), so those channels are not hidden by the others."""
    g = torch.Generator().manual_seed(n + C)
    mean = torch.randn(C, generator=g)
    spread = 0.5 + torch.rand(C, generator=g)
    tight = torch.arange(C) % 4 == 1
    mean[tight], spread[tight] = 3.0 + torch.rand(int(tight.sum()), generator=g), 1e-3
    x = (mean + spread * torch.randn(n, C, generator=g)).float()
    bn = nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * torch.randn(C, generator=g))
        bn.bias.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    rm0, rv0 = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    xg = x.cuda()
    sums = T.batch_stats(xg, n, C)
    gamma, beta = bn.weight.detach().clone().requires_grad_(True), bn.bias.detach().clone().requires_grad_(True)
    sums_l = sums.clone().requires_grad_(True)
    scale, shift = T.BNFold.apply(sums_l, gamma, beta, n, bn)
    gs, gsh = torch.randn(C, generator=g), torch.randn(C, generator=g)
    torch.autograd.backward([scale, shift], [gs.cuda(), gsh.cuda()])
    torch.cuda.synchronize()
    # float64
    x64 = x.double().requires_grad_(True)
    g64, b64 = bn.weight.detach().double().cpu().requires_grad_(True), bn.bias.detach().double().cpu().requires_grad_(True)
    mu, var = x64.mean(0), x64.var(0, unbiased=False)
    r = 1.0 / torch.sqrt(var + bn.eps)
    s64, t64 = g64 * r, b64 - mu * g64 * r
    ((gs.double() * s64).sum() + (gsh.double() * t64).sum()).backward()
    m = bn.momentum
    want_rm = (1 - m) * rm0 + m * mu.detach()
    want_rv = (1 - m) * rv0 + m * var.detach() * n / (n - 1)
    d = sums_l.grad.double().cpu()
    dx = d[0] + d[1] * x.double()                       # ColStats' convention
    errs = dict(scale=rel(scale, s64), shift=rel(shift, t64), dx=rel(dx[:, ~tight], x64.grad[:, ~tight]),
                dx_tight=rel(dx[:, tight], x64.grad[:, tight]), dgamma=rel(gamma.grad, g64.grad),
                dbeta=rel(beta.grad, b64.grad), running_mean=rel(bn.running_mean, want_rm),
                running_var=float(((bn.running_var.double().cpu() - want_rv) / want_rv).abs().max()))
    for k, e in errs.items():
        print("MEASURE bn n=%d C=%d %s %.3e" % (n, C, k, e))
    # measured maxima over every n: scale 4.5e-8, shift 8.3e-8, dgamma 9.1e-8, running_mean 5.6e-8, running_var 2.1e-7; dbeta is
    # g_shift itself. dx_tight: the channels whose mean is 3000x their spread -- dx = c1 + cx * x is a float32 cancellation
    # there (c1 ~ -cx * mean), 6e-8 * 3000 = 1.8e-4 of the gradient's size; measured 1.2e-4
    bounds = dict(scale=1.4e-7, shift=2.4e-7, dx=3e-6, dx_tight=3.5e-4, dgamma=2.7e-7, dbeta=1e-30, running_mean=1.6e-7,
                  running_var=6e-7)
    for k, e in errs.items():
        assert e < bounds[k], (n, C, k, e, bounds[k])
    # n versus n - 1: with momentum 1 the running variance IS the batch's unbiased variance, held per channel (measured
    # 1.6e-6, on a tight channel); where 1 / n is above the bound (n <= 144 768) a biased estimate fails
    bn.momentum = 1.0
    T.BNFold.apply(sums.clone(), gamma, beta, n, bn)
    torch.cuda.synchronize()
    want_u = var.detach() * n / (n - 1)
    e1 = float(((bn.running_var.double().cpu() - want_u) / want_u).abs().max())
    print("MEASURE bn n=%d C=%d running_var_m1 %.3e" % (n, C, e1))
    assert e1 < 4.8e-6, (n, C, e1)


# ---- 3. dw_xcorr ---------------------------------------------------------------------------------------------------------------
def test_dw_xcorr_at_the_head_shape_against_float64(hiplib):
    """ops.dw_xcorr(feat [8,640,29,39] channels-last, t2 [8,640,3,3]): forward and both gradients against the float64
    grouped convolution. Measured 1.5e-7 / 1.4e-7 / 1.1e-7."""
    g = torch.Generator().manual_seed(11)
    x, k, go = torch.randn(B, 640, GH, GW, generator=g), torch.randn(B, 640, 3, 3, generator=g), torch.randn(B, 640, GH, GW, generator=g)
    xg, kg = cl(x).requires_grad_(True), k.cuda().requires_grad_(True)
    y = ops.dw_xcorr(xg, kg)
    y.backward(go.cuda())
    x64, k64 = x.double().requires_grad_(True), k.double().requires_grad_(True)
    y64 = dtoid_oracle.dw_xcorr(x64, k64)
    y64.backward(go.double())
    errs = (rel(y, y64), rel(xg.grad, x64.grad), rel(kg.grad, k64.grad))
    print("MEASURE dw_xcorr %.3e %.3e %.3e" % errs)
    assert errs[0] < 4.5e-7 and errs[1] < 4e-7 and errs[2] < 3.3e-7, errs


# ---- 4. the one-output-channel convolutions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["heat 512->1 1x1", "seg_final 16->1 3x3"])
def test_one_output_channel_convs_at_the_head_shapes_against_float64(hiplib, which):
    """corr_conv_heatmap (conv1x1_c1, 512 -> 1 on [8, 29, 39]) and seg_final (conv3x3_c1, 16 -> 1 on [8, 480, 640]):
    forward, data, weight and bias gradient against float64 (measured 2.4e-7 at most); two runs bit-equal."""
    g = torch.Generator().manual_seed(12)
    cin, k, H, W = (512, 1, GH, GW) if which.startswith("heat") else (16, 3, 480, 640)
    conv = nn.Conv2d(cin, 1, k, padding=k // 2)
    x, go = torch.randn(B, cin, H, W, generator=g), torch.randn(B, 1, H, W, generator=g)
    fn = T.conv1x1_c1 if k == 1 else T.conv3x3_c1

    def run():
        cg = nn.Conv2d(cin, 1, k, padding=k // 2).cuda()
        cg.load_state_dict(conv.state_dict())
        xg = cl(x).requires_grad_(True)
        y = fn(xg, cg)
        y.backward(go.cuda())
        torch.cuda.synchronize()
        return y.detach(), xg.grad, cg.weight.grad, cg.bias.grad
    got, again = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    c64 = conv.double()
    x64 = x.double().requires_grad_(True)
    y64 = c64(x64)
    y64.backward(go.double())
    errs = [rel(a, b) for a, b in zip(got, (y64, x64.grad, c64.weight.grad, c64.bias.grad))]
    print("MEASURE c1 %s %s" % (which, " ".join("%.3e" % e for e in errs)))
    assert max(errs) < 7e-7, errs


# ---- 5. the ELU epilogue -------------------------------------------------------------------------------------------------
def _elu_sweep():
    x = torch.linspace(-30.0, 2.0, 40000)
    sw = torch.tensor(-0.35, dtype=torch.float32)
    near = [sw]
    for d in (1, -1):
        v = sw
        for _ in range(8):
            v = torch.nextafter(v, torch.tensor(d * 1.0))
            near.append(v)
    tiny = torch.tensor([-0.0, 0.0, -1e-45, 1e-45, -1e-40, 1e-40, -1.17e-38, -1e-30, -1e-7, -1e-3, -0.1, -0.3499, -0.3501,
                         -0.36, -1.0, -5.0, -16.0, -17.5, -88.0, -30.0, 1.0])
    x = torch.cat([x, torch.stack(near).float(), tiny])
    pad = (-x.numel()) % 16
    return torch.cat([x, torch.full((pad,), -0.5)])


def _ulp(y):
    a = y.abs().float()
    return (torch.nextafter(a, torch.tensor(float("inf"))) - a).double().clamp(min=2.0 ** -149)


@pytest.mark.parametrize("wino", [False, True])
def test_elu_epilogue_in_ulps_against_float64_expm1(hiplib, wino, monkeypatch):
    """The ELU epilogue (elu_fast, csrc/common.h) over x in [-30, 2], both sides of the -0.35 switch between the polynomial
    and __expf, -0.0 and subnormals. The same launch with act = 0 and act = 1: where the pre-activation is positive the two
    outputs are the same bits, elsewhere act = 1 must be within 4 ulps of the RESULT of float64 expm1(pre) (measured 1.66).
    Direct kernel: a 1x1 identity convolution of 16 channels (each output the sum of one exact product and zeros).
    Winograd: a 3x3 layer forced onto csrc/wino.hip. The backward's ELU' = u + 1 (chan_op mask_mode 2) on the same u
    against float64: two roundings (u + 1, then the product), within 2 ulps (measured 1.16)."""
    xs = _elu_sweep()
    C = 16
    if not wino:
        pix = xs.numel() // C
        x = xs.view(1, pix, 1, C).permute(0, 3, 1, 2)                  # [1, C, pix, 1]
        w = torch.eye(C).view(C, C, 1, 1)
        B_, H, W, cin, cout = 1, pix, 1, C, C
    else:
        monkeypatch.setattr(T, "WINO_MIN_WGS", 1)
        g = torch.Generator().manual_seed(13)
        cin, cout, H, W = 64, 64, 25, 25
        B_ = 1
        x = torch.randn(B_, cin, H, W, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) * (4.0 / (9 * cin)) ** 0.5
        assert T.wino_fits(B_, H, W, cin, cout, 9)
    xg, wg = cl(x), w.cuda().contiguous()
    outs = []
    with T.exact_forward(not wino):                   # direct: the three-way split, exact for a product with 1.0
        for act in (0, 1, 0):
            outs.append(T.FusedConv.apply(xg, wg, None, None, None, False, act, None, False).detach())
    torch.cuda.synchronize()
    pre, elu = outs[0].double().cpu(), outs[1].double().cpu()
    assert torch.equal(outs[0], outs[2])
    if not wino:                                      # the pre-activation is x (bar subnormals: the pieces may flush)
        xv = x.double()
        normal = (xv.abs() >= 1e-30) | (xv == 0)
        assert torch.equal(pre[normal], xv[normal])
    pos = pre > 0
    assert torch.equal(elu[pos], pre[pos])
    want = torch.where(pos, pre, torch.expm1(pre))
    ulps = float(((elu - want).abs() / _ulp(want)).max())
    print("MEASURE elu wino=%s max ulps %.2f" % (wino, ulps))
    assert ulps <= 4, ulps
    # backward factor: dv = du * (u > 0 ? 1 : u + 1)
    N = B_ * H * W
    u = outs[1]
    du = cl(torch.randn(u.shape, generator=torch.Generator().manual_seed(14)))
    dv = torch.empty_like(du)
    T.chan_op(du, N, cout, x=u, out=dv, mask_mode=2)
    torch.cuda.synchronize()
    u64 = u.double().cpu()
    want_dv = du.double().cpu() * torch.where(u64 > 0, torch.ones_like(u64), u64 + 1.0)
    e = float(((dv.double().cpu() - want_dv).abs() / _ulp(want_dv)).max())
    print("MEASURE elu_bwd wino=%s max ulps %.2f" % (wino, e))
    assert e <= 2, e


# ---- 6. the fused detection loss --------------------------------------------------------------------------------------------
def _placed_loss_inputs(net, margin):
    """cls / reg at the head's 27 144 anchors per image, B = 8, with every decision at least `margin` from its kink: p either
    side of the 1e-4 / 1 - 1e-4 clamps and between them, |t - reg| either side of 1/9 on the positives."""
    g = torch.Generator().manual_seed(15)
    ann = gen.seeded_inputs(gen.SEED + 10)[2]
    anc = R.anchors64(net)
    A = anc.shape[1]
    u = torch.rand(B, A, 2, generator=g, dtype=torch.float64)
    p = 10 ** (-3.999 + 3.5 * u)                                     # 1.0002e-4 .. 0.3
    side = torch.rand(B, A, 2, generator=g) < 0.02
    p = torch.where(side, 1e-4 * (1 + torch.where(torch.rand(B, A, 2, generator=g) < 0.5, -1.0, 1.0) * (2 * margin + 0.3 *
                                                                                                             torch.rand(B, A, 2, generator=g))), p)
    hi = torch.rand(B, A, 2, generator=g) < 0.01
    p = torch.where(hi, 1.0 - 1e-4 * (1 + torch.where(torch.rand(B, A, 2, generator=g) < 0.5, -1.0, 1.0) * 0.5), p)
    _, _, info = R.detection_loss(p, torch.zeros(B, A, 4, dtype=torch.float64), anc, ann.double())
    # the regression target of every anchor (the restatement's t): reg = t - sign * (1/9 +- d), d >= margin
    t = _targets(anc, ann.double())
    d = (margin + 0.05 * torch.rand(B, A, 4, generator=g, dtype=torch.float64)) * torch.where(
        torch.rand(B, A, 4, generator=g) < 0.5, -1.0, 1.0)
    sgn = torch.where(torch.rand(B, A, 4, generator=g) < 0.5, -1.0, 1.0)
    reg = t - sgn * (R.SL1_BETA + d)
    far = torch.rand(B, A, 4, generator=g) < 0.3                    # well inside the linear branch
    reg = torch.where(far, t - sgn * (0.5 + 2.0 * torch.rand(B, A, 4, generator=g, dtype=torch.float64)), reg)
    return p.float(), reg.float(), anc.float(), ann, info


def _targets(anc, ann):
    anchor = anc[0]
    aw, ah = anchor[:, 2] - anchor[:, 0], anchor[:, 3] - anchor[:, 1]
    acx, acy = anchor[:, 0] + 0.5 * aw, anchor[:, 1] + 0.5 * ah
    out = []
    for b in range(ann.shape[0]):
        gb = ann[b, 0]                                               # one box per image in this fixture
        gw, gh = gb[2] - gb[0], gb[3] - gb[1]
        gcx, gcy = gb[0] + 0.5 * gw, gb[1] + 0.5 * gh
        out.append(torch.stack([(gcx - acx) / aw / 0.1, (gcy - acy) / ah / 0.1, torch.log(gw.clamp(min=1) / aw) / 0.2,
                                torch.log(gh.clamp(min=1) / ah) / 0.2], 1))
    return torch.stack(out)


def test_fused_detection_loss_at_placed_margins_against_float64(hiplib):
    """ossid_focal_smoothl1_loss_{fwd,bwd} on 27 144 anchors x 8 images against the float64 restatement, with inputs placed
    at least 1e-4 (relative: p; absolute: |t - reg|) from every clamp and kink, and both losses weighted. The assignment
    is the restatement's exactly (positives: the anchors whose regression gradient is non-zero; counted: whose class
    gradient is). Measured: losses 4.4e-10 / 2.3e-8, class gradient 4.3e-8, regression gradient 1.1e-5 of scale."""
    net = R.build_head()[0]
    margin = 1e-4
    p, reg, anc, ann, _ = _placed_loss_inputs(net, margin)
    p64, r64 = p.double().requires_grad_(True), reg.double().requires_grad_(True)
    lc64, lr64, info = R.detection_loss(p64, r64, anc.double(), ann.double())
    mg = R.min_margins(info)
    assert float(info["margins"]["smooth_l1"].min()) >= margin * 0.99, mg
    rel_clamp = torch.min((p.double() / R.P_LO - 1).abs(), ((1 - p.double()) / R.P_LO - 1).abs())
    assert float(rel_clamp.min()) >= margin, float(rel_clamp.min())
    assert float(info["margins"]["iou"].min()) > 1e-5, mg
    (0.7 * lc64 + 1.3 * lr64).sum().backward()
    pg, rg = p.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    lc, lr = DetectionLoss()(pg, rg, anc.cuda(), ann.cuda())
    (0.7 * lc + 1.3 * lr).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal((rg.grad != 0).any(-1).cpu(), info["positive"])
    assert torch.equal((pg.grad != 0).cpu(), p64.grad != 0)
    errs = (rel(lc, lc64), rel(lr, lr64), rel(pg.grad, p64.grad), rel(rg.grad, r64.grad))
    print("MEASURE det_loss %s" % " ".join("%.3e" % e for e in errs))
    # the regression gradient's error is the kernel's float32 box targets (t = log(g / a) / 0.2 etc., ~1e-6 absolute) times
    # 9 in the quadratic branch
    assert errs[0] < 1.3e-9 and errs[1] < 7e-8 and errs[2] < 1.3e-7 and errs[3] < 3.4e-5, errs
    # the same launch twice: the same bits
    pg2, rg2 = p.cuda().requires_grad_(True), reg.cuda().requires_grad_(True)
    lc2, lr2 = _FusedDetectionLoss.apply(pg2, rg2, anc.cuda(), ann.cuda(), 0.25, 2.0)
    (0.7 * lc2 + 1.3 * lr2).sum().backward()
    assert torch.equal(lc2, lc) and torch.equal(lr2, lr) and torch.equal(pg2.grad, pg.grad) and torch.equal(rg2.grad, rg.grad)


# ---- whole head ----------------------------------------------------------------------------------------------------------------
HEAT_GAP = 1e-4
TAU = dict(iou=1e-5, smooth_l1=1e-4, p_clamp=1e-6, seg_logit=1.0, heat_l1=HEAT_GAP)


@pytest.fixture(scope="module")
def head64():
    """Inputs of the fixture (heat-map target moved HEAT_GAP clear of the float64 heat map) and the float64 restatement."""
    net = R.build_head()[0]
    ins = list(gen.seeded_inputs(gen.SEED + 10))
    out = R.reference(net, *ins, heat_gap=HEAT_GAP)
    ins[3] = out["heat_t"]
    return ins, out


def _head_net():
    net = R.build_head()[0]
    return net.cuda().train()


def _head_product(net, ins):
    feat, tmpl, ann, heat_t, mask_t = (t.cuda() for t in ins)
    f, t = feat.clone().requires_grad_(True), tmpl.clone().requires_grad_(True)
    c, r, anc, heat, seg = net._head_train_hip(f.view_as(f), t.view_as(t))
    c.retain_grad()
    r.retain_grad()
    lc, lr = DetectionLoss()(c, r, anc, ann)
    l_center = nn.L1Loss()(heat_t, heat)
    _, l_seg, _ = SegBceIou.apply(seg, mask_t)
    (20 * l_seg + 20 * l_center + lc + lr).sum().backward()
    torch.cuda.synchronize()
    out = dict(cls=c.detach(), reg=r.detach(), heat=heat.detach(), seg=seg.detach(), loss_cls=lc.detach(), loss_reg=lr.detach(),
               loss_center=l_center.detach(), loss_seg=l_seg.detach(), grad_feat=f.grad, grad_tmpl=t.grad,
               grad_cls=c.grad, grad_reg=r.grad)
    for prefix, m in (("corr", net.correlation_model), ("cls", net.classification), ("reg", net.regression)):
        for name, p in m.named_parameters():
            out["g.%s.%s" % (prefix, name)] = p.grad
        for name, b in m.named_buffers():
            out["b.%s.%s" % (prefix, name)] = b.detach().clone()
    T.end_step()
    return out


# Bounds of the whole head, max |got - float64| / max |float64| per tensor, per group. Measured maxima: outputs 2.2e-5 (seg),
# losses 1.8e-7, feat / tmpl gradients 2.0e-5, weight gradients 3.7e-5 (reg.conv1), bias and BatchNorm-parameter gradients
# 3.7e-5 (corr_conv_dot.bias), running buffers 6.5e-7. Every tensor is held to its own scale: no bias gradient here is a
# near-cancellation that needs its layer's weight-gradient scale instead.
HEAD_BOUND = dict(out=6e-5, loss=5e-7, grad_input=6e-5, grad_w=1.1e-4, grad_vec=1.1e-4, buffer=1.9e-6)


def _group(k, v):
    if k.startswith("loss_"):
        return "loss"
    if k in ("grad_feat", "grad_tmpl"):
        return "grad_input"
    if k.startswith("g."):
        return "grad_w" if v.dim() == 4 else "grad_vec"
    if k.startswith("b."):
        return "buffer"
    return "out"


def test_whole_head_every_element_against_float64(hiplib, head64):
    """_head_train_hip + DetectionLoss + SegBceIou + L1 + backward at B = 8 with the product dispatch (no threshold
    overridden). First: every decision of the loss has a float64 margin above its tau, and the product's own error on the
    decided quantity is below that tau; the anchor assignment is the restatement's. Then every element of cls, reg, heat,
    the full 480x640 segmentation, the four losses, feat.grad, tmpl.grad, every parameter gradient and every running
    buffer, against the float64 restatement; num_batches_tracked incremented exactly once."""
    ins, want = head64
    mg = R.min_margins(want["info"])
    for k, tau in TAU.items():
        assert mg[k] > tau, (k, mg[k], tau)
    assert T.wino_fits(B, GH, GW, 768, 512, 9) and T.wino_fits(B, GH, GW, 256, 256, 9)
    net = _head_net()
    got = _head_product(net, ins)
    # decisions: the product's error on what is decided is below the margin every decision has
    assert float((got["reg"].double().cpu() - want["reg"]).abs().max()) < TAU["smooth_l1"]
    assert float((got["heat"].double().cpu() - want["heat"]).abs().max()) < TAU["heat_l1"]
    assert torch.equal((got["grad_reg"] != 0).any(-1).cpu(), want["info"]["positive"])
    assert torch.equal((got["grad_cls"] != 0).cpu(), want["grad_cls"] != 0)
    worst = {}
    bad = []
    for k, v in want.items():
        if k in ("info", "heat_t", "x2", "grad_cls", "grad_reg"):
            continue
        g = got[k]
        if k.endswith("num_batches_tracked"):
            assert int(g) == int(v) == 1, (k, int(g))
            continue
        grp = _group(k, v)
        e = float((g.double().cpu() - v).abs().max()) / max(float(v.abs().max()), 1e-30)
        print("MEASURE head %s %s %.3e" % (grp, k, e))
        worst[grp] = max(worst.get(grp, 0.0), e)
        if e >= HEAD_BOUND[grp]:
            bad.append((k, grp, "%.2e" % e))
    print("MEASURE head worst %s" % worst)
    assert not bad, bad


def _bits_equal(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


# use_train_streams on / off: the same kernels on the same operands, but a tensor read by several branches (feat: by
# corr_conv_dot, corr_conv_sub and dw_xcorr; u2 and its BatchNorm fold: by both trunks, the heat map and s1) gets its
# gradient contributions summed by autograd in the order its consumers' nodes run, and the forks create those nodes in
# another order than the serial path. Only the gradients upstream of u2 differ (26 tensors: feat, tmpl and the correlation
# layers' parameters); every output, loss, running buffer and every trunk / decoder gradient is the same bits. Float32
# reordering of a few-term sum, amplified by the training BatchNorms' backward on channels whose spread is small against
# their mean (saturated ELU outputs): measured 1.8e-5 of scale at most, below the distance of either path from float64.
STREAMS_REORDER_BOUND = 5.5e-5


def test_whole_head_is_deterministic_across_streams_wgrad_side_and_packing(hiplib, head64, monkeypatch):
    """Two runs bit-equal; train_ops.WGRAD_SIDE on / off bit-equal; weights packed by the step's PackPlan (second step on:
    the plan has learned the layouts the decoder asked for through plan.misses) bit-equal to self-packed weights.
    use_train_streams on / off: equal up to float32 reordering of multi-consumer gradient sums (STREAMS_REORDER_BOUND)."""
    ins, _ = head64
    base = _head_product(_head_net(), ins)
    found = {"again": _bits_equal(base, _head_product(_head_net(), ins))}
    monkeypatch.setattr(T, "WGRAD_SIDE", False)
    found["wgrad_side_off"] = _bits_equal(base, _head_product(_head_net(), ins))
    monkeypatch.undo()
    # PackPlan: step 1 packs through the plan and records what the head packed by itself; step 2 runs on the learned plan
    net = _head_net()
    state = {k: v.clone() for k, v in net.state_dict().items()}
    net._train_pack_plan().run()
    _head_product(net, ins)
    net.load_state_dict(state)
    for p in net.parameters():
        p.grad = None
    plan = net._train_pack_plan()
    assert not plan.misses
    plan.run()
    found["pack_plan"] = _bits_equal(base, _head_product(net, ins))
    assert not plan.misses, plan.misses                  # the learned plan foresaw every layout the head asked for
    net = _head_net()
    net.use_train_streams = False
    serial = _head_product(net, ins)
    diff = {k: rel(serial[k], base[k]) for k in _bits_equal(base, serial)}
    print("MEASURE streams_off differs in %d tensors, max %.3e: %s" % (len(diff), max(diff.values(), default=0.0), sorted(diff)))
    print("MEASURE determinism %s" % found)
    assert all(not v for v in found.values()), found
    assert max(diff.values(), default=0.0) < STREAMS_REORDER_BOUND, diff
    # the forward values themselves do not depend on the streams: only gradients are reordered
    assert not any(k in diff for k in ("cls", "reg", "heat", "seg", "loss_cls", "loss_reg", "loss_center", "loss_seg"))
