"""GPU tests (pytest -m gpu) of the fused dense-block training kernels (csrc/dense_bwd.hip) and of the grouped 1x1 weight
gradient's dy_add staging (csrc/wgrad_t9.hip), each called directly through the helpers of ossid_code_amd/dtoid/train_ops.py
and compared with a plain float64 restatement of the same operation on the CPU, at the four DenseNet-121 blocks' production
shapes (first and last layer of each: blocks 1 and 2 at a pixel count that makes the persistent workgroups walk several
stages, blocks 3 and 4 up to 31 channel tiles and Ct = 1024), at ragged small shapes and at the channel limits.

Every input is drawn away from the ReLU kink (|s x + t| >= 1e-2), so the float32 mask the kernels compute and the float64
mask are the same: the bounds below are hard in every case. Error model: the forward is the three-way bf16 split
(f32-level, 5e-6 of the output scale), the data gradients are split-bf16 (three products, 2e-5), column sums and weight
gradients are f32 sums of those products (5e-5). Every kernel is deterministic by design (fixed-order partial rows, no
float atomics): a second run on the same inputs must reproduce every bit. The measured maximum error of each check is noted
beside its bound."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

from ossid_code_amd import _lib
from ossid_code_amd.dtoid import backbones
from ossid_code_amd.dtoid import train_ops as T

pytestmark = pytest.mark.gpu

MID, EINVAL = 128, -22
EPS, MOM = 1e-5, 0.1


@pytest.fixture(autouse=True)
def _split_bf16_build(hiplib):
    # the fused dense kernels exist on the split-bf16 build only (the all-exact build returns EINVAL from all of them)
    if not hiplib.lib().ossid_conv_split_bf16():
        pytest.skip("the fused dense-block kernels are built only with the split-bf16 convolutions")


def rel(a, b):
    """max |a - b| relative to max |b|."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def bound(name, err, tol):
    print("%-28s %.3e  (bound %.0e)" % (name, err, tol))
    assert err < tol, (name, err, tol)


def away(n, c, g, lo=0.02):
    """x [n, c] and per-channel (s, t), float32, with |s x + t| >= 1e-2 everywhere in float64: about half the entries on
    each side of the ReLU, none near its kink."""
    s = (0.5 + torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    t = 0.5 * torch.randn(c, generator=g)
    z = (lo + torch.randn(n, c, generator=g).abs()) * torch.where(torch.rand(n, c, generator=g) < 0.5, -1.0, 1.0)
    x = (z - t) / s
    assert float((x.double() * s.double() + t.double()).abs().min()) >= 1e-2
    return x, s, t


def relu_mask(x, s, t):
    return (x.double() * s.double() + t.double() > 0).double()


def fold_bwd64(S0, S1, gamma, mean, rstd, n):
    """ossid_bn_fold_bwd restated: BatchNorm's backward from d shift = S0, d scale = S1 (scale = gamma rstd, shift = beta -
    mean scale) -> (d gamma, d beta, coef_x, coef_1) with dx = coef_x x + coef_1 from the statistics."""
    g, mu, r = gamma.double(), mean.double(), rstd.double()
    ds = S1 - S0 * mu
    dmean, dvar = -S0 * g * r, -0.5 * ds * g * r ** 3
    return ds * r, S0, 2.0 * dvar / n, dmean / n - 2.0 * mu * dvar / n


def fold_args(C, g):
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    mean, rstd = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    return gamma, beta, mean, rstd


def run_bn_fold_bwd(partials, gamma, mean, rstd, C, n, coef0):
    """(d gamma, d beta, coef_x, coef_1) from partial rows; coef_x / coef_1 accumulate onto coef0 as _dense_backward does."""
    r = torch.empty(2, C, device="cuda")
    coef = coef0.cuda().clone()
    T.bn_fold_bwd(None, None, gamma.cuda(), mean.cuda(), rstd.cuda(), C, n, r[0], r[1], coef[0], coef[1], accumulate=True,
                  partials=partials)
    return torch.cat([r, coef]).clone()


def fn(name):
    return _lib.fn(name)


# (B, H, W, c, Ct): the first and last dense layer of each DenseNet-121 block at finetune batch sizes (block 1 at batch 2, so
# that blocks 1 and 2 both have N = 38 400: 600 stages of 64 pixels, 1 200 tiles of 4 x 8, more than the persistent grid);
# blocks 3 and 4 reach 31 channel tiles (8 per wave) at Ct = 1024, block 4's 29 x 39 is ragged against the tiles and stages
PROD = [
    pytest.param(2, 120, 160, 64, 256, id="block1-first"), pytest.param(2, 120, 160, 224, 256, id="block1-last"),
    pytest.param(8, 60, 80, 128, 512, id="block2-first"), pytest.param(8, 60, 80, 480, 512, id="block2-last"),
    pytest.param(8, 30, 40, 256, 1024, id="block3-first"), pytest.param(8, 30, 40, 992, 1024, id="block3-last"),
    pytest.param(8, 29, 39, 512, 1024, id="block4-first"), pytest.param(8, 29, 39, 992, 1024, id="block4-last"),
]
# ragged and limit cases: N = 1, 63, 65, 1 x 1 images, 3 x 5, three 5 x 9 images (tiles and stages across image boundaries),
# c = 32 and c = 1024
SMALL = [
    pytest.param(1, 1, 1, 32, 64, id="N1"), pytest.param(1, 7, 9, 64, 96, id="N63"), pytest.param(1, 5, 13, 96, 128, id="N65"),
    pytest.param(5, 1, 1, 128, 160, id="1x1"), pytest.param(2, 3, 5, 160, 192, id="3x5"), pytest.param(3, 5, 9, 224, 256, id="B3-5x9"),
    pytest.param(2, 9, 11, 32, 32, id="c32"), pytest.param(1, 30, 40, 1024, 1024, id="c1024"),
]


def walks(N):
    """Blocks 1 and 2 at production N: the persistent grids are smaller than the work, and the forward runs PT = 2."""
    return N >= 38400


# ---- forward: y1 = W1 relu(s1 x + t1) with norm2's statistics as pivoted partial rows ------------------------------------
def _fwd1(x_full, w1, ps, pt, N, c, Ct, gamma, beta, rm, rv):
    bufd, w1d = x_full.cuda(), w1.cuda()
    y1 = torch.full((N, MID), float("nan"), device="cuda")
    rows = T.dense_fwd1_stats(bufd, T._pack(w1d, "fwd_x6"), y1, N, c, Ct, ps.cuda(), pt.cuda())
    rmd, rvd = rm.cuda(), rv.cuda()
    out = T.bn_fold_fwd_rows(rows, MID, N, gamma.cuda(), beta.cuda(), EPS, MOM, rmd, rvd)
    torch.cuda.synchronize()
    return y1.clone(), torch.cat([out, rmd[None], rvd[None]]).clone(), rows[2]


def _stats64(y, gamma, beta, rm, rv, N):
    """scale, shift, mean, rstd, running mean, running var of a training BatchNorm over y [N, C], in float64."""
    mean, var = y.mean(0), y.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma.double() * rstd
    unb = var * N / (N - 1) if N > 1 else var
    return torch.stack([scale, beta.double() - mean * scale, mean, rstd, (1 - MOM) * rm.double() + MOM * mean,
                        (1 - MOM) * rv.double() + MOM * unb])


def _check_fwd1(tag, x, ps, pt, w1, N, c, Ct, g, own_tol, f64_tol):
    x_full = torch.full((N, Ct), float("nan"))
    x_full[:, :c] = x                                              # channels c..Ct of the block buffer: never read
    gamma, beta, _, _ = fold_args(MID, g)
    rm, rv = 0.1 * torch.randn(MID, generator=g), 1 + torch.rand(MID, generator=g)
    y1, out, P = _fwd1(x_full, w1, ps, pt, N, c, Ct, gamma, beta, rm, rv)
    pxs = 64 if math.ceil(N / 64) >= 384 else 32
    if walks(N):
        assert pxs == 64 and N >= 24513 and P < math.ceil(N / pxs), (P, N)      # PT = 2, several stages per workgroup
    assert torch.isfinite(y1).all()
    a = torch.relu(x.double() * ps.double() + pt.double())
    y64 = a @ w1.view(MID, c).double().t()
    bound(tag + " y1", rel(y1, y64), 5e-6)
    names = ("scale", "shift", "mean", "rstd", "running_mean", "running_var")
    # the reduction alone: statistics of the kernel's own y1, in float64
    own = _stats64(y1.cpu().double(), gamma, beta, rm, rv, N)
    for i, nm in enumerate(names):
        bound("%s %s/own" % (tag, nm), rel(out[i], own[i]), own_tol)
    # ... and product + reduction: statistics of the float64 y1
    ref = _stats64(y64, gamma, beta, rm, rv, N)
    for i, nm in enumerate(names):
        bound("%s %s/f64" % (tag, nm), rel(out[i], ref[i]), f64_tol)
    y1b, outb, _ = _fwd1(x_full, w1, ps, pt, N, c, Ct, gamma, beta, rm, rv)
    assert torch.equal(y1, y1b) and torch.equal(out, outb)


@pytest.mark.parametrize("B,H,W,c,Ct", PROD + SMALL)
def test_dense_fwd1_stats_and_fold_against_float64(hiplib, B, H, W, c, Ct):
    """ossid_dense_fwd1_stats + ossid_bn_fold_fwd_rows: y1 (f32-level, 5e-6; measured <= 1.2e-6), norm2's fold and running
    statistics against float64 statistics of the kernel's own y1 (the reduction alone: 1e-6; measured <= 2.9e-7) and of the
    float64 y1 (5e-6; measured <= 1.2e-6); the buffer's channels past c hold NaN and must not reach y1."""
    N = B * H * W
    g = torch.Generator().manual_seed(N + 7 * c + Ct)
    x, ps, pt = away(N, c, g)
    w1 = torch.randn(MID, c, 1, 1, generator=g) / c ** 0.5
    _check_fwd1("fwd1", x, ps, pt, w1, N, c, Ct, g, 1e-6, 5e-6)


@pytest.mark.parametrize("B,H,W,c,Ct", [pytest.param(8, 60, 80, 480, 512, id="block2-last"),
                                        pytest.param(8, 29, 39, 992, 1024, id="block4-last"),
                                        pytest.param(3, 5, 9, 64, 96, id="B3-5x9")])
def test_dense_fwd1_stats_large_mean_small_spread(hiplib, B, H, W, c, Ct):
    """relu(s1 x + t1) ~ 50 +- 0.01: every y1 channel has |mean| >> std, so sums about any fixed pivot would cancel. Each
    workgroup's partial row carries its own pivot and ossid_bn_fold_fwd_rows re-centres them in double: the fold must still
    match float64 statistics of the kernel's own y1 (1e-6; measured <= 1.7e-7), and y1 must match its float64 value (5e-6; measured
    <= 2.0e-6). Against the float64 y1 the product's f32 rounding (~1e-7 of |y1| ~ 50) is a visible fraction of the spread:
    1e-3 (measured <= 2.3e-4 on rstd and scale)."""
    N = B * H * W
    g = torch.Generator().manual_seed(N + c)
    x = torch.randn(N, c, generator=g)
    ps = 0.01 * (0.5 + torch.rand(c, generator=g))
    pt = 50 + 0.1 * torch.randn(c, generator=g)
    w1 = torch.randn(MID, c, 1, 1, generator=g) / c ** 0.5
    _check_fwd1("fwd1-large-mean", x, ps, pt, w1, N, c, Ct, g, 1e-6, 1e-3)


# ---- 3x3 data gradient with norm2 / ReLU's backward -----------------------------------------------------------------------
def _dgrad3(Gfull, coff, Ct, w2, y1, alpha, ms, mt, B, H, W):
    N = B * H * W
    Gd, w2d, y1d = Gfull.cuda(), w2.cuda(), y1.cuda()
    al, msd, mtd = alpha.cuda(), ms.cuda(), mt.cuda()
    db = torch.full((N, MID), float("nan"), device="cuda")
    P = fn("ossid_dense_dgrad3_mask_partials")(B, H, W)
    part = torch.empty(P * 2 * MID, device="cuda")
    _lib.check(fn("ossid_dense_dgrad3_mask")(Gd.view(-1)[coff:].data_ptr(), Ct, T._pack(w2d, "dgrad").data_ptr(), y1d.data_ptr(),
                                             db.data_ptr(), B, H, W, al.data_ptr(), msd.data_ptr(), mtd.data_ptr(),
                                             part.data_ptr(), _lib.stream()), "ossid_dense_dgrad3_mask")
    return db, (part, P)


@pytest.mark.parametrize("B,H,W,Ct,coff", [
    pytest.param(2, 120, 160, 256, 64, id="block1-first"), pytest.param(2, 120, 160, 256, 224, id="block1-last"),
    pytest.param(8, 60, 80, 512, 128, id="block2-first"), pytest.param(8, 60, 80, 512, 480, id="block2-last"),
    pytest.param(8, 30, 40, 1024, 256, id="block3-first"), pytest.param(8, 30, 40, 1024, 992, id="block3-last"),
    pytest.param(8, 29, 39, 1024, 512, id="block4-first"), pytest.param(8, 29, 39, 1024, 992, id="block4-last"),
    pytest.param(1, 1, 1, 32, 0, id="1x1"), pytest.param(1, 3, 5, 64, 32, id="3x5"), pytest.param(3, 5, 9, 96, 64, id="B3-5x9"),
    pytest.param(2, 7, 9, 64, 0, id="7x9"), pytest.param(1, 4, 8, 32, 0, id="one-tile"), pytest.param(2, 29, 39, 96, 32, id="B2-29x39"),
])
def test_dense_dgrad3_mask_and_fold_against_float64(hiplib, B, H, W, Ct, coff):
    """ossid_dense_dgrad3_mask: db = alpha m conv2d_input(g, W2) with m = relu'(ms y1 + mt), g the 32-channel slice at coff
    of a Ct-stride buffer whose other channels hold NaN (2e-5 of the output scale, split-bf16; measured <= 6.9e-6), and the
    (d gamma, d beta, coef) of norm2 from its column sums (5e-5; measured <= 1.4e-5). alpha differs from ms here (production
    passes the same vector twice), so two swapped arguments are seen."""
    N = B * H * W
    g = torch.Generator().manual_seed(N + Ct + coff)
    gs = torch.randn(N, 32, generator=g)
    Gfull = torch.full((N, Ct), float("nan"))
    Gfull[:, coff:coff + 32] = gs
    y1, ms, mt = away(N, MID, g)
    alpha = torch.randn(MID, generator=g)
    w2 = torch.randn(32, MID, 3, 3, generator=g) / (MID * 9) ** 0.5
    gamma, _, mean, rstd = fold_args(MID, g)
    coef0 = torch.randn(2, MID, generator=g)
    db, part = _dgrad3(Gfull, coff, Ct, w2, y1, alpha, ms, mt, B, H, W)
    res = run_bn_fold_bwd(part, gamma, mean, rstd, MID, N, coef0)
    tiles = B * math.ceil(H / 4) * math.ceil(W / 8)
    if walks(N):
        assert part[1] < tiles, (part[1], tiles)                  # several tiles per workgroup
    assert torch.isfinite(db).all()
    gimg = gs.double().view(B, H, W, 32).permute(0, 3, 1, 2)
    conv = F.conv_transpose2d(gimg, w2.double(), padding=1).permute(0, 2, 3, 1).reshape(N, MID)
    m = relu_mask(y1, ms, mt)
    bound("dgrad3 db", rel(db, alpha.double() * m * conv), 2e-5)
    want = fold_bwd64((conv * m).sum(0), (conv * m * y1.double()).sum(0), gamma, mean, rstd, N)
    want = list(want[:2]) + [coef0[0].double() + want[2], coef0[1].double() + want[3]]
    for i, nm in enumerate(("dgamma", "dbeta", "coef_x", "coef_1")):
        bound("dgrad3 " + nm, rel(res[i], want[i]), 5e-5)
    db2, part2 = _dgrad3(Gfull, coff, Ct, w2, y1, alpha, ms, mt, B, H, W)
    assert torch.equal(db, db2) and torch.equal(res, run_bn_fold_bwd(part2, gamma, mean, rstd, MID, N, coef0))


# ---- 1x1 data gradient accumulated onto the block's gradient buffer, norm1's column sums ----------------------------------
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("B,H,W,c,Ct", PROD + SMALL)
def test_dense_dgrad1_acc_and_fold_against_float64(hiplib, B, H, W, c, Ct, with_add):
    """ossid_dense_dgrad1_acc: G[:, :c] += alpha m (dz_eff @ W1), m = relu'(ms x + mt), dz_eff = (dz + scale y + shift) with
    add (the 3x3's BatchNorm backward formed while dz is staged), else dz. The increment against float64 (2e-5 of its scale,
    split-bf16; measured <= 6.8e-6), G[:, c:Ct] bit-unchanged, norm1's (d gamma, d beta, coef) against float64 (5e-5; measured
    <= 1.4e-5); the block buffer's channels past c hold NaN."""
    N = B * H * W
    g = torch.Generator().manual_seed(N + 3 * c + Ct + with_add)
    x, ms, mt = away(N, c, g)
    xfull = torch.full((N, Ct), float("nan"))
    xfull[:, :c] = x
    G0 = torch.randn(N, Ct, generator=g)
    dz = torch.randn(N, MID, generator=g)
    w1 = torch.randn(MID, c, 1, 1, generator=g) / MID ** 0.5
    alpha = torch.randn(c, generator=g)
    add = (torch.randn(N, MID, generator=g), torch.randn(MID, generator=g), torch.randn(MID, generator=g)) if with_add else None
    gamma, _, mean, rstd = fold_args(c, g)
    coef0 = torch.randn(2, c, generator=g)
    bufd, dzd, w1d = xfull.cuda(), dz.cuda(), w1.cuda()
    al, msd, mtd = alpha.cuda(), ms.cuda(), mt.cuda()
    addd = None if add is None else tuple(t.cuda() for t in add)

    def run():
        Gd = G0.cuda()
        part = T.dense_dgrad1_acc(dzd, T._pack(w1d, "dgrad"), bufd, Gd, N, c, Ct, al, msd, mtd, add=addd)
        res = run_bn_fold_bwd(part, gamma, mean, rstd, c, N, coef0)
        torch.cuda.synchronize()
        return Gd.cpu(), res.cpu(), part[1]
    G, res, P = run()
    if walks(N):
        assert P < math.ceil(N / 64), (P, N)                       # several 64-pixel stages per workgroup
    dz_eff = dz.double() if add is None else (dz.double() + add[1].double() * add[0].double()) + add[2].double()
    prod = dz_eff @ w1.view(MID, c).double()
    m = relu_mask(x, ms, mt)
    assert torch.equal(G[:, c:], G0[:, c:])
    bound("dgrad1 G", rel(G[:, :c].double() - G0[:, :c].double(), alpha.double() * m * prod), 2e-5)
    want = fold_bwd64((prod * m).sum(0), (prod * m * x.double()).sum(0), gamma, mean, rstd, N)
    want = list(want[:2]) + [coef0[0].double() + want[2], coef0[1].double() + want[3]]
    for i, nm in enumerate(("dgamma", "dbeta", "coef_x", "coef_1")):
        bound("dgrad1 " + nm, rel(res[i], want[i]), 5e-5)
    G2, res2, _ = run()
    assert torch.equal(G, G2) and torch.equal(res, res2)


# ---- the 1x1 weight gradient of wgrad_group with dy_add staging -----------------------------------------------------------
@pytest.mark.parametrize("B,H,W,c,Ct", [
    pytest.param(2, 120, 160, 224, 256, id="block1-last"), pytest.param(8, 60, 80, 480, 512, id="block2-last"),
    pytest.param(8, 30, 40, 992, 1024, id="block3-last"), pytest.param(8, 29, 39, 992, 1024, id="block4-last"),
    pytest.param(8, 29, 39, 512, 1024, id="block4-first"), pytest.param(3, 5, 9, 64, 96, id="B3-5x9"),
    pytest.param(1, 1, 1, 32, 32, id="N1"),
])
def test_wgrad_group_1x1_with_dy_add_against_float64(hiplib, B, H, W, c, Ct):
    """The deferred 1x1 weight-gradient job _dense_backward hands to wgrad_group: x = relu(ps buf[:, :c] + pt) (buf of
    channel stride Ct), dy = dz + scale y1 + shift formed while staging; dw1 against float64 autograd (5e-5; measured <= 9.5e-6)
    and bit-reproducible."""
    N = B * H * W
    g = torch.Generator().manual_seed(N + c)
    x, ps, pt = away(N, c, g)
    buf = torch.randn(N, Ct, generator=g)
    buf[:, :c] = x
    dz, y1 = torch.randn(N, MID, generator=g), torch.randn(N, MID, generator=g)
    sc, sh = torch.randn(MID, generator=g), torch.randn(MID, generator=g)
    a = torch.relu(x.double() * ps.double() + pt.double()).view(B, H, W, c).permute(0, 3, 1, 2)
    w = torch.zeros(MID, c, 1, 1, dtype=torch.float64, requires_grad=True)
    dy = ((dz.double() + sc.double() * y1.double()) + sh.double()).view(B, H, W, MID).permute(0, 3, 1, 2)
    F.conv2d(a, w).backward(dy)
    bufd, dzd, y1d = buf.cuda(), dz.cuda(), y1.cuda()
    item = dict(x=bufd, dy=dzd, B=B, H=H, W=W, cin=c, cout=MID, taps=1, pre=(ps.cuda(), pt.cuda()), pre_relu=True, in_cs=Ct,
                dy_add=(y1d, sc.cuda(), sh.cuda()))
    dws = []
    for _ in range(2):
        dw = torch.full((MID, c, 1, 1), float("nan"), device="cuda")
        T.wgrad_group([dict(item, dw=dw)])
        torch.cuda.synchronize()
        dws.append(dw.cpu())
    bound("wgrad1 dy_add", rel(dws[0], w.grad), 5e-5)
    assert torch.equal(dws[0], dws[1])


# ---- argument checks ----------------------------------------------------------------------------------------------------
def test_dense_entry_points_reject_bad_arguments_without_launching(hiplib):
    """Arguments the fused dense kernels cannot take come back as EINVAL from the host-side checks, before any launch: c not
    a multiple of 32, c > 1024 (the 1x1 data gradient's eight channel tiles per wave), a channel stride below c (or not a
    multiple of 4), misaligned dz / x / g / dz_add, N Ct >= 2^32 (32-bit element offsets) and B H W 128 >= 2^31. (The 1x1
    forward walks the input channels in chunks and has no channel limit.)"""
    buf = torch.zeros(1 << 16, device="cuda")
    p, s = buf.data_ptr(), _lib.stream()
    d1, f1, d3 = fn("ossid_dense_dgrad1_acc"), fn("ossid_dense_fwd1_stats"), fn("ossid_dense_dgrad3_mask")
    # ossid_dense_dgrad1_acc(dz, wpk, x, G, n_rows, c, channel_stride, alpha, ms, mt, partials, dz_add, add_scale, add_shift, s)
    assert d1(p, p, p, p, 64, 48, 64, p, p, p, p, None, None, None, s) == EINVAL                 # c % 32 != 0
    assert d1(p, p, p, p, 4, 1056, 1056, p, p, p, p, None, None, None, s) == EINVAL              # c > 1024
    assert d1(p, p, p, p, 64, 64, 32, p, p, p, p, None, None, None, s) == EINVAL                 # channel stride < c
    assert d1(p + 4, p, p, p, 64, 64, 64, p, p, p, p, None, None, None, s) == EINVAL             # misaligned dz
    assert d1(p, p, p, p, 1 << 22, 1024, 1024, p, p, p, p, None, None, None, s) == EINVAL        # N Ct = 2^32
    assert d1(p, p, p, p, 64, 64, 64, p, p, p, p, p + 4, p, p, s) == EINVAL                      # misaligned dz_add
    assert d1(p, p, p, p, 64, 64, 64, p, p, p, p, p, None, p, s) == EINVAL                       # dz_add without its scale
    # ossid_dense_fwd1_stats(x, channel_stride, c, ps, pt, wpk, n_rows, y1, partials, counts, s)
    assert f1(p, 64, 48, p, p, p, 64, p, p, p, s) == EINVAL                                      # c % 32 != 0
    assert f1(p, 32, 64, p, p, p, 64, p, p, p, s) == EINVAL                                      # channel stride < c
    assert f1(p, 66, 64, p, p, p, 64, p, p, p, s) == EINVAL                                      # channel stride % 4 != 0
    assert f1(p + 4, 64, 64, p, p, p, 64, p, p, p, s) == EINVAL                                  # misaligned x
    # ossid_dense_dgrad3_mask(g, g_channel_stride, wpk, y1, db, B, H, W, alpha, ms, mt, partials, s)
    assert d3(p, 16, p, p, p, 1, 4, 8, p, p, p, p, s) == EINVAL                                  # channel stride < 32
    assert d3(p, 34, p, p, p, 1, 4, 8, p, p, p, p, s) == EINVAL                                  # channel stride % 4 != 0
    assert d3(p + 4, 32, p, p, p, 1, 4, 8, p, p, p, p, s) == EINVAL                              # misaligned g
    assert d3(p, 32, p, p, p, 1, 4096, 4096, p, p, p, p, s) == EINVAL                            # B H W 128 = 2^31
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


# ---- whole blocks at production channel counts ----------------------------------------------------------------------------
def _module_path(mod, xx, g):
    xr = xx.clone().requires_grad_(True)
    feats = [xr]
    for layer in mod.values():
        feats.append(layer(torch.cat(feats, 1)))
    yr = torch.cat(feats, 1)
    yr.backward(g)
    return yr, xr.grad


def l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.parametrize("L,C0,B,H,W", [pytest.param(24, 256, 1, 30, 40, id="block3"), pytest.param(16, 512, 1, 29, 39, id="block4")])
def test_dense_block_at_production_channels_matches_module_path(hiplib, L, C0, B, H, W, monkeypatch):
    """T.dense_block_train on DenseNet-121's blocks 3 and 4 (Ct = 1024: the fused backward's limit) at batch 1: the slab
    statistics finished inside the next layer's fold (ossid_bn_fold_fwd_tail), the statistics coefficients accumulated over
    up to 24 layers, every layer on the fused kernels (checked). Round 0 records the launch sequences, round 1 replays them.
    The same block run with the weight gradients on the main stream (WGRAD_SIDE off) must give every bit of the side-stream
    run: the grouped launch only changes stream.

    Output and running statistics: the bounds of test_dense_block_training_path_matches_module_path. Gradients: its float64
    bounds (input 2e-3, parameters 5e-3, or 3x torch's own float32 distance). Not its float32-vs-float32 ones: with ~7 M
    BatchNorm-ReLU decisions per pass at these channel counts, torch's float32 path lands some on the other side of the kink
    (measured: up to 4.6e-2 from float64, in L2, on 92 of block 4's 96 parameter gradients) and so does this one (block 3,
    round 0: 5.8e-3 .. 8.9e-3 on the four gradients of one layer; every other gradient <= 1.4e-3, most ~1e-5). A flipped kink
    is not systematic, a kernel fault is: one of the two rounds may miss the float64 bounds, by no more than 5e-2 (a dropped
    stage or channel tile costs O(1))."""
    torch.manual_seed(3)
    blk = backbones.DenseBlock(L, C0).cuda().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1, 0.2)
                m.bias.normal_(0, 0.2)
    ref, ref64, blk_off = copy.deepcopy(blk), copy.deepcopy(blk).double().cpu(), copy.deepcopy(blk)
    Ct = C0 + 32 * L
    seen = {"fwd1": [], "dgrad1": []}
    f_fwd, f_bwd = T.dense_fwd1_stats, T.dense_dgrad1_acc
    monkeypatch.setattr(T, "dense_fwd1_stats", lambda *a, **k: (seen["fwd1"].append(a[4]), f_fwd(*a, **k))[1])
    monkeypatch.setattr(T, "dense_dgrad1_acc", lambda *a, **k: (seen["dgrad1"].append(a[5]), f_bwd(*a, **k))[1])
    missed = []
    for rnd in range(2):
        x = torch.randn(B, C0, H, W, device="cuda") * (1 + rnd)
        go = torch.randn(B, Ct, H, W, device="cuda")
        for mod in (blk, ref, ref64, blk_off):
            for p in mod.parameters():
                p.grad = None
        yr, xr_grad = _module_path(ref, x, go)
        y64, x64_grad = _module_path(ref64, x.double().cpu(), go.double().cpu())
        res = {}
        for side, mod in ((True, blk), (False, blk_off)):
            monkeypatch.setattr(T, "WGRAD_SIDE", side)
            xm = x.clone().requires_grad_(True)
            y = T.dense_block_train(xm, mod)
            y.backward(go)
            T.join_wgrad_stream()
            torch.cuda.synchronize()
            res[side] = [y.detach().clone(), xm.grad.clone()] + [p.grad.clone() for p in mod.parameters()]
        if rnd == 0:                                               # (recorded: the fused kernels up to c = Ct - 32)
            assert max(seen["fwd1"]) == max(seen["dgrad1"]) == Ct - 32 and len(seen["dgrad1"]) == 2 * L, seen
        for a, b in zip(res[True], res[False]):
            assert torch.equal(a, b), rnd
        y, xg, pg = res[True][0], res[True][1], res[True][2:]
        assert rel(y, yr) < 5e-5, rnd
        assert rel(y, y64) < max(2e-6, 3 * rel(yr, y64)), (rnd, rel(y, y64), rel(yr, y64))
        for (n, b), q, q64 in zip(blk.named_buffers(), ref.buffers(), ref64.buffers()):
            if b.dtype.is_floating_point:
                assert rel(b, q) < 1e-4 and rel(b, q64) < 1e-4, (rnd, n)
        errs = [("input", l2(xg, x64_grad), max(2e-3, 3 * l2(xr_grad, x64_grad)))]
        errs += [(n, l2(pgr, q64.grad), max(5e-3, 3 * l2(q.grad, q64.grad)))
                 for (n, _), q, q64, pgr in zip(blk.named_parameters(), ref.parameters(), ref64.parameters(), pg)]
        for n, e, tol in errs:
            assert e < 5e-2, (rnd, n, e)
        bad = [(n, "%.2e" % e, "%.2e" % tol) for n, e, tol in errs if not e < tol]
        if bad:
            missed.append((rnd, bad))
    assert len(missed) <= 1, missed
