"""GPU tests (pytest -m gpu) of the pieces of the SqueezeNet template encoders' training node
(ossid_code_amd/dtoid/train_encoders.py) at the encoders' real shapes, each against a plain float64 restatement on the CPU:
max-pool with argmax and its gather backward, the tap-table resampler (bilinear resize, crop and their adjoints), training
BatchNorm through deferred column-sum partials, the stem as im2col + 1x1 convolution with its weight gradient re-laid, and
the encoder's grouped weight-gradient launch on its own operands. Every kernel here is deterministic (no float atomics):
every launch under test is run twice on the same inputs, and the second run must reproduce every bit. Bounds are max
|error| relative to max |float64 value|; the measured maximum is noted beside each."""
import pytest
import torch
import torch.nn.functional as F

from ossid_code_amd import _lib
from ossid_code_amd.dtoid import network, ops
from ossid_code_amd.dtoid import train_encoders as TE
from ossid_code_amd.dtoid import train_ops as T

pytestmark = pytest.mark.gpu

EINVAL = -22
B = 8                     # the finetune step's template batch


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _maxpool(x, k, stride, pad, ceil):
    _, C, H, W = x.shape
    Ho, Wo = TE._pool_out(H, k, stride, pad, ceil), TE._pool_out(W, k, stride, pad, ceil)
    out = T.empty_nhwc(B, C, Ho, Wo, "cuda")
    idx = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.fn("ossid_maxpool_idx_nhwc")(x.data_ptr(), B, H, W, C, k, stride, pad, 1 if ceil else 0, out.data_ptr(),
                                                  idx.data_ptr(), _lib.stream()), "ossid_maxpool_idx_nhwc")
    return out, idx.view(B, Ho, Wo, C).permute(0, 3, 1, 2)


def _maxpool_bwd(g, idx, H, W, k, stride, pad):
    _, C, Ho, Wo = g.shape
    dx = T.empty_nhwc(B, C, H, W, "cuda")
    _lib.check(_lib.fn("ossid_maxpool_bwd_nhwc")(g.data_ptr(), idx.permute(0, 2, 3, 1).contiguous().data_ptr(), B, H, W, C, k,
                                                  stride, pad, Ho, Wo, dx.data_ptr(), _lib.stream()), "ossid_maxpool_bwd_nhwc")
    return dx


def _flat_input_index(idx, W, k, stride, pad):
    """Window position dy * k + dx -> torch's index into the input plane."""
    Ho, Wo = idx.shape[2], idx.shape[3]
    yo = torch.arange(Ho, device=idx.device).view(1, 1, -1, 1)
    xo = torch.arange(Wo, device=idx.device).view(1, 1, 1, -1)
    a = idx.long()
    return (yo * stride - pad + a // k) * W + (xo * stride - pad + a % k)


@pytest.mark.parametrize("C,H,W,k,stride,pad,ceil", [
    (64, 61, 61, 3, 2, 0, True),        # 61 -> 30
    (128, 30, 30, 3, 2, 0, True),       # 30 -> 15: the last window of each row and column is partial (two of three)
    (256, 15, 15, 3, 2, 0, True),       # 15 -> 7
    (64, 30, 40, 3, 2, 1, False),       # padded windows (DenseNet's pool0 form)
])
def test_maxpool_argmax_and_backward_at_the_encoder_shapes(hiplib, C, H, W, k, stride, pad, ceil):
    """ossid_maxpool_idx_nhwc: output torch.equal to F.max_pool2d, argmax = torch's indices (tie-free inputs);
    ossid_maxpool_bwd_nhwc (a gather over the <= 4 overlapping windows of each input) against a float64 scatter-add
    (bound 2.5e-7; measured 8.9e-8: at most four float32 terms per input)."""
    g = torch.Generator().manual_seed(C + H + pad)
    x = cl(torch.randn(B, C, H, W, generator=g))
    want, want_idx = F.max_pool2d(x, k, stride, pad, ceil_mode=ceil, return_indices=True)
    out, idx = _maxpool(x, k, stride, pad, ceil)
    assert out.shape == want.shape and torch.equal(out, want)
    assert torch.equal(_flat_input_index(idx, W, k, stride, pad), want_idx)
    go = cl(torch.randn(want.shape, generator=g))
    dx = _maxpool_bwd(go, idx, H, W, k, stride, pad)
    ref = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, want_idx.cpu().view(B, C, -1), go.double().cpu().view(B, C, -1))
    assert rel(dx, ref.view(B, C, H, W)) < 2.5e-7
    out2, idx2 = _maxpool(x, k, stride, pad, ceil)
    assert torch.equal(out2, out) and torch.equal(idx2, idx)
    assert torch.equal(_maxpool_bwd(go, idx, H, W, k, stride, pad), dx)


def test_maxpool_all_zero_windows_take_the_first_maximum(hiplib):
    """ReLU outputs: whole windows of exact zeros (and ties between equal positives). The documented rule -- the first
    maximum in window order wins -- decides the argmax, and the backward sends each window's gradient there only (bound
    1.8e-7 against float64; measured 5.9e-8)."""
    g = torch.Generator().manual_seed(4)
    C, H, W = 128, 30, 30
    x = torch.relu(torch.randn(B, C, H, W, generator=g) - 1.0)           # ~84 % zeros: many all-zero windows
    x[:, :, 10:20, 10:20] = 0.0
    x[:, :, 0:3, 0:3] = 0.5                                              # a window of equal positives
    xd = cl(x)
    out, idx = _maxpool(xd, 3, 2, 0, True)
    win = F.pad(x.double(), (0, 1, 0, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2).reshape(B, C, 15, 15, 9)
    first = (win == win.max(-1, keepdim=True).values).double().argmax(-1)       # first position holding the maximum
    assert torch.equal(idx.long().cpu(), first)
    assert bool((idx[:, :, 5:9, 5:9] == 0).all()) and bool((idx[:, :, 0, 0] == 0).all())
    assert torch.equal(out, F.max_pool2d(xd, 3, 2, 0, ceil_mode=True))
    go = cl(torch.randn(B, C, 15, 15, generator=g))
    dx = _maxpool_bwd(go, idx, H, W, 3, 2, 0)
    ref = torch.zeros(B, C, H * W, dtype=torch.float64).scatter_add_(2, _flat_input_index(idx, W, 3, 2, 0).cpu().view(B, C, -1),
                                                                       go.double().cpu().view(B, C, -1))
    assert rel(dx, ref.view(B, C, H, W)) < 1.8e-7
    out2, idx2 = _maxpool(xd, 3, 2, 0, True)
    assert torch.equal(out2, out) and torch.equal(idx2, idx)
    assert torch.equal(_maxpool_bwd(go, idx, H, W, 3, 2, 0), dx)


def _resample(x_flat, Hin, Win, C, x_cs, Hout, Wout, ty, tx, out_flat, out_cs=0, out_coff=0):
    TE.resample(x_flat, B, Hin, Win, C, x_cs, Hout, Wout, ty, tx, out_flat, out_cs=out_cs, out_coff=out_coff)


def test_resample_bilinear_tap_into_a_channel_slice_and_its_adjoint(hiplib):
    """The 30 -> 7 bilinear resize of the 128-channel tap into channels 512..639 of the 640-channel result (channels 0..511,
    pre-filled with NaN, must come back untouched), and its adjoint read from that channel slice (x_cs 640, offset 512),
    against float64 F.interpolate(bilinear, align_corners=False) and its autograd. Bounds 6e-6 (measured 1.9e-6 and
    2.1e-6): the tap weights are torch's float32 formula, whose source coordinate (up to ~29) carries ~2e-6 of rounding."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 128, 30, 30, generator=g)
    xf = torch.full((B, 640, 7, 7), float("nan")).cuda().contiguous(memory_format=torch.channels_last)
    tyf, txf = TE.tap_tables("bilinear", 30, 7, "cuda"), TE.tap_tables("bilinear", 30, 7, "cuda")
    _resample(T.flat(cl(x)), 30, 30, 128, 0, 7, 7, tyf, txf, T.flat(xf), out_cs=640, out_coff=512)
    x64 = x.double().requires_grad_(True)
    want = F.interpolate(x64, size=(7, 7), mode="bilinear", align_corners=False)
    assert bool(torch.isnan(xf[:, :512]).all())
    assert rel(xf[:, 512:], want) < 6e-6
    xf2 = torch.full((B, 640, 7, 7), float("nan")).cuda().contiguous(memory_format=torch.channels_last)
    _resample(T.flat(cl(x)), 30, 30, 128, 0, 7, 7, tyf, txf, T.flat(xf2), out_cs=640, out_coff=512)
    assert torch.equal(xf2[:, 512:], xf[:, 512:]) and bool(torch.isnan(xf2[:, :512]).all())
    gf = torch.randn(B, 640, 7, 7, generator=g)
    want.backward(gf[:, 512:].double())
    gd = cl(gf)
    dx = T.empty_nhwc(B, 128, 30, 30, "cuda")
    tya, txa = TE.tap_tables("bilinear", 30, 7, "cuda", adjoint=True), TE.tap_tables("bilinear", 30, 7, "cuda", adjoint=True)
    _resample(T.flat(gd, 512), 7, 7, 128, 640, 30, 30, tya, txa, T.flat(dx))
    assert rel(dx, x64.grad) < 6e-6
    dx2 = T.empty_nhwc(B, 128, 30, 30, "cuda")
    _resample(T.flat(gd, 512), 7, 7, 128, 640, 30, 30, tya, txa, T.flat(dx2))
    assert torch.equal(dx2, dx)


def test_resample_non_square_pads_the_shorter_tap_table(hiplib):
    """30 x 24 -> 7 x 15 and its adjoint through train_encoders.resample: the adjoint's row table has one tap per output
    index and its column table two, so resample pads the row table (_pad_taps) to a common T (bounds 6e-6 as above;
    measured 2.2e-6 and 1.7e-6)."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(B, 64, 30, 24, generator=g)
    out = T.empty_nhwc(B, 64, 7, 15, "cuda")
    _resample(T.flat(cl(x)), 30, 24, 64, 0, 7, 15, TE.tap_tables("bilinear", 30, 7, "cuda"), TE.tap_tables("bilinear", 24, 15, "cuda"),
              T.flat(out))
    x64 = x.double().requires_grad_(True)
    want = F.interpolate(x64, size=(7, 15), mode="bilinear", align_corners=False)
    assert rel(out, want) < 6e-6
    out2 = T.empty_nhwc(B, 64, 7, 15, "cuda")
    _resample(T.flat(cl(x)), 30, 24, 64, 0, 7, 15, TE.tap_tables("bilinear", 30, 7, "cuda"), TE.tap_tables("bilinear", 24, 15, "cuda"),
              T.flat(out2))
    assert torch.equal(out2, out)
    go = torch.randn(B, 64, 7, 15, generator=g)
    want.backward(go.double())
    ty, tx = TE.tap_tables("bilinear", 30, 7, "cuda", adjoint=True), TE.tap_tables("bilinear", 24, 15, "cuda", adjoint=True)
    assert ty[2] == 1 and tx[2] == 2                      # (so that the padding path is the one under test)
    dx = T.empty_nhwc(B, 64, 30, 24, "cuda")
    _resample(T.flat(cl(go)), 7, 15, 64, 0, 30, 24, ty, tx, T.flat(dx))
    assert rel(dx, x64.grad) < 6e-6
    dx2 = T.empty_nhwc(B, 64, 30, 24, "cuda")
    _resample(T.flat(cl(go)), 7, 15, 64, 0, 30, 24, ty, tx, T.flat(dx2))
    assert torch.equal(dx2, dx)


@pytest.mark.parametrize("C,H", [(128, 7), (64, 5)])
def test_resample_crop_and_its_zero_padding_adjoint(hiplib, C, H):
    """The crops behind the global branch's valid 3x3 convolutions (7 -> 5 at 128 channels, 5 -> 3 at 64) are exact copies
    of the interior; their adjoints put the gradient back with exact zeros on the border. Each direction runs twice (a
    repeat into a NaN-filled buffer)."""
    g = torch.Generator().manual_seed(C + H)
    x = cl(torch.randn(B, C, H, H, generator=g))
    dc = cl(torch.randn(B, C, H - 2, H - 2, generator=g))
    tc, ta = TE.tap_tables("crop", H, H - 2, "cuda"), TE.tap_tables("crop", H, H - 2, "cuda", adjoint=True)
    for _ in range(2):
        c = torch.full((B, C, H - 2, H - 2), float("nan")).cuda().contiguous(memory_format=torch.channels_last)
        _resample(T.flat(x), H, H, C, 0, H - 2, H - 2, tc, tc, T.flat(c))
        assert torch.equal(c, x[:, :, 1:-1, 1:-1])
        du = torch.full((B, C, H, H), float("nan")).cuda().contiguous(memory_format=torch.channels_last)
        _resample(T.flat(dc), H - 2, H - 2, C, 0, H, H, ta, ta, T.flat(du))
        assert torch.equal(du, F.pad(dc, (1, 1, 1, 1)))
        assert float(du[:, :, 0].abs().max()) == 0 and float(du[:, :, :, -1].abs().max()) == 0


def test_resample_rejects_bad_arguments(hiplib):
    """EINVAL from the host-side checks, before any launch, for a channel count that is no multiple of 4, more than 8
    taps, and a channel slice that does not fit its stride. (The first call, with valid arguments, does launch: all-zero
    tap weights, every read in bounds.) Not repeated: nothing here computes a value."""
    x = torch.zeros(B * 30 * 30 * 640, device="cuda")
    out = torch.zeros(B * 7 * 7 * 640, device="cuda")
    idx = torch.zeros(9 * 30, dtype=torch.int32, device="cuda")
    w = torch.zeros(9 * 30, device="cuda")
    f = _lib.fn("ossid_resample_taps_nhwc")

    def call(C, x_cs, T_, out_cs, out_coff):
        return f(x.data_ptr(), B, 30, 30, C, x_cs, 7, 7, idx.data_ptr(), w.data_ptr(), idx.data_ptr(), w.data_ptr(), T_,
                 out.data_ptr(), out_cs, out_coff, _lib.stream())
    assert call(128, 0, 2, 640, 512) == 0
    assert call(126, 0, 2, 0, 0) == EINVAL                # C % 4
    assert call(128, 0, 9, 0, 0) == EINVAL                # T > 8
    assert call(128, 0, 2, 640, 516) == EINVAL            # offset + C past the stride
    assert call(128, 64, 2, 0, 0) == EINVAL               # input stride below C
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_img,C,g_cs", [(30 * 30, 128, 0), (7 * 7, 512, 640), (5 * 5, 128, 0), (3 * 3, 64, 0)])
def test_training_batchnorm_through_deferred_partials_matches_float64(hiplib, n_img, C, g_cs):
    """Training BatchNorm at the encoders' shapes -- B x 30 x 30 x 128, B x 7 x 7 x 512 with the gradient read from the
    640-channel result (g_cs 640), B x 5 x 5 x 128 and B x 3 x 3 x 64 -- against float64 BatchNorm2d forward / backward.
    Inputs sit at mean 3 with spread 1 (the pivot matters). Forward two ways: the encoders' own _bn_train (pivoted column
    sums finished by chan_op, then folded) and batch_stats(defer=True) -> bn_fold_fwd, which combines the per-block partial
    rows itself (n_partials > 0); both folds, the normalised output and the running statistics against float64, and the
    two folds against each other. Backward through _bn_back, whose chan_op leaves deferred partials for bn_fold_bwd.
    Bounds: folds, output and running statistics 1e-6 (measured 3.2e-7; the two folds differ by up to 2.8e-7); input,
    gamma and beta gradients 1.5e-6 (measured 7.1e-7)."""
    import copy
    g = torch.Generator().manual_seed(n_img + C)
    H = int(round(n_img ** 0.5))
    x = 3.0 + torch.randn(B, C, H, H, generator=g)
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
        bn.bias.copy_(0.3 * torch.randn(C, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=g))
    r64 = copy.deepcopy(bn).double().cpu()
    x64 = x.double().requires_grad_(True)
    y64 = r64(x64)
    gw = torch.randn(B, g_cs or C, H, H, generator=g)
    y64.backward(gw[:, :C].double())                     # (norm_2's gradient: channels 0..511 of the result's)
    xd64 = x64.detach()
    mean64 = xd64.mean((0, 2, 3))
    rstd64 = 1.0 / torch.sqrt(xd64.var((0, 2, 3), unbiased=False) + bn.eps)
    scale64 = r64.weight.detach() * rstd64
    fold64 = torch.stack([scale64, r64.bias.detach() - mean64 * scale64, mean64, rstd64])
    n = B * H * H
    xd = cl(x)
    gd = cl(gw)
    res = []
    for _ in range(2):
        b2, b3 = copy.deepcopy(bn), copy.deepcopy(bn)
        f = TE._bn_train(T.flat(xd), n, C, b2)
        st = T.batch_stats(T.flat(xd), n, C, defer=True)
        assert st[1] > 1                                  # (several partial rows for the fold to combine)
        fd = T.bn_fold_fwd(st, C, n, b3.weight, b3.bias, b3.eps, T._mom(b3), b3.running_mean, b3.running_var)
        y = T.empty_nhwc(B, C, H, H, "cuda")
        T.chan_op(T.flat(xd), n, C, out=T.flat(y), alpha=f[0], kappa=f[1])
        yd = T.empty_nhwc(B, C, H, H, "cuda")
        T.chan_op(T.flat(xd), n, C, out=T.flat(yd), alpha=fd[0], kappa=fd[1])
        dx = T.empty_nhwc(B, C, H, H, "cuda")
        dg, db = TE._bn_back(T.flat(gd), T.flat(xd), n, C, f, b2, T.flat(dx), g_cs=g_cs)
        torch.cuda.synchronize()
        res.append([f, fd, y, yd, dx, dg.clone(), db.clone(), b2.running_mean, b2.running_var, b3.running_mean, b3.running_var])
    f, fd, y, yd, dx, dg, db, rm, rv, rmd, rvd = res[0]
    for fold, ys, m, v in ((f, y, rm, rv), (fd, yd, rmd, rvd)):
        assert all(rel(fold[i], fold64[i]) < 1e-6 for i in range(4))
        assert rel(ys, y64) < 1e-6 and rel(m, r64.running_mean) < 1e-6 and rel(v, r64.running_var) < 1e-6
    # the same column sums combined in another order (finished partials vs partials summed in the fold, both in double)
    assert rel(fd, f) < 1e-6 and rel(yd, y) < 1e-6 and rel(rmd, rm) < 1e-6 and rel(rvd, rv) < 1e-6
    assert rel(dx, x64.grad) < 1.5e-6 and rel(dg, r64.weight.grad) < 1.5e-6 and rel(db, r64.bias.grad) < 1.5e-6
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def test_stem_weight_relayout_is_a_permutation_and_its_inverse_undoes_it(hiplib):
    """[64,4,3,3] -> [64,48] in ossid_im2col_stem's column order ((ky * 3 + kx) * 4 + c, columns 36..47 zero) and back."""
    g = torch.Generator().manual_seed(8)
    w = torch.randn(64, 4, 3, 3, generator=g).cuda()
    m = torch.full((64, TE.STEM_KPAD), float("nan"), device="cuda")
    TE.stem_relayout(w, m, 64, 4, 3, TE.STEM_KPAD)
    want = torch.zeros(64, TE.STEM_KPAD)
    want[:, :36] = w.cpu().permute(0, 2, 3, 1).reshape(64, 36)
    assert torch.equal(m.cpu(), want)
    back = torch.full((64, 4, 3, 3), float("nan"), device="cuda")
    TE.stem_relayout(m, back, 64, 4, 3, TE.STEM_KPAD, inverse=True)
    assert torch.equal(back, w)


def test_stem_as_im2col_plus_1x1_and_its_weight_gradient_match_float64(hiplib):
    """The 4-channel 3x3/s2 stem at 8 x 4 x 124 x 124: ossid_im2col_stem + the 1x1 exact-f32 convolution with the ReLU in
    its epilogue against float64 conv2d + ReLU (bound 9e-7; measured 3.1e-7), and the weight gradient as the encoder takes
    it -- the grouped launch on the im2col columns in column order, re-laid by the inverse relayout -- against float64
    conv2d's weight gradient (bound 1.2e-5; measured 4.3e-6). Both bit-reproducible."""
    g = torch.Generator().manual_seed(9)
    img = torch.rand(B, 4, 124, 124, generator=g)
    w = torch.randn(64, 4, 3, 3, generator=g) * (2.0 / 36) ** 0.5
    bias = torch.randn(64, generator=g) * 0.1
    cols = ops.im2col_stem(img.cuda(), 3, 2, 0, TE.STEM_KPAD)
    wpk = TE.stem_packed(w.cuda())                       # (the encoders' own packing of the stem)
    outs = []
    for _ in range(2):
        x0 = T.empty_nhwc(B, 64, 61, 61, "cuda")
        T.conv_raw(cols, wpk, B, 61, 61, TE.STEM_KPAD, 64, 1, x0, bias=bias.cuda(), act=2)
        outs.append(x0)
    w64 = w.double().requires_grad_(True)
    want = torch.relu(F.conv2d(img.double(), w64, bias.double(), stride=2))
    assert rel(outs[0], want) < 9e-7 and torch.equal(outs[0], outs[1])
    dy = torch.randn(B, 64, 61, 61, generator=g) * (want > 0).float()
    F.conv2d(img.double(), w64, bias.double(), stride=2).backward(dy.double())
    dys = cl(dy)
    got = []
    for _ in range(2):
        dw_cols = torch.empty(64, TE.STEM_KPAD, 1, 1, device="cuda")
        T.wgrad_group([dict(x=cols, dy=dys, B=B, H=61, W=61, cin=TE.STEM_KPAD, cout=64, taps=1, dw=dw_cols)])
        dw = torch.empty(64, 4, 3, 3, device="cuda")
        TE.stem_relayout(dw_cols, dw, 64, 4, 3, TE.STEM_KPAD, inverse=True)
        got.append(dw)
    assert rel(got[0], w64.grad) < 1.2e-5 and torch.equal(got[0], got[1])


def _nhwc_view(t, Bn, H, W, C, cs):
    """[B,H,W,C] float64 CPU copy of a channels-last operand: a 4-D channels-last tensor or a flat pointer + channel stride."""
    cs = cs or C
    if t.dim() == 4:
        return t.detach().permute(0, 2, 3, 1)[..., :C].double().cpu()
    return torch.as_strided(t, (Bn, H, W, C), (H * W * cs, W * cs, cs, 1)).double().cpu()


def test_grouped_weight_gradient_of_an_encoder_on_its_own_operands(hiplib, monkeypatch):
    """The ONE grouped launch that computes all ~25 weight gradients of a training encoder (TemplateFeatExtractGlobal: every
    layer of the local one plus the two global convolutions), on the descriptor list _encoder_backward builds -- 1x1 and 3x3
    layers, the expand 3x3's dy a channel slice at offset n1 of the Fire output's gradient (dy_cs = n1 + n3), pixel counts
    per image of 225 and 49 (no multiple of 32), the stem on its 48 im2col columns, the global convolutions with the
    previous BatchNorm as an input affine without ReLU -- each dw against float64 conv2d's weight gradient of the same
    operands (bound 4e-5; measured 1.3e-5), and bit-reproducible."""
    torch.manual_seed(12)
    mod = network.TemplateFeatExtractGlobal().cuda().train()
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1, 0.2)
                m.bias.normal_(0, 0.2)
            elif isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                m.bias.normal_(0, 0.1)
    captured = []
    real = T.wgrad_group

    def spy(items):
        captured.append(list(items))
        return real(items)
    monkeypatch.setattr(T, "wgrad_group", spy)
    g = torch.Generator().manual_seed(13)
    img = torch.rand(B, 4, 124, 124, generator=g).cuda()
    out, sv = TE._encoder_forward(mod, ops.im2col_stem(img, 3, 2, 0, TE.STEM_KPAD))
    go = cl(torch.randn(out.shape, generator=g))
    TE._encoder_backward(mod, go, sv, side=False)
    torch.cuda.synchronize()
    assert len(captured) == 1
    items = captured[0]
    assert len(items) == 1 + 8 * 3 + 2
    # the Fire modules' expand pair: e3's dy is e1's pointer + n1 floats, both with the Fire output's channel stride
    fires = [m for part in (mod.backbone_1, mod.backbone_2) for m in part if hasattr(m, "squeeze")]
    n_pairs = 0
    for i in range(len(items) - 1):
        a, b = items[i], items[i + 1]
        if a["taps"] == 1 and b["taps"] == 9 and a["dy_cs"] and a["dy_cs"] == b["dy_cs"] == a["cout"] + b["cout"]:
            assert b["dy"].data_ptr() == a["dy"].data_ptr() + 4 * a["cout"]
            n_pairs += 1
    assert n_pairs == len(fires)
    assert sum(1 for it in items if it.get("pre") is not None) == 1          # final_conv_2 behind final_norm_1
    assert {(it["H"], it["W"]) for it in items} >= {(15, 15), (7, 7), (5, 5), (61, 61)}
    for it in items:
        Bn, H, W, cin, cout, taps = it["B"], it["H"], it["W"], it["cin"], it["cout"], it["taps"]
        x = _nhwc_view(it["x"], Bn, H, W, cin, it["in_cs"]).permute(0, 3, 1, 2)
        if it.get("pre") is not None:
            x = x * it["pre"][0].double().cpu().view(1, -1, 1, 1) + it["pre"][1].double().cpu().view(1, -1, 1, 1)
        dy = _nhwc_view(it["dy"], Bn, H, W, cout, it["dy_cs"]).permute(0, 3, 1, 2)
        k = 3 if taps == 9 else 1
        want = torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dy, padding=k // 2)
        e = rel(it["dw"].view(cout, cin, k, k), want)
        assert e < 4e-5, (cin, cout, taps, H, e)
    again = [dict(it, dw=torch.full_like(it["dw"], float("nan"))) for it in items]
    real(again)
    torch.cuda.synchronize()
    assert all(torch.equal(a["dw"], b["dw"]) for a, b in zip(items, again))
