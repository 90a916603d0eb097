"""The scorer's training kernels (csrc/pn2_train.hip, SPEC.md 12) at their edges: every case of tests/pn2_train_cases.py
through the ossid_pn2_train_* stage entry points and, for the whole-model shapes, through the float64 harness of
tests/test_pn2_train_gpu.py (the GPU's decisions exported, imposed on the restatement, compared against float64).

Stage kernels: every output buffer is pre-filled with NaN. Where the inputs are small integers every partial sum is exact in
float32 and the result is compared bit for bit with integer arithmetic: a dropped, doubled or misplaced term shows at any
shape. tests/test_pn2_train_edges.py says on the host which tail each shape is there for.

Which test holds which guard of the kernels (read through, guard by guard; without it the kernel would do as said):
  gk < k1 in gemm_kernel                  test_gemm_exact: with K = Kr = Kp ending inside a slice (1, 7, 15, 17, ...) row m of
                                          the forward takes in X[m + 1][0..] * W[n + 1][0..]; test_pad_columns_are_not_read: with
                                          Kp > Kr it takes in the NaN pads; test_weight_gradient_splits_exact: the last split
                                          (R 511, 513, 544, 65537, 131073) takes in the NaN rows behind both operands
  min(R, r0 + rpc) in colstats_kernel     test_bn_stats_at_chunk_edges: R 257, 544, 65537, 70001 have a short last chunk, which
                                          then takes in the NaN rows behind Z
  min(R, r0 + rpc) in bn_bwd_reduce_kernel  test_whole_model_gradients[E2-gamma] and [E2-beta]: R3 = 544, the third chunk of layers
                                          6..8 takes in two rows of whatever follows Z and dA in the workspace. This rests on
                                          the order in which carve() lays the workspace out: finite non-zero activations follow
                                          Z and A of layers 6 and 7 (the sums then move by about 2 / 544); at the pooled layer
                                          8 the stray arg-max entry would have to name the row, so it most likely does not
                                          show there. No stage entry point reaches this kernel alone
  c < Cf in ungroup_kernel                test_ungroup_exact: Cf 1, 63, 65, 255, 257, 300; the lanes past Cf add the next
                                          entry's values and write over the next target's first channels
"""
import numpy as np
import pytest
import torch

import pn2_train_cases as pc
import test_pn2_train_gpu as tg
from test_pn2_train_gpu import _bounded, _dev, _gpu_step, _model, _param_list

pytestmark = pytest.mark.gpu

NAN = float("nan")
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module", autouse=True)
def _drop_the_cases_afterwards():
    yield
    for k in [k for k in tg._CASES if k not in tg.SHAPES]:
        del tg._CASES[k]


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def with_nan_rows(t, extra):
    """t [R, C] on the device with `extra` rows of NaN behind it: a reduction that runs past row R shows, and reads nothing
    it does not own."""
    out = nans(t.shape[0] + extra, t.shape[1])
    out[:t.shape[0]] = t
    return out


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


# ---- the three GEMM settings ------------------------------------------------------------------------------------------------------
def linear_fwd(lib, Xp, W):
    """Xp [R, Kp] (the weight's Kr columns first), W [C, Kr] -> Z [R, C] over a NaN pre-fill."""
    (R, Kp), (C, Kr) = Xp.shape, W.shape
    Xd, Wd, Z = _dev(Xp), _dev(W), nans(R, C)
    lib.check(lib.fn("ossid_pn2_train_linear_fwd")(Xd.data_ptr(), R, Kp, Wd.data_ptr(), Kr, C, Z.data_ptr(), lib.stream()), "fwd")
    return Z.cpu()


def linear_dgrad(lib, dZ, W, c0):
    """dX [R, Kr - c0] = dZ . W[:, c0:], the weight's row stride left at Kr (ldw > N where c0 > 0, as SA2 and SA3 call it)."""
    (R, C), Kr = dZ.shape, W.shape[1]
    N = Kr - c0
    dZd, Wd, dX = _dev(dZ), _dev(W), nans(R, N)
    lib.check(lib.fn("ossid_pn2_train_linear_dgrad")(dZd.data_ptr(), R, C, Wd.data_ptr() + 4 * c0, Kr, N, dX.data_ptr(),
                                                     lib.stream()), "dgrad")
    return dX.cpu()


def linear_wgrad(lib, dZ, Xp, Kr, runs=1):
    """dW [C, Kr] = dZ^T . Xp[:, :Kr], the workspace sized by the query; `runs` results, each over a NaN pre-fill. Both
    operands are followed by a slice's worth of NaN rows."""
    (R, C), Kp = dZ.shape, Xp.shape[1]
    nb = lib.fn("ossid_pn2_train_wgrad_workspace_bytes")(R, C, Kr)
    assert nb == (pc.wgrad_split(R)[1] * C * Kr * 4 if pc.wgrad_split(R)[1] > 1 else 0) + 256
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dZd, Xd, out = with_nan_rows(dZ, 16), with_nan_rows(Xp, 16), []
    for _ in range(runs):
        dW = nans(C, Kr)
        lib.check(lib.fn("ossid_pn2_train_linear_wgrad")(dZd.data_ptr(), R, C, Xd.data_ptr(), Kp, Kr, dW.data_ptr(), ws.data_ptr(),
                                                         nb, lib.stream()), "wgrad")
        out.append(dW.cpu())
    return out if runs > 1 else out[0]


def dgrad_columns(Kr):
    return (0, 3) if Kr > 3 else (0,)


@pytest.mark.parametrize("R,C,Kr", pc.GEMM_GRID, ids=[pc.gid(t) for t in pc.GEMM_GRID])
def test_gemm_exact(hiplib, R, C, Kr):
    """Forward, data gradient (from column 0 and from column 3) and weight gradient on integers in [-3, 3]: bit-equal to
    the int64 product, at every padded width."""
    X, W, dZ = pc.gemm_operands(R, C, Kr)
    want_z, want_dw = pc.exact(X, W.t()), pc.exact(dZ.t(), X)
    for Kp in pc.kp_variants(Kr):
        Xp = pc.padded(X, Kp, 0.0)
        assert torch.equal(linear_fwd(hiplib, Xp, W), want_z), ("fwd", Kp)
        assert torch.equal(linear_wgrad(hiplib, dZ, Xp, Kr), want_dw), ("wgrad", Kp)
    for c0 in dgrad_columns(Kr):
        assert torch.equal(linear_dgrad(hiplib, dZ, W, c0), pc.exact(dZ, W[:, c0:])), ("dgrad", c0)


@pytest.mark.parametrize("R,C,Kr", pc.GEMM_GRID, ids=[pc.gid(t) for t in pc.GEMM_GRID])
def test_pad_columns_are_not_read(hiplib, R, C, Kr):
    """X[:, Kr:Kp] full of NaN: forward and weight gradient give the bits they give with zeros there."""
    X, W, dZ = pc.gemm_operands(R, C, Kr)
    for Kp in pc.kp_variants(Kr):
        if Kp == Kr:
            continue
        zero, nan = pc.padded(X, Kp, 0.0), pc.padded(X, Kp, NAN)
        assert torch.isnan(nan[:, Kr:]).all() and not torch.isnan(nan[:, :Kr]).any()
        assert same_bits(linear_fwd(hiplib, nan, W), linear_fwd(hiplib, zero, W)), ("fwd", Kp)
        assert same_bits(linear_wgrad(hiplib, dZ, nan, Kr), linear_wgrad(hiplib, dZ, zero, Kr)), ("wgrad", Kp)


@pytest.mark.parametrize("R", pc.WGRAD_R)
def test_weight_gradient_splits_exact(hiplib, R):
    """C = 64, Kr = 8, integers in [-3, 3] (|sum| <= 9 * 133120 < 2^24): bit-equal to the int64 product whatever the
    split's tail, and the same bits twice."""
    C, Kr = pc.WGRAD_C, pc.WGRAD_KR
    X, _, dZ = pc.gemm_operands(R, C, Kr)
    a, b = linear_wgrad(hiplib, dZ, X, Kr, runs=2)
    print("R %d: chunk %d, %d splits, %d rows in the last" % ((R,) + pc.wgrad_split(R)))
    assert torch.equal(a, pc.exact(dZ.t(), X))
    assert same_bits(a, b)


@pytest.mark.parametrize("R,C,Kr", pc.GEMM_REAL, ids=[pc.gid(t) for t in pc.GEMM_REAL])
def test_gemm_against_float64(hiplib, R, C, Kr):
    """Real-valued operands at ragged M, N and K: err <= 4 * max(e32, 2^-24), both relative to max|float64 result|, e32 a
    float32 torch product of the same operands. Measured on the MI355X: the largest ratio err / max(e32, 2^-24) over the
    four products of a shape is 1.00 at (33, 31, 7) and (63, 65, 17) and 0.46 .. 0.76 at the other six."""
    X, W, dZ = pc.gemm_operands(R, C, Kr, real=True)
    Kp = (Kr + 7) // 8 * 8
    Xp = pc.padded(X, Kp, 0.0)
    what = "%s" % ((R, C, Kr),)
    ratios = [_bounded(linear_fwd(hiplib, Xp, W), X.double() @ W.double().t(), X @ W.t(), "fwd " + what, FLOOR)]
    for c0 in dgrad_columns(Kr):
        ratios.append(_bounded(linear_dgrad(hiplib, dZ, W, c0), dZ.double() @ W.double()[:, c0:], dZ @ W[:, c0:],
                               "dgrad %s from column %d" % (what, c0), FLOOR))
    ratios.append(_bounded(linear_wgrad(hiplib, dZ, Xp, Kr), dZ.double().t() @ X.double(), dZ.t() @ X, "wgrad " + what, FLOOR))
    print("%s: the largest ratio is %.2f" % (what, max(ratios)))


@pytest.mark.parametrize("R", pc.WGRAD_REAL_R)
def test_weight_gradient_splits_against_float64(hiplib, R):
    """The ragged splits of test_weight_gradient_splits_exact on real-valued operands (C = 64, Kr = 8), the same bound.
    Measured on the MI355X: ratio 0.43 at R = 544 (err 1.8e-7) and 0.06 at R = 131073 (err 4.4e-7 against torch's 7.3e-6)."""
    C, Kr = pc.WGRAD_C, pc.WGRAD_KR
    X, _, dZ = pc.gemm_operands(R, C, Kr, real=True)
    _bounded(linear_wgrad(hiplib, dZ, X, Kr), dZ.double().t() @ X.double(), dZ.t() @ X, "wgrad %s" % ((R, C, Kr),), FLOOR)


# ---- BatchNorm statistics ---------------------------------------------------------------------------------------------------------
def bn_stats(lib, z):
    R, C = z.shape
    nb = lib.fn("ossid_pn2_train_bn_stats_workspace_bytes")()
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    mean, rstd, var = nans(C), nans(C), nans(C)
    zd = with_nan_rows(z, pc.stat_chunks(R)[1])           # a chunk's worth of NaN rows behind row R
    rc = lib.fn("ossid_pn2_train_bn_stats")(zd.data_ptr(), R, C, ws.data_ptr(), nb, mean.data_ptr(), rstd.data_ptr(),
                                            var.data_ptr(), lib.stream())
    torch.cuda.synchronize()
    return rc, mean.cpu(), rstd.cpu(), var.cpu()


@pytest.mark.parametrize("R,C", pc.STATS_CASES, ids=[pc.gid(t) for t in pc.STATS_CASES])
def test_bn_stats_at_chunk_edges(hiplib, R, C):
    """Integers in [-8, 8], so the float64 sums are exact: mean, rstd and var within 1 float32 ulp of the kernel's own
    formulas evaluated in numpy float64 (not equality: nobody has pinned the device's rounding of the three divisions and
    the square root). Measured on the MI355X: mean and var are equal in every case, and rstd differs, by its last bit, in
    1 of 1 and 1024 of 1024 channels at R = 1, in 3 of 63 and 56 of 1024 at R = 2, and nowhere from R = 3 on. These are the
    channels with zero variance: the kernel adds eps as the float32 1e-5f (9.99999975e-6), and 1 / sqrt of that rounds to
    316.22778 where 1 / sqrt(1e-5) rounds to 316.22775."""
    z = pc.stats_input(R, C)
    rc, mean, rstd, var = bn_stats(hiplib, z)
    assert rc == 0
    differ = []
    for what, got, want in zip(("mean", "rstd", "var"), (mean, rstd, var), pc.stats_expected(z)):
        got = got.numpy()
        off = np.abs(got.astype(np.float64) - want.astype(np.float64))
        differ.append("%s %d" % (what, int((got != want).sum())))
        assert np.isfinite(got).all(), what
        assert (off <= np.spacing(np.abs(want)).astype(np.float64)).all(), (what, float(off.max()))
    print("R %d C %d: chunks %s, of %d values each differ from the float64 formulas' float32: %s"
          % (R, C, pc.stat_chunks(R), C, ", ".join(differ)))


def test_bn_stats_refuses_more_than_1024_channels(hiplib):
    rc, mean, _, _ = bn_stats(hiplib, torch.zeros(2, 1025))
    assert rc == hiplib.EINVAL and torch.isnan(mean).all()


def test_bn_stats_do_not_cancel_at_the_chunk_cap(hiplib):
    """z ~ N(100, 1), 70001 rows (256 chunks of 274, the last 131): test_batchnorm_statistics_do_not_cancel's criterion."""
    R, C = 70001, 64
    z = 100.0 + torch.randn(R, C, generator=torch.Generator().manual_seed(4))
    rc, mean, rstd, var = bn_stats(hiplib, z)
    assert rc == 0
    want = z.double().var(0, unbiased=False)
    rel = float(((var.double() - want) / want).abs().max())
    print("variance: worst relative error %.3g" % rel)
    assert rel <= 1e-5
    assert float((mean.double() - z.double().mean(0)).abs().max()) <= 1e-5
    assert float((rstd.double() * torch.sqrt(want + 1e-5) - 1).abs().max()) <= 1e-5


# ---- BatchNorm + ReLU + max-pool --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,S,C", pc.POOL_CASES, ids=[pc.gid(t) for t in pc.POOL_CASES])
def test_bn_relu_pool_exact(hiplib, G, S, C):
    """Bit-equal to relu(bn(z)).max and the first arg-max in float32 torch by the kernel's two steps, (z - mu) * rs, then
    * gamma + beta; a group that ends below zero everywhere (arg-max 0), a maximum at s = 0 and again at s = S - 1 (0 wins),
    a group whose only positive row is the last."""
    Z, mean, rstd, gamma, beta, made = pc.pool_inputs(G, S, C)
    a, want, want_arg = pc.pool_expected(Z, mean, rstd, gamma, beta)
    out = nans(G, C)
    arg = torch.full((G, C), -1, dtype=torch.int32, device="cuda")
    Zd, md, rd, gd, bd = (_dev(t) for t in (Z, mean, rstd, gamma, beta))
    hiplib.check(hiplib.fn("ossid_pn2_train_bn_relu_pool")(Zd.data_ptr(), G, S, C, md.data_ptr(), rd.data_ptr(), gd.data_ptr(),
                                                           bd.data_ptr(), out.data_ptr(), arg.data_ptr(), hiplib.stream()), "pool")
    assert torch.equal(out.cpu(), want)
    assert torch.equal(arg.cpu().long(), want_arg)
    arg = arg.cpu()
    assert (a[made["negative"]] == 0).all() and (arg[made["negative"]] == 0).all() and (out[made["negative"]] == 0).all()
    if "repeated" in made:
        g = made["repeated"]
        assert torch.equal(a[g, 0], a[g, S - 1]) and (a[g, 0] > 0).all() and (arg[g] == 0).all()
    if "last" in made:
        g = made["last"]
        assert (a[g, :S - 1] == 0).all() and (a[g, S - 1] > 0).all() and (arg[g] == S - 1).all()


# ---- ungroup ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,E,n,Cf,kind", pc.UNGROUP_CASES, ids=[pc.gid(t) for t in pc.UNGROUP_CASES])
def test_ungroup_exact(hiplib, B, E, n, Cf, kind):
    """Integer-valued dG: bit-equal to an int64 index_add_; targets without an entry are exact zeros over the NaN pre-fill."""
    idx, dG = pc.ungroup_inputs(B, E, n, Cf, kind)
    out = nans(B, n, Cf)
    dGd, idxd = _dev(dG), _dev(idx.int())
    hiplib.check(hiplib.fn("ossid_pn2_train_ungroup")(dGd.data_ptr(), idxd.data_ptr(), B, E, n, Cf, out.data_ptr(),
                                                      hiplib.stream()), "ungroup")
    out = out.cpu()
    assert torch.equal(out, pc.ungroup_expected(idx, dG, n))
    empty = torch.ones(B, n, dtype=torch.bool)
    empty.scatter_(1, idx, False)
    assert (out[empty] == 0).all()


# ---- whole model ------------------------------------------------------------------------------------------------------------------
def whole(name, hiplib):
    return tg._case(name, hiplib, shape=pc.WHOLE[name], inputs=pc.WHOLE_INPUTS[name])


@pytest.mark.parametrize("name", list(pc.WHOLE))
def test_whole_model_decisions_and_scores(hiplib, name):
    """test_decisions_and_scores at E1 (B = 2, M = npoint1 = npoint2 = 32), E2 (R3 = 544) and E3 (npoint 512 / 128, padded
    and truncated balls in one batch). Measured on the MI355X: 0 of 3.3 M (E1, e_fwd 4.3e-4), 0 of 36.9 M (E2, e_fwd 2.5e-5)
    and 1 of 25.8 M (E3, e_fwd 6.1e-3, margin 1.5e-7) decisions differ from float64's; the scores' ratio err / e32 is 0.74,
    0.76 and 0.23."""
    tg._check_decisions_and_scores(whole(name, hiplib), name)


KINDS = ("w", "gamma", "beta", "bias")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(pc.WHOLE))
def test_whole_model_gradients(hiplib, name, kind):
    """test_gradients_of_every_parameter at E1, E2, E3, the 35 tensors in four parts (12 weights, 11 gamma, 11 beta, the
    bias) so that one part can fail alone. Measured on the MI355X, the largest ratio err / e32 of each part:
        E1  w 0.75 (w11)   gamma 0.73 (gamma2)   beta 1.00 (beta10)   bias: err 0 = e32
        E2  w 0.92 (w2)    gamma 1.08 (gamma9)   beta 1.54 (beta2)    bias 1.00
        E3  w 0.42 (w1)    gamma 0.38 (gamma4)   beta 1.00 (beta10)   bias: err 0 = e32
    The bias gradient is the float64 sum of the dscores in row order, rounded once (test_bias_gradient_is_the_row_order_sum):
    the nearest float32 to the float64 result, so never further from it than the restatement is (E2: err 4.11e-9 = e32)."""
    tg._check_gradients(whole(name, hiplib), name, kind)


def row_order_sum(v, dtype=torch.float32):
    """The sum of v's elements taken one after the other in `dtype`, as float32."""
    want = torch.zeros((), dtype=dtype)
    for t in v.reshape(-1):
        want = want + t.to(dtype)
    assert want.dtype == dtype
    return want.float()


@pytest.mark.parametrize("name", list(pc.WHOLE))
def test_bias_gradient_is_the_row_order_sum(hiplib, name):
    """sum_kernel's one thread adds the dscores in row order in float64 and rounds once: bit for bit, at B = 2 and 17. (At
    B = 2 that is the float32 sum as well, which test_dropout_keeps_nothing asserts.)"""
    c = whole(name, hiplib)
    assert torch.equal(c["grads"][34].reshape(()), row_order_sum(c["dsc"], torch.float64))
    if c["dsc"].numel() == 2:
        assert torch.equal(c["grads"][34].reshape(()), row_order_sum(c["dsc"]))


@pytest.mark.parametrize("name", list(pc.WHOLE))
def test_whole_model_bit_reproducible(hiplib, name):
    tg._check_bit_reproducible(whole(name, hiplib))


@pytest.mark.parametrize("name", list(pc.WHOLE))
def test_whole_model_running_statistics(hiplib, name):
    tg._check_running_statistics(whole(name, hiplib), name)


def test_dropout_keeps_everything(hiplib):
    """E1 with the keep mask all ones and the head's dropout p = 0: scores and gradients within the usual bounds."""
    c = tg._case("E1-keep-all", hiplib, shape=pc.WHOLE["E1"], inputs=pc.WHOLE_INPUTS["E1"],
                 keep=lambda B: torch.ones(B, 256, dtype=torch.uint8), p_drop=0.0)
    assert float(c["gpu"].fc_layer[6].p) == 0.0 and bool(c["keep"].all())
    tg._check_decisions_and_scores(c, "E1-keep-all")
    tg._check_gradients(c, "E1-keep-all")


def test_dropout_keeps_nothing(hiplib):
    """E1 with the keep mask all zeros: the scores are the bias, every gradient but the bias's is zero exactly (of either
    sign), and the bias's is the float32 sum of dscores in row order."""
    B, M, np1, np2 = pc.WHOLE["E1"]
    g = torch.Generator().manual_seed(11)
    model = _model(np1, np2, 7).cuda().train()
    x = pc.WHOLE_INPUTS["E1"](B, M)
    dsc = torch.randn(B, 1, generator=g)
    scores, grads, _ = _gpu_step(model, x, torch.zeros(B, 256, dtype=torch.uint8), dsc)
    bias = _param_list(model)[34].detach().cpu()
    assert torch.equal(scores, bias.expand(B, 1))
    for n, t in zip(tg.GRAD_NAMES[:34], grads[:34]):
        assert bool((t == 0).all()), n
    assert torch.equal(grads[34].reshape(()), row_order_sum(dsc))


def test_constant_input(hiplib):
    """E1 with every point of every set the same point: every pre-activation channel has zero variance (the clamp, and
    rstd = 1 / sqrt(1e-5), are in play). Scores, gradients and running statistics are finite and within the usual bounds, and
    every pooling arg-max the GPU reports is 0.

    The usual gradient bound is a ratio to max|float64 gradient|. Here the two rows of the batch cancel, and the float64
    gradient of most tensors is exactly zero: for those the ratio does not exist. So the same bound is taken in absolute
    terms for all 35 tensors, err <= 4 x the float32 restatement's absolute error; where the float64 gradient and that error
    are both zero it pins an exact zero. Measured on the MI355X: the scores' ratio is 0.01; gamma0..10, beta0..8 and
    w0 are exactly zero on the GPU and in both restatements. w1..w8 are rounding noise in every one of the three (float64:
    9.5e7 at w1 falling to 8.9e-11 at w8 -- each BatchNorm below multiplies by rstd = 316 -- the GPU's and the float32
    restatement's are both far smaller, so err = e32 to three digits and the bound says little there); w9, w10 and beta9 are
    float32 noise on both sides (2.38e-4 against 2.42e-4, 9.5e-7 against 9.0e-7, 9.5e-7 against 9.5e-7)."""
    c = tg._case("E1-constant", hiplib, shape=pc.WHOLE["E1"], inputs=pc.constant_input)
    assert all(float(v.max()) <= 1e-20 for v in c["free64"]["var"])
    for m in range(3):
        assert int(c["dbg"]["argmax"][m].abs().max()) == 0, m
    assert bool(torch.isfinite(c["scores"]).all()) and all(bool(torch.isfinite(t).all()) for t in c["grads"])
    assert all(bool(torch.isfinite(t).all()) for t in c["stats1"][:22])
    for k in ("fps1", "ball1", "fps2", "ball2"):
        assert torch.equal(c["dbg"][k].cpu().long(), c["idx"][k]), k
    ref = float(c["s64"].abs().max())
    e32 = float((c["s32"].double() - c["s64"]).abs().max()) / ref
    err = float((c["scores"].double() - c["s64"]).abs().max()) / ref
    print("E1-constant: scores err %.3g, f32 restatement %.3g, ratio %.2f" % (err, e32, err / max(e32, 1e-30)))
    assert err <= 4 * e32
    fails = []
    for n, got, g64, g32 in zip(tg.GRAD_NAMES, c["grads"], c["g64"], c["g32"]):
        ref = float(g64.abs().max())
        err = float((got.double().reshape(g64.shape) - g64).abs().max())
        e32 = float((g32.double() - g64).abs().max())
        print("E1-constant %-8s max|f64| %.3g  err %.3g  f32 restatement %.3g" % (n, ref, err, e32))
        if not err <= 4 * e32:
            fails.append((n, err, e32))
    assert not fails, fails
    tg._check_running_statistics(c, "E1-constant")
