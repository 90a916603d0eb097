"""CPU side of the detection post-processing / AMSGrad edge tests: every case of tests/detect_post_cases.py exists once and
holds the edge it is named after (the premise figures are printed: tie counts per chunk, IoU gaps, the share of elements
on which AMSGrad and Adam differ), the restatement tests/ref_detect_post.py agrees with today's yardsticks on inputs
without edges (torch.topk, oracle/dtoid_oracle.py, the golden boxes of tests/golden/dtoid_head.npz), and the keep lists
written in closed form are the greedy restatement's."""
import os

import numpy as np
import pytest
import torch

import detect_post_cases as dc
import ref_detect_post as rd
from oracle import dtoid_oracle

GROUPS = tuple(dc.NAMES)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dtoid_head.npz")


@pytest.mark.parametrize("group", GROUPS)
def test_every_premise_holds(group):
    """Building asserts each premise; here: every named case exists exactly once, and its figures are printed."""
    cases = dc.BUILDERS[group]()
    assert sorted(c["name"] for c in cases) == sorted(dc.NAMES[group]) and len(set(dc.NAMES[group])) == len(dc.NAMES[group])
    for c in cases:
        print(c["name"], c["premise"])


def test_sizes_that_take_another_path():
    """The sizes the kernels branch on, read off the built cases."""
    tk = {(c["x"].size, c["k"]) for c in dc.topk_cases()}
    assert tk >= {(1, 1), (2, 2), (63, 63), (257, 1), (2048, 2048), (2049, 2048), (5000, 2047), (5000, 1025), (5000, 1024),
                  (512 * 2048 + 1, 1000)}
    assert max(k for _n, k in tk) == dc.TOPK_CAP and dc.topk_blocks(512 * 2048 + 1)[1] > dc.TOPK_CHUNK
    assert {c["deltas"].shape[0] * c["deltas"].shape[1] for c in dc.decode_cases()} == {1, 255, 256, 257}
    assert {c["deltas"].shape[1] for c in dc.decode_cases()} == {1, 3}
    ns = {len(c["boxes"]) for c in dc.nms_cases()}
    assert ns >= {1, 64, 65, dc.NMS_LDS_MAX, dc.NMS_LDS_MAX + 1, dc.NMS_MAX, 3000}
    assert {(c["n_t"], c["A"], c["k"]) for c in dc.post_cases()} == {(1, 3, 3), (2, 5, 10), (3, 96, 64), (21, 288, 288)}
    assert {c["premise"]["seg_row"] % 4 for c in dc.emit_cases()} == {0, 3}
    assert {c["src"].shape[1] // 4 > 1024 * 256 for c in dc.gather_cases()} == {False, True}
    assert {c["n"] for c in dc.amsgrad_cases()} == {4, 4 * dc.AMS_GRID + 4}


# ---- the restatement against today's yardsticks, on inputs without edges ---------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 1), (257, 7), (5000, 1000), (40000, 2048)])
def test_topk_restatement_equals_torch_topk(n, k):
    """Values as torch.topk gives them on finite scores with ties (torch leaves the order among equal values open, so the
    indices are checked for what both promise: they point at the values)."""
    g = torch.Generator().manual_seed(n + k)
    x = (torch.randn(n, generator=g) * 8).round() / 8
    vals, idx = rd.topk(x.numpy(), k)
    assert np.array_equal(vals, torch.topk(x, k).values.numpy()) and np.array_equal(x.numpy()[idx], vals)
    assert all(a > b or (a == b and i < j) for a, b, i, j in zip(vals[:-1], vals[1:], idx[:-1], idx[1:]))
    cut = vals[-1]
    assert np.array_equal(idx[vals == cut], np.flatnonzero(x.numpy() == cut)[:int((vals == cut).sum())])     # lowest indices at the cut


def test_order_key_is_the_total_order():
    x = np.array([0xFFC00000, 0xFF800000, 0xC0000000, 0x80000001, 0x80000000, 0, 1, 0x3F800000, 0x7F800000, 0x7FC00000,
                  0x7FC00001], np.uint32).view(np.float32)
    assert np.all(np.diff(rd.order_key(x).astype(np.int64)) > 0)


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_nms_restatement_equals_the_oracle(n):
    boxes, scores = dc.random_boxes(max(n, 8), n)
    boxes, scores = boxes[:n], scores[:n]
    order = torch.sort(torch.from_numpy(scores), descending=True, stable=True).indices.numpy()
    want = dtoid_oracle.nms(torch.from_numpy(boxes), torch.from_numpy(scores), 0.5).numpy()
    assert np.array_equal(order[rd.nms_sorted(boxes[order], 0.5)], want)


def test_decode_restatement_equals_the_oracle_and_the_golden_boxes():
    """Against the float32 oracle and the reference's own BBoxTransform output (clipped here as ClipBoxes does): the float32
    results lie within 4 roundings of the largest coordinate of the float64 restatement."""
    G = np.load(GOLDEN)
    want = rd.decode_clip(G["anchors"].reshape(-1, 4), G["reg"], 40, 32)
    tol = 4 * 2.0 ** -24 * np.abs(want).max()
    o32 = dtoid_oracle.decode_clip_boxes(torch.from_numpy(G["anchors"]), torch.from_numpy(G["reg"]), 40, 32).numpy()
    ref = torch.from_numpy(G["boxes"]).clone()
    ref[..., 0].clamp_(min=0), ref[..., 1].clamp_(min=0), ref[..., 2].clamp_(max=40), ref[..., 3].clamp_(max=32)
    e_o, e_g = np.abs(o32 - want).max(), np.abs(ref.numpy() - want).max()
    print("decode: f32 oracle off by %.3g, golden boxes by %.3g, 4 roundings = %.3g" % (e_o, e_g, tol))
    assert want.shape == o32.shape == tuple(ref.shape) and e_o <= tol and e_g <= tol
    for c in dc.decode_cases():                                     # ... and the float32 oracle on the edge cases
        assert np.abs(dc.decode_f32(c["anchors"], c["deltas"]) - c["want"]).max() <= 4 * 2.0 ** -24 * np.abs(c["want"]).max(), c["name"]


@pytest.mark.parametrize("lr,wd", [(1e-2, 1e-3), (1e-4, 1e-6)])
def test_amsgrad_restatement_equals_torch_adam_in_float64(lr, wd):
    rng = np.random.default_rng(5)
    p0, grads = rng.normal(size=257), [rng.normal(size=257) * s for s in dc.AMS_SCHEDULE]
    for steps in (1, 3, 5):
        want = dtoid_oracle.amsgrad_reference(torch.from_numpy(p0), [torch.from_numpy(g) for g in grads], lr, wd, steps=steps)
        assert want.dtype == torch.float64
        got = rd.amsgrad(p0, grads[:steps], lr, (0.9, 0.999), 1e-8, wd)[-1][0]
        assert np.abs(got - want.numpy()).max() <= 1e-13
    # the state buffers, and a late first step, against torch's own state
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=lr, weight_decay=wd, amsgrad=True)
    p.grad = torch.from_numpy(grads[0])
    opt.step()
    one = rd.amsgrad(p0, grads[:1], lr, (0.9, 0.999), 1e-8, wd)[0]
    s = opt.state[p]
    for got, want in zip(one, (p.data, s["exp_avg"], s["exp_avg_sq"], s["max_exp_avg_sq"])):
        assert np.abs(got - want.numpy()).max() <= 1e-13 * max(1.0, float(want.abs().max()))
    h = dict(lr=lr, wd=wd, betas=(0.9, 0.999), eps=1e-8)
    late32 = dc.amsgrad_f32(p0, grads[:1], h, first_step=100000)[0]
    late64 = rd.amsgrad(p0, grads[:1], lr, (0.9, 0.999), 1e-8, wd, first_step=100000)[0]
    assert all(dc.rel_err(a, b) <= 4 * 2.0 ** -24 for a, b in zip(late32[1:], late64[1:]))
    assert np.abs(late32[0] - late64[0]).max() <= 2.0 ** -23 * np.abs(p0).max()


def test_adam_and_amsgrad_part_only_under_the_running_maximum():
    """The switch of the restatement: identical while exp_avg_sq rises, different once it has fallen below its maximum."""
    c = dc.by_name("amsgrad")["a_n4_lr1e-2"]
    h = c["hyper"]
    adam = rd.amsgrad(c["p0"], c["grads"], h["lr"], h["betas"], h["eps"], h["wd"], use_max=False)
    same = [np.array_equal(a[0], w[0]) for a, w in zip(adam, c["want"])]
    assert same == [True, True, False, False, False]


# ---- closed forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in dc.NAMES["nms"] if n != "n_random_3000"])
def test_closed_form_keep_lists_are_the_greedy_ones(name):
    c = dc.by_name("nms")[name]
    for thr, keep in c["want"].items():
        assert np.array_equal(rd.nms_sorted(c["boxes"], thr), keep), (name, thr)


def test_detect_emit_restatement_is_the_list_of_the_reference_lines():
    """network.py:564-575 written out with plain indexing on an emit case."""
    c = dc.emit_cases()[0]
    for count in (0, 3, 5):
        s, b, o, seg, heat = rd.detect_emit(c["vals"], c["idx"], c["boxes"], c["keep"], count, c["A"], c["seg"], c["heat"], False)
        ids = c["keep"][:count].astype(np.int64)
        obj = (c["idx"] // c["A"])[ids]
        assert np.array_equal(s, c["vals"][ids]) and np.array_equal(b, c["boxes"][ids]) and np.array_equal(o[:, 0], obj)
        assert np.array_equal(seg, c["seg"][obj], equal_nan=True) and np.array_equal(heat, c["heat"][obj], equal_nan=True)
