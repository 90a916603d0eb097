"""The non-convolution entries of csrc/dtoid.hip at their edges: every case of tests/detect_post_cases.py through ossid_topk,
_decode_clip_boxes, _nms, _detect_post, _detect_emit, _gather_rows and _amsgrad_step against the restatement
tests/ref_detect_post.py.

Decisions (top-k indices, keep lists and counts, template indices, gathered rows) are exact. Copied values (top-k values,
emitted scores, heat rows, seg rows without the sigmoid) are bit-equal as int32, so NaN payloads and the sign of zero count.
Computed values (decoded boxes, the sigmoid, the AMSGrad buffers) follow the `_bounded` rule of tests/test_pn2_train_gpu.py
with its floor: max|got - f64| / max|f64| <= 4 x max(the same figure of a float32 torch CPU computation on the same inputs,
2^-24). err, e32 and their ratio are printed per case. Outputs carry guard elements behind them, workspaces are handed over
filled with 0xFF bytes, and an entry that refuses its arguments leaves every output as it was."""
import numpy as np
import pytest
import torch

import detect_post_cases as dc
import ref_detect_post as rd
from ossid_code_amd.dtoid import ops

pytestmark = pytest.mark.gpu

G = 8                                                   # guard rows behind every output
GI, GF = -7, 777.0
f32, f64 = np.float32, np.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def guard(rows, tail, dtype):
    """an output of `rows` rows (+ G guard rows), filled with the guard value"""
    return torch.full((rows + G,) + tuple(tail), GF if dtype == torch.float32 else GI, dtype=dtype, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def untouched(a, start=0):
    a = a[start:]
    return bool(np.all(a == (GF if a.dtype.kind == "f" else GI)))


def same(a, b):
    """equal as bit patterns"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dirty(nbytes):
    """a workspace of nbytes + 64 guard bytes, every byte 0xFF"""
    return torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device="cuda")


def clean_tail(ws, nbytes):
    return bool((ws[nbytes:] == 0xFF).all().item())


def bounded(got, want64, ref32, what):
    """max|got - f64| / max|f64| <= 4 x max(the same for the float32 torch computation, one float32 rounding)"""
    want64 = np.asarray(want64, dtype=f64)
    ref = float(np.abs(want64).max())
    if ref == 0.0:
        assert not np.any(got), what
        return 0.0
    e32 = float(np.abs(np.asarray(ref32, dtype=f64) - want64).max()) / ref
    err = float(np.abs(np.asarray(got, dtype=f64) - want64).max()) / ref
    ratio = err / max(e32, dc.FLOOR)
    print("%s: err %.3g, f32 torch %.3g, ratio %.2f" % (what, err, e32, ratio))
    assert err <= dc.bound(e32), what
    return ratio


# ---- top-k ----------------------------------------------------------------------------------------------------------------
def run_topk(lib, x, k, ws=None, expect=0):
    n = x.size
    wsb = lib.fn("ossid_topk_workspace_bytes")(n, k)
    if ws is None:
        ws = dirty(wsb)
    xd = dev(x)
    vals, idx = guard(min(k, 4096), (), torch.float32), guard(min(k, 4096), (), torch.int64)
    rc = lib.fn("ossid_topk")(xd.data_ptr(), n, k, ws.data_ptr(), wsb, vals.data_ptr(), idx.data_ptr(), lib.stream())
    assert rc == expect
    vals, idx = host(vals), host(idx)
    if expect:
        assert untouched(vals) and untouched(idx)
        return None
    assert untouched(vals, k) and untouched(idx, k) and clean_tail(ws, max(wsb, ws.numel() - 64))
    return vals[:k], idx[:k]


@pytest.mark.parametrize("name", dc.NAMES["topk"])
def test_topk(hiplib, name):
    """Indices exact (equal values lowest index first, also at the cut), values bit-equal (NaN payloads, signed zeros and
    denormals come through), from a workspace full of 0xFF; two runs and the Python wrapper give the same bits."""
    c = dc.by_name("topk")[name]
    print(c["premise"])
    vals, idx = run_topk(hiplib, c["x"], c["k"])
    assert np.array_equal(idx, c["want"]["indices"]) and same(vals, c["want"]["values"])
    again = run_topk(hiplib, c["x"], c["k"])
    assert same(again[0], vals) and same(again[1], idx)
    v2, i2 = ops.topk_scores(dev(c["x"]), c["k"])
    assert same(host(v2), vals) and same(host(i2), idx)


def test_topk_workspace_reuse_and_refusals(hiplib):
    """One workspace, dirtied once, serves three different inputs in turn: each call returns its own answer. k > n, k above
    the cap, k = 0 and a workspace one byte short are refused with the outputs untouched."""
    by = dc.by_name("topk")
    ws = dirty(hiplib.fn("ossid_topk_workspace_bytes")(5000, dc.TOPK_CAP))
    for name in ("t_n5000_k2047", "t_tie_run_across_chunks", "t_n63_k63", "t_bin_boundary_one_tie", "t_n5000_k2047"):
        c = by[name]
        vals, idx = run_topk(hiplib, c["x"], c["k"], ws=ws)
        assert np.array_equal(idx, c["want"]["indices"]) and same(vals, c["want"]["values"]), name
    x = by["t_n5000_k1024"]["x"]
    for n, k in ((100, 101), (5000, dc.TOPK_CAP + 1), (100, 0)):
        run_topk(hiplib, x[:n], k, expect=dc.EINVAL)
    xd, wsb = dev(x), hiplib.fn("ossid_topk_workspace_bytes")(5000, 10)
    vals, idx = guard(10, (), torch.float32), guard(10, (), torch.int64)
    rc = hiplib.fn("ossid_topk")(xd.data_ptr(), 5000, 10, ws.data_ptr(), wsb - 1, vals.data_ptr(), idx.data_ptr(), hiplib.stream())
    assert rc == dc.EINVAL and untouched(host(vals)) and untouched(host(idx))


# ---- decode + clip --------------------------------------------------------------------------------------------------------
def run_decode(lib, anchors, deltas, expect=0):
    R, A = deltas.shape[:2]
    a, d = dev(anchors), dev(deltas) if R else guard(0, (A, 4), torch.float32)
    out = guard(R, (A, 4), torch.float32)
    rc = lib.fn("ossid_decode_clip_boxes")(a.data_ptr(), d.data_ptr(), R, A, dc.IMG_W, dc.IMG_H, out.data_ptr(), lib.stream())
    assert rc == expect
    out = host(out)
    assert untouched(out, R)
    return out[:R]


@pytest.mark.parametrize("name", dc.NAMES["decode"])
def test_decode_clip(hiplib, name):
    """R A in {1, 255, 256, 257}, A in {1, 3} (anchor i % A, one without a size), and the rows with a closed form: exactly on the
    frame, wholly left of / above it (x2 < x1 stays), exp overflowing to inf (0 .. img_w) and underflowing (width 0).
    Measured ratios err / max(e32, 2^-24) on an MI355X: 0.00 .. 0.29 (err equals float32 torch's own, 1.7e-8, in every case)."""
    c = dc.by_name("decode")[name]
    print(c["premise"])
    got = run_decode(hiplib, c["anchors"], c["deltas"])
    bounded(got, c["want"], dc.decode_f32(c["anchors"], c["deltas"]), name)
    assert same(host(ops.decode_clip_boxes(dev(c["anchors"]), dev(c["deltas"]), dc.IMG_W, dc.IMG_H)), got)
    flat, want = got.reshape(-1, 4), c["want"].reshape(-1, 4)
    p = c["premise"]
    if p.get("exact_frame"):
        assert flat[0].tolist() == list(dc.FRAME)
    if "exp_overflow" in p:
        rows = {nm: int(np.flatnonzero((want == np.array(p[nm])).all(1))[0]) for nm, _d, _f in dc.DECODE_SPECIALS}
        for nm, _d, holds in dc.DECODE_SPECIALS:                    # the closed-form property holds on the device's box too
            assert holds(flat[rows[nm]].astype(f64)), (nm, flat[rows[nm]])
        assert flat[rows["exp_overflow"]].tolist() == want[rows["exp_overflow"]].tolist()
    assert np.isfinite(got).all()


def test_decode_clip_zero_rows(hiplib):
    assert run_decode(hiplib, dc.decode_cases()[0]["anchors"], np.zeros((0, 1, 4), f32)).shape[0] == 0
    c = dc.decode_cases()[1]
    out = guard(4, (1, 4), torch.float32)
    rc = hiplib.fn("ossid_decode_clip_boxes")(dev(c["anchors"]).data_ptr(), dev(c["deltas"]).data_ptr(), 4, 0, dc.IMG_W, dc.IMG_H,
                                             out.data_ptr(), hiplib.stream())
    assert rc == dc.EINVAL and untouched(host(out))


# ---- NMS ------------------------------------------------------------------------------------------------------------------
def run_nms(lib, boxes, thr, expect=0, n=None):
    n = len(boxes) if n is None else n
    wsb = lib.fn("ossid_nms_workspace_bytes")(min(n, dc.NMS_MAX))
    ws = dirty(wsb)
    b = dev(np.asarray(boxes, dtype=f32)) if len(boxes) else guard(0, (4,), torch.float32)
    keep, count = guard(n, (), torch.int32), guard(1, (), torch.int32)
    rc = lib.fn("ossid_nms")(b.data_ptr(), n, float(thr), ws.data_ptr(), wsb, keep.data_ptr(), count.data_ptr(), lib.stream())
    assert rc == expect
    keep, count = host(keep), host(count)
    if expect:
        assert untouched(keep) and untouched(count)
        return None
    assert untouched(count, 1) and 0 <= count[0] <= n and untouched(keep, int(count[0])) and clean_tail(ws, wsb)
    return keep[:int(count[0])]


@pytest.mark.parametrize("name", dc.NAMES["nms"])
def test_nms(hiplib, name):
    """The keep list and its count, exact, at every threshold of the case (0.5 everywhere; 1 for identical boxes, 0 for
    touching ones), from a mask workspace full of 0xFF; nothing is written behind the count."""
    c = dc.by_name("nms")[name]
    print(c["premise"])
    if name == "n_random_3000":
        got = ops.nms(dev(c["boxes"]), dev(c["scores"]), 0.5)
        assert got.dtype == torch.long and np.array_equal(host(got), c["want"][0.5])
        sorted_boxes = c["boxes"][c["order"]]
        assert np.array_equal(c["order"][run_nms(hiplib, sorted_boxes, 0.5)], c["want"][0.5])
        return
    for thr, want in c["want"].items():
        got = run_nms(hiplib, c["boxes"], thr)
        assert np.array_equal(got, want), (name, thr, len(got), len(want))
    assert np.array_equal(host(ops.nms(dev(c["boxes"]), -torch.arange(len(c["boxes"]), device="cuda").float(), 0.5)), c["want"][0.5])


def test_nms_size_limits(hiplib):
    """n = 16385 is refused with the outputs untouched; n = 0 writes a count of 0 and nothing else."""
    boxes = dc.by_name("nms")["n_chain_w6_16384"]["boxes"]
    run_nms(hiplib, np.concatenate([boxes, boxes[:1]]), 0.5, expect=dc.EINVAL)
    assert len(run_nms(hiplib, boxes[:0], 0.5)) == 0


# ---- detect_post ----------------------------------------------------------------------------------------------------------
def poisoned_state(c):
    st = ops.DetectPost(c["n_t"] * c["A"], c["k"], c["A"], torch.device("cuda"))
    for t in (st.scores, st.indices, st.boxes, st.keep, st.count, st.ws):
        t.view(torch.uint8).fill_(0xFF)
    return st


def post(c, st):
    return ops.detect_post(dev(c["cls"]), dev(c["deltas"]), dev(c["anchors"])[None], dc.POST_W, dc.POST_H, c["k"], dc.POST_THR, state=st)


def read_post(st):
    torch.cuda.synchronize()
    n = int(st.count.item())
    return dict(scores=st.scores.cpu().numpy(), indices=st.indices.cpu().numpy(), boxes=st.boxes.cpu().numpy(),
                keep=st.keep.cpu().numpy()[:n], count=n)


@pytest.mark.parametrize("name", dc.NAMES["post"])
def test_detect_post_stage_by_stage(hiplib, name):
    """Top-k on the strided object column (the class-0 column holds NaN and larger values and is never read): values bit-equal,
    flat indices exact. Boxes of the survivors: within the bound of the float64 decode, and bit-equal to
    ossid_decode_clip_boxes gathered at the same indices. NMS: the greedy restatement run on the device's own boxes (whose
    IoUs, asserted here, stay 2e-6 clear of the threshold) gives the keep list and the count. The state starts full of 0xFF.
    Measured box ratios on an MI355X: 0.86 .. 1.00 (err 5.1e-8 .. 9.7e-8, equal to float32 torch's own in every case)."""
    c = dc.by_name("post")[name]
    print(c["premise"])
    st = poisoned_state(c)
    assert post(c, st) is st
    got, want = read_post(st), c["want"]
    assert same(got["scores"], want["values"]) and np.array_equal(got["indices"], want["indices"])
    dec32 = dc.decode_f32(c["anchors"], c["deltas"], dc.POST_W, dc.POST_H).reshape(-1, 4)[want["indices"]]
    bounded(got["boxes"], want["boxes"], dec32, name + " boxes")
    full = host(ops.decode_clip_boxes(dev(c["anchors"]), dev(c["deltas"]), dc.POST_W, dc.POST_H)).reshape(-1, 4)
    assert same(got["boxes"], full[want["indices"]])
    k = c["k"]
    if k > 1:
        gap = float(np.nanmin(np.abs(rd.iou(got["boxes"][:, None], got["boxes"][None])[np.triu_indices(k, 1)] - dc.POST_THR)))
        print("min |IoU - thr| on the device's boxes: %.3g" % gap)
        assert gap >= dc.RANDOM_NMS_GAP                             # the premise, on the boxes the NMS stage really saw
    keep = rd.nms_sorted(got["boxes"], dc.POST_THR)
    assert got["count"] == len(keep) and np.array_equal(got["keep"], keep)
    assert np.array_equal(got["indices"][got["keep"]] // c["A"], want["indices"][want["keep"]] // c["A"])     # template of each detection
    if "placed" in c["premise"]:
        assert got["indices"][:3].tolist() == c["premise"]["placed"] and got["keep"][:2].tolist() == [0, 1] and 2 in got["keep"]


@pytest.mark.parametrize("t,a,k", [(1, 3, 3), (2, 5, 10), (3, 96, 64), (21, 288, 288)])
def test_detect_post_state_reuse(hiplib, t, a, k):
    """One DetectPost serves different inputs of the same sizes in turn; each result is, bit for bit, what a fresh state
    gives: no trace of the call before."""
    tag = "t%d_a%d_k%d" % (t, a, k)
    by = dc.by_name("post")
    names = [n for n in ("p_random_" + tag, "p_equal_" + tag, "p_placed_" + tag, "p_random_" + tag) if n in by]
    st = None
    for n in names:
        c = by[n]
        st = post(c, st if st is not None else poisoned_state(c))
        got, fresh = read_post(st), read_post(post(c, poisoned_state(c)))
        assert all(same(got[q], fresh[q]) for q in ("scores", "indices", "boxes", "keep")) and got["count"] == fresh["count"], n


def test_detect_post_refusals(hiplib):
    """k > n, k above the cap, n not a multiple of A, a score stride of 0 and a workspace one byte short: EINVAL, and the
    outputs stay as they were."""
    c = dc.by_name("post")["p_random_t21_a288_k288"]
    n, A, k = c["n_t"] * c["A"], c["A"], c["k"]
    cls, reg, anc = dev(c["cls"]), dev(c["deltas"]), dev(c["anchors"])
    wsb = hiplib.fn("ossid_detect_post_workspace_bytes")(n, dc.TOPK_CAP)
    ws = dirty(wsb)
    for what, (n_, stride, k_, A_, wsb_) in dict(k_over_n=(200, 2, 201, 5, wsb), k_over_cap=(n, 2, dc.TOPK_CAP + 1, A, wsb),
                                                 n_not_rows_of_A=(n - 1, 2, k, A, wsb), stride_0=(n, 0, k, A, wsb),
                                                 short_workspace=(n, 2, k, A, hiplib.fn("ossid_detect_post_workspace_bytes")(n, k) - 1)).items():
        o = [guard(k, (), torch.float32), guard(k, (), torch.int64), guard(k, (4,), torch.float32), guard(k, (), torch.int32),
             guard(1, (), torch.int32)]
        rc = hiplib.fn("ossid_detect_post")(cls.data_ptr() + 4, n_, stride, k_, anc.data_ptr(), reg.data_ptr(), A_, dc.POST_W, dc.POST_H,
                                           0.5, ws.data_ptr(), wsb_, *[t.data_ptr() for t in o], hiplib.stream())
        assert rc == dc.EINVAL and all(untouched(host(t)) for t in o), what


# ---- detect_emit ----------------------------------------------------------------------------------------------------------
def emit_state(c):
    st = ops.DetectPost(c["k"] * 2, c["k"], c["A"], torch.device("cuda"))
    st.scores.copy_(dev(c["vals"])), st.indices.copy_(dev(c["idx"])), st.boxes.copy_(dev(c["boxes"]))
    st.keep.zero_()
    st.keep[:c["n_keep"]] = dev(c["keep"])
    st.count.fill_(c["n_keep"])
    return st


def run_emit(lib, c, st, count, seg_row, heat_row, sig, expect=0, rows=None):
    """ossid_detect_emit itself, every output with guard rows behind it; a row count of 0 goes with null pointers"""
    rows = count if rows is None else rows
    seg, heat = dev(c["seg"]), dev(c["heat"])
    o = [guard(rows, (), torch.float32), guard(rows, (4,), torch.float32), guard(rows, (), torch.float32),
         guard(rows, (max(seg_row, 1),), torch.float32), guard(rows, (max(heat_row, 1),), torch.float32)]
    rc = lib.fn("ossid_detect_emit")(st.scores.data_ptr(), st.indices.data_ptr(), st.boxes.data_ptr(), st.keep.data_ptr(), count, st.A,
                                     seg.data_ptr() if seg_row else None, seg_row, heat.data_ptr() if heat_row else None, heat_row, sig,
                                     o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr() if seg_row else None,
                                     o[4].data_ptr() if heat_row else None, lib.stream())
    assert rc == expect
    o = [host(t) for t in o]
    if expect:
        assert all(untouched(t) for t in o)
        return None
    assert all(untouched(t, rows) for t in o) and (seg_row or untouched(o[3])) and (heat_row or untouched(o[4]))
    return [t[:rows] for t in o]


@pytest.mark.parametrize("name", dc.NAMES["emit"])
def test_detect_emit(hiplib, name):
    """Rows of the first `count` kept candidates, in order, for count = 0, count below the keep count, and all of it: scores,
    boxes and heat rows bit-equal (a NaN and a -0.0 among them), template index = flat index / A, seg rows bit-equal without
    the sigmoid and within the bound of float64 with it (inputs of +-100 give 1 and 0, never NaN). Seg rows of 35 floats take
    the scalar path, of 48 the float4 path; a seg or heat row count of 0 leaves that output untouched.
    Measured sigmoid ratios on an MI355X: 1.00 in every case (err 6.1e-8 .. 6.4e-8, float32 torch's own)."""
    c = dc.by_name("emit")[name]
    print(c["premise"])
    st = emit_state(c)
    seg_row, heat_row = c["premise"]["seg_row"], c["premise"]["heat_row"]
    segs, heats = c["seg"].reshape(len(c["seg"]), -1), c["heat"].reshape(len(c["heat"]), -1)
    for count in (0, 3, c["n_keep"]):
        for sig in (0, 1):
            want = rd.detect_emit(c["vals"], c["idx"], c["boxes"], c["keep"], count, c["A"], segs, heats, bool(sig))
            got = run_emit(hiplib, c, st, count, seg_row, heat_row, sig)
            assert same(got[0], want[0]) and same(got[1], want[1]) and same(got[2], want[2][:, 0]) and same(got[4], want[4])
            if not sig:
                assert same(got[3], want[3])
            elif count:
                src = rd.gather_rows(segs, want[2][:, 0].astype(np.int64), False)
                bounded(got[3], want[3], torch.sigmoid(torch.from_numpy(src.astype(f32))).numpy(), "%s count %d sigmoid" % (name, count))
                assert not np.isnan(got[3]).any() and (got[3][src == 100.0] == 1.0).all() and (got[3][src == -100.0] < 1e-40).all()
                assert (src == 100.0).any() and (src == -100.0).any()
            via = ops.detect_emit(st, count, dev(c["seg"]), dev(c["heat"]), seg_sigmoid=bool(sig))
            assert [tuple(t.shape) for t in via] == [(count,), (count, 4), (count, 1), (count,) + c["seg"].shape[1:], (count,) + c["heat"].shape[1:]]
            assert all(same(host(t).reshape(g.shape), g) for t, g in zip(via, got))
    full = run_emit(hiplib, c, st, c["n_keep"], seg_row, heat_row, 0)
    no_seg = run_emit(hiplib, c, st, c["n_keep"], 0, heat_row, 1)
    no_heat = run_emit(hiplib, c, st, c["n_keep"], seg_row, 0, 0)
    assert all(same(no_seg[i], full[i]) for i in (0, 1, 2, 4)) and all(same(no_heat[i], full[i]) for i in (0, 1, 2, 3))
    run_emit(hiplib, c, st, 65536, seg_row, heat_row, 0, expect=dc.EINVAL, rows=1)


# ---- gather_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.NAMES["gather"])
def test_gather_rows(hiplib, name):
    """Rows of 4 floats, and of 4 (1024 256 + 3) floats (past what one trip of a row's grid covers), repeated and descending
    indices: copies bit-equal (a NaN and a -0.0 among them), the sigmoid within the bound (+-100 give 1 and 0); k = 0 writes
    nothing. Measured sigmoid ratios on an MI355X: 0.84 and 1.00 (err 5.0e-8 and 8.5e-8)."""
    c = dc.by_name("gather")[name]
    print(c["premise"])
    src, idx = c["src"], c["idx"]
    k, row = len(idx), src.shape[1]
    srcd, idxd = dev(src), dev(idx)
    for sig in (0, 1):
        out = guard(k, (row,), torch.float32)
        assert hiplib.fn("ossid_gather_rows")(srcd.data_ptr(), len(src), row, idxd.data_ptr(), k, sig, out.data_ptr(), hiplib.stream()) == 0
        out = host(out)
        assert untouched(out, k)
        if not sig:
            assert same(out[:k], src[idx])
        else:
            ok = ~np.isnan(src[idx])
            bounded(out[:k][ok], rd.sigmoid(src[idx])[ok], torch.sigmoid(torch.from_numpy(src[idx])).numpy()[ok], name + " sigmoid")
            assert np.array_equal(np.isnan(out[:k]), ~ok) and (out[:k][src[idx] == 100.0] == 1.0).all() and (out[:k][src[idx] == -100.0] < 1e-40).all()
        assert same(host(ops.gather_rows(srcd, idxd, sigmoid=bool(sig))), out[:k])
    out = guard(1, (row,), torch.float32)
    assert hiplib.fn("ossid_gather_rows")(srcd.data_ptr(), len(src), row, idxd.data_ptr(), 0, 0, out.data_ptr(), hiplib.stream()) == 0
    assert untouched(host(out))


# ---- AMSGrad ---------------------------------------------------------------------------------------------------------------
POISON = np.int32(0x7FC0DEAD)                           # a NaN with a payload, in the 64 floats behind each buffer
AMS_NAMES = ("p - p0", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def ams_buffers(n, p0, state=None):
    """param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq of n floats, each with AMS_PAD poisoned floats behind it"""
    bufs = []
    for q in range(5):
        a = np.zeros(n + dc.AMS_PAD, f32)
        a[n:] = np.full(dc.AMS_PAD, POISON, np.int32).view(f32)
        bufs.append(a)
    bufs[0][:n] = p0
    if state is not None:
        for b, s in zip(bufs[2:], state):
            b[:n] = s
    return [dev(b) for b in bufs]


def ams_step(lib, bufs, n, g, h, step, expect=0):
    if g is not None:
        bufs[1][:len(g)].copy_(dev(g))
    b1, b2 = h["betas"]
    rc = lib.fn("ossid_amsgrad_step")(bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(),
                                      n, h["lr"], b1, b2, h["eps"], h["wd"], step, lib.stream())
    assert rc == expect
    out = [host(b) for b in bufs]
    for i in (0, 2, 3, 4):
        assert np.all(out[i][n:].view(np.int32) == POISON)          # the floats behind the buffer, bit for bit
    return [out[i][:n] for i in (0, 2, 3, 4)]


@pytest.mark.parametrize("name", dc.NAMES["amsgrad"])
def test_amsgrad_five_steps(hiplib, name):
    """g_t = g s_t, s = (1, 1, .01, .01, .01): from step 3 on exp_avg_sq lies under its running maximum, and dropping the
    maximum would move the parameters by more than 100 bounds on >= 90 % of the elements (premise). After every step the
    device's p - p0, exp_avg, exp_avg_sq and max_exp_avg_sq are within the bound of the float64 restatement, e32 from
    torch.optim.Adam(amsgrad=True) in float32 on the CPU; n = 4 and n = 4 (2048 256) + 4 (second trip of the grid-stride
    loop); the 64 floats behind every buffer keep their bits. The hyper-parameters are the float32 values the entry receives.
    Measured ratios on an MI355X over the four cases and five steps: p - p0 0.69 .. 2.09, exp_avg 0.38 .. 2.84, exp_avg_sq
    0.51 .. 1.40, max_exp_avg_sq 0.51 .. 1.28 (bound: 4)."""
    c = dc.by_name("amsgrad")[name]
    print(c["premise"])
    n, h, p0 = c["n"], c["hyper"], c["p0"].astype(f64)
    bufs = ams_buffers(n, c["p0"])
    for t, g in enumerate(c["grads"], 1):
        got = ams_step(hiplib, bufs, n, g, h, t)
        want, r32 = c["want"][t - 1], c["ref32"][t - 1]
        bounded(got[0].astype(f64) - p0, want[0] - p0, r32[0].astype(f64) - p0, "%s step %d %s" % (name, t, AMS_NAMES[0]))
        for q in (1, 2, 3):
            bounded(got[q], want[q], r32[q], "%s step %d %s" % (name, t, AMS_NAMES[q]))


def test_amsgrad_sizes_refused_or_empty(hiplib):
    """n = 0 is accepted and writes nothing; n % 4 != 0 and step < 1 are refused; the buffers keep their bits."""
    c = dc.by_name("amsgrad")["a_n4_lr1e-2"]
    for n, step, rc in ((0, 1, 0), (3, 1, dc.EINVAL), (6, 1, dc.EINVAL), (4, 0, dc.EINVAL), (4, -1, dc.EINVAL)):
        bufs = ams_buffers(8, np.arange(8, dtype=f32) + 1)
        bufs[1][:8].fill_(1.0)
        before = [host(b).copy() for b in bufs]
        b1, b2 = c["hyper"]["betas"]
        got = hiplib.fn("ossid_amsgrad_step")(*[b.data_ptr() for b in bufs], n, c["hyper"]["lr"], b1, b2, c["hyper"]["eps"], c["hyper"]["wd"],
                                             step, hiplib.stream())
        assert got == rc and all(same(host(b), a) for b, a in zip(bufs, before)), (n, step)


@pytest.mark.parametrize("lr,wd", [(1e-2, 1e-3), (1e-4, 1e-6)])
def test_amsgrad_zero_gradient_late_step_and_repeatability(hiplib, lr, wd):
    """g = 0: p != 0 moves by weight decay alone (within the bound of float64), p = 0 stays exactly 0 with every buffer 0 (the
    denominator is eps, nothing becomes NaN). step = 100000 on fresh state follows the restatement called with that step number.
    Two runs from the same state are bit-equal. Measured ratios on an MI355X: 0.80 .. 1.00."""
    h = dc.hyper(lr, wd)
    n = 1024
    rng = np.random.default_rng(17)
    p0 = rng.normal(size=n).astype(f32)
    p0[::4] = 0.0
    zero = np.zeros(n, f32)
    got = ams_step(hiplib, ams_buffers(n, p0), n, zero, h, 1)
    want = rd.amsgrad(p0, [zero], h["lr"], h["betas"], h["eps"], h["wd"])[0]
    r32 = dc.amsgrad_f32(p0, [zero], h)[0]
    assert all(not np.isnan(a).any() and not a[::4].any() for a in got)
    moved = (got[0] != p0).mean()
    print("zero gradient: %.0f %% of the parameters moved" % (100 * moved))
    assert moved >= 0.7 and float(np.abs(want[0] - p0)[p0 != 0].min()) > 0
    bounded(got[0].astype(f64) - p0, want[0] - p0, r32[0].astype(f64) - p0, "zero gradient p - p0")
    for q in (1, 2, 3):
        bounded(got[q], want[q], r32[q], "zero gradient " + AMS_NAMES[q])
    # a late first step: the bias corrections are 1 - 0.9^100000 = 1 and 1 - 0.999^100000 = 1 - 3.5e-44
    g = rng.normal(size=n).astype(f32)
    late = ams_step(hiplib, ams_buffers(n, p0), n, g, h, 100000)
    want = rd.amsgrad(p0, [g], h["lr"], h["betas"], h["eps"], h["wd"], first_step=100000)[0]
    r32 = dc.amsgrad_f32(p0, [g], h, first_step=100000)[0]
    bounded(late[0].astype(f64) - p0, want[0] - p0, r32[0].astype(f64) - p0, "step 100000 p - p0")
    for q in (1, 2, 3):
        bounded(late[q], want[q], r32[q], "step 100000 " + AMS_NAMES[q])
    first = rd.amsgrad(p0, [g], h["lr"], h["betas"], h["eps"], h["wd"])[0]
    assert np.abs(first[0] - want[0]).max() > 100 * dc.bound(0) * np.abs(want[0] - p0).max()      # step 1 would not pass as step 100000
    # the same state twice
    state = [late[1], late[2], late[3]]
    a = ams_step(hiplib, ams_buffers(n, late[0], state), n, g * f32(0.5), h, 7)
    b = ams_step(hiplib, ams_buffers(n, late[0], state), n, g * f32(0.5), h, 7)
    assert all(same(x, y) for x, y in zip(a, b)) and not same(a[0], late[0])
