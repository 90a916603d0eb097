"""The keypoint-feature kernels (csrc/features.hip) at their edges: every case of tests/features_cases.py through
ossid_feat_detect, _describe, _match and _hypotheses directly, against the restatement tests/ref_features.py. Every output
lives in a tests/guarded.py buffer filled with a sentinel and is compared bit for bit (integers by value, f64 frames and
poses through their int64 view); rows past min(count, cap) still hold the sentinel, the guard words around every output and
workspace are intact, and two runs are byte-identical. No tolerance anywhere.

The builders are cached: the first test of a stage builds all of that stage's cases on the CPU (a few seconds for detect,
whose four scan pyramids are up to 480 x 640 x 3), every later one only looks its case up."""
import numpy as np
import pytest
import torch

import features_cases as fc
import guarded
import ref_features as rf
from guarded import Guarded

pytestmark = pytest.mark.gpu

SENT = guarded.OUT_FILL


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(g, dtype, rows=None):
    """The payload of a Guarded as a numpy array of `dtype` (the first `rows` rows of it)."""
    a = g.payload.cpu().numpy().view(dtype)
    return a if rows is None else a[:rows]


def sentinel_from(g, nbytes):
    """Every payload byte from `nbytes` on still holds the sentinel."""
    return bool((g.payload[nbytes:] == SENT).all().item())


def finish(rc, *bufs):
    assert rc == 0
    guarded.sync()
    for g in bufs:
        assert g.intact(), "guard words around a %d-byte buffer were overwritten" % g.nbytes


# ---- detect -------------------------------------------------------------------------------------------------------------
def run_detect(lib, c):
    guarded.ready()
    H, W, oc, cap = c["H"], c["W"], c["octaves"], c["cap"]
    assert lib.fn("ossid_feat_pyramid_bytes")(H, W, oc) == 4 * fc.pyramid_words(H, W, oc)
    wb = int(lib.fn("ossid_feat_detect_workspace_bytes")(H, W, oc))
    flat = sum(2 * h * w for h, w in rf.octave_sizes(H, W, oc))
    assert (wb - flat) // 4 == c["premise"]["blocks"] and (wb - flat) % 4 == 0
    pyr, depth, mask = dev(fc.pyramid_buffer(c["levels"], H, W, oc)), dev(c["depth"]), dev(c["mask"])
    ws, kps, count = Guarded(wb, 0x5A), Guarded(cap * 16, SENT), Guarded(8, SENT)
    rc = lib.fn("ossid_feat_detect")(pyr.data_ptr(), H, W, oc, depth.data_ptr(), mask.data_ptr(), c["contrast"], cap, ws.ptr, wb,
                                     kps.ptr, count.ptr, lib.stream())
    finish(rc, ws, kps, count)
    return kps, count


@pytest.mark.parametrize("name", fc.NAMES["detect"])
def test_detect(hiplib, name):
    c = fc.by_name("detect")[name]
    want, cap = c["want"], c["cap"]
    kps, count = run_detect(hiplib, c)
    k = min(len(want), cap)
    got = host(kps, np.int32).reshape(-1, 4)[:k]
    print(name, c["premise"], "device count", host(count, np.int32).tolist())
    assert host(count, np.int32).tolist() == [len(want), 1 if len(want) > cap else 0]
    bad = np.flatnonzero((got != want[:k]).any(1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(got, want[:k].astype(np.int32)) and sentinel_from(kps, 16 * k)
    kps2, count2 = run_detect(hiplib, c)
    assert torch.equal(kps.payload, kps2.payload) and torch.equal(count.payload, count2.payload)


# ---- describe -----------------------------------------------------------------------------------------------------------
def run_describe(lib, c, count=None):
    guarded.ready()
    H, W, oc, cap, n = c["H"], c["W"], c["octaves"], c["cap"], c["n"]
    pyr, depth, rows = dev(fc.pyramid_buffer(c["levels"], H, W, oc)), dev(c["depth"]), dev(c["kps"])
    cnt = dev(np.array([n, 0] if count is None else count, dtype=np.int32))
    assert rows.shape == (cap, 4) and rows.dtype == torch.int32
    o = dict(bins=Guarded(cap * 4, SENT), desc=Guarded(cap * 128, SENT), frames=Guarded(cap * 128, SENT), ok=Guarded(cap, SENT))
    fx, fy, cx, cy = (float(v) for v in c["K"])
    rc = lib.fn("ossid_feat_describe")(pyr.data_ptr(), H, W, oc, depth.data_ptr(), fx, fy, cx, cy, rows.data_ptr(), cnt.data_ptr(),
                                       cap, o["bins"].ptr, o["desc"].ptr, o["frames"].ptr, o["ok"].ptr, lib.stream())
    finish(rc, *o.values())
    return o


def check_describe(o, w, n):
    bins, ok = host(o["bins"], np.int32, n), host(o["ok"], np.uint8, n)
    desc = host(o["desc"], np.int8).reshape(-1, 128)[:n]
    frames = host(o["frames"], np.int64).reshape(-1, 4, 4)[:n]
    assert np.array_equal(bins, w["bins"].astype(np.int32)), np.flatnonzero(bins != w["bins"])[:8]
    assert np.array_equal(ok, w["ok"].astype(np.uint8)), np.flatnonzero(ok != w["ok"])[:8]
    assert np.array_equal(desc, w["desc"]), np.flatnonzero((desc != w["desc"]).any(1))[:8]
    wf = w["frames"].view(np.int64)
    assert np.array_equal(frames, wf), np.flatnonzero((frames != wf).any((1, 2)))[:8]
    for k, width in (("bins", 4), ("desc", 128), ("frames", 128), ("ok", 1)):
        assert sentinel_from(o[k], n * width), "%s: a row behind count was written" % k


@pytest.mark.parametrize("name", fc.NAMES["describe"])
def test_describe(hiplib, name):
    c = fc.by_name("describe")[name]
    print(name, c["premise"])
    a = run_describe(hiplib, c)
    check_describe(a, c["want"], c["n"])
    b = run_describe(hiplib, c)
    assert all(torch.equal(a[k].payload, b[k].payload) for k in a)


def test_describe_over_the_cap_reads_and_writes_nothing(hiplib):
    c = fc.by_name("describe")["b_full_range"]
    o = run_describe(hiplib, c, count=[c["cap"] + 1, 1])
    assert all(sentinel_from(g, 0) for g in o.values())


def test_full_size_frame_in_every_stage(hiplib):
    """480 x 640, the product size: 3150 detect blocks (four per scanning thread), compared stage by stage."""
    from ossid_code_amd import features
    c = fc.full_size_frame()
    print(c["premise"])
    w = c["want"]
    f = features.featurize(c["img"], c["depth"], c["mask"], c["K"])
    guarded.sync()
    buf, off = f["pyramid"].cpu().numpy(), 0
    for lv in c["pyramid"]:
        assert np.array_equal(buf[off:off + lv.size].reshape(lv.shape), lv)
        off += lv.size
    n = len(w["kps"])
    assert f["count"].cpu().numpy().tolist() == [n, 0]
    assert np.array_equal(f["keypoints"].cpu().numpy()[:n], w["kps"].astype(np.int32))
    assert np.array_equal(f["bins"].cpu().numpy()[:n], w["bins"].astype(np.int32))
    assert np.array_equal(f["ok"].cpu().numpy()[:n], w["ok"].astype(np.uint8))
    assert np.array_equal(f["descriptors"].cpu().numpy()[:n].view(np.int8), w["desc"])
    assert np.array_equal(f["frames"].cpu().numpy()[:n].view(np.int64), w["frames"].view(np.int64))


# ---- match --------------------------------------------------------------------------------------------------------------
def run_match(lib, c):
    guarded.ready()
    cap, Nm = c["cap"], len(c["B"])
    A, ok, cnt, B = dev(c["A"]), dev(c["ok"]), dev(c["count"]), dev(c["B"])
    wb = int(lib.fn("ossid_feat_match_workspace_bytes")(cap))
    assert wb == cap * 8
    ws, out = Guarded(wb, 0x5A), Guarded(cap * 12, SENT)
    rc = lib.fn("ossid_feat_match")(A.data_ptr(), ok.data_ptr(), cnt.data_ptr(), cap, B.data_ptr(), Nm, ws.ptr, wb, out.ptr,
                                    lib.stream())
    finish(rc, ws, out)
    return out


@pytest.mark.parametrize("name", fc.NAMES["match"])
def test_match(hiplib, name):
    c = fc.by_name("match")[name]
    print(name, c["premise"])
    want = c["want"]
    out = run_match(hiplib, c)
    got = host(out, np.int32).reshape(-1, 3)[:len(want)]
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(got, want) and sentinel_from(out, 12 * len(want))
    assert torch.equal(out.payload, run_match(hiplib, c).payload)


# ---- hypotheses ---------------------------------------------------------------------------------------------------------
def run_hypotheses(lib, c):
    guarded.ready()
    cap, Nm = c["cap"], c["Nm"]
    m, Fs, Fm, cnt = dev(c["match"]), dev(c["Fs"]), dev(c["Fm"]), dev(c["count"])
    assert m.shape == (cap, 3) and Fs.shape == (cap, 4, 4) and Fs.dtype == torch.float64
    peaks, cand = Guarded(cap * 12, SENT), Guarded(cap * 128, SENT)
    rc = lib.fn("ossid_feat_hypotheses")(m.data_ptr(), Fs.data_ptr(), cnt.data_ptr(), cap, Fm.data_ptr(), Nm, peaks.ptr, cand.ptr,
                                         lib.stream())
    finish(rc, peaks, cand)
    return peaks, cand


@pytest.mark.parametrize("name", fc.NAMES["hypotheses"])
def test_hypotheses(hiplib, name):
    c = fc.by_name("hypotheses")[name]
    print(name, c["premise"])
    peaks, cand = run_hypotheses(hiplib, c)
    n = 0 if c["count"][0] > c["cap"] else c["n"]
    w = c["want"]
    got_p = host(peaks, np.int32).reshape(-1, 3)[:n]
    got_c = host(cand, np.int64).reshape(-1, 4, 4)[:n]
    assert np.array_equal(got_p, w["peaks"][:n]), np.flatnonzero((got_p != w["peaks"][:n]).any(1))[:8]
    wc = w["cand"][:n].view(np.int64)
    assert np.array_equal(got_c, wc), np.flatnonzero((got_c != wc).any((1, 2)))[:8]
    rejected = w["peaks"][:n, 2] == 0
    assert not got_c[rejected].any() and not got_p[rejected].any()      # all-zero bits: no -0.0 either
    assert sentinel_from(peaks, 12 * n) and sentinel_from(cand, 128 * n)
    p2, c2 = run_hypotheses(hiplib, c)
    assert torch.equal(peaks.payload, p2.payload) and torch.equal(cand.payload, c2.payload)
