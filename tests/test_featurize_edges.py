"""CPU tests (no GPU) of the Zephyr featurizer at its edges: oracle/zephyr_oracle.c against the two numpy restatements
of SPEC 3.1-3.6 (tests/ref_featurize.py: float32, bit for bit; float64, decisions exactly and float channels within 4 x
the float32 restatement's own error) on the inputs of tests/featurize_cases.py, in both gather modes. The same cases run
on the kernels in tests/test_featurize_edges_gpu.py."""
import numpy as np
import pytest

import featurize_cases as fc
import ref_featurize as rf

CASES = list(fc.featurize_cases())
F64_CASES = [n for n in CASES if n not in fc.NOT_IN_F64]


def oracle_frame_and_table(ozr, c):
    rgbd = ozr.pack_rgbd(c["rgb"], c["depth"])
    return rgbd, ozr.prep_model(c["pts"], c["nrm"], c["col"])


def check_against_restatements(c, interp, sel, px, uv, counts, label):
    """px, uv for (interp, sel) and counts {margin: [N]} from the oracle or the kernels: bit for bit what the float32
    restatement gives; for the float64 leg, the restatements decide alike and the float channels obey the 4 x rule.
    -> (err of px, err of the float32 restatement) per channel, or None outside the float64 leg"""
    r32 = fc.ref(c, interp, sel=sel)
    assert np.array_equal(uv, r32["uv"]), (label, "uv_original")
    assert fc.same_bits(px, r32["point_x"]), (label, "point_x", np.argwhere(px.view(np.uint32) != r32["point_x"].view(np.uint32))[:4])
    for m, cnt in counts.items():
        assert np.array_equal(cnt, fc.ref(c, interp, margin=m)["count"]), (label, "inconst_count", m)
    if c["name"] in fc.NOT_IN_F64:
        return None
    r64 = fc.ref(c, interp, sel=sel, dtype=np.float64)
    for k in rf.DECISIONS:
        assert np.array_equal(r32[k], r64[k]), (label, "float32 and float64 decide differently", k)
    for m, cnt in counts.items():
        assert np.array_equal(cnt, fc.ref(c, interp, margin=m, dtype=np.float64)["count"]), (label, "float64 count", m)
    e32 = fc.channel_errors(r32["point_x"], r64["point_x"])
    err = fc.channel_errors(px, r64["point_x"])
    assert not fc.within_4x(err, e32), (label, fc.within_4x(err, e32), err, e32)
    return err, e32


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_both_restatements(ozr, name):
    c = fc.featurize_cases()[name]
    rgbd, tab = oracle_frame_and_table(ozr, c)
    assert fc.same_bits(rgbd, rf.pack_rgbd(c["rgb"], c["depth"]))
    assert fc.same_bits(tab, rf.model_table(c["pts"], c["nrm"], c["col"]))
    worst = np.zeros((2, 8))
    for interp in (0, 1):
        counts = {m: ozr.inconst_count(rgbd, c["T"], tab, c["K"], margin=m) for m in c["margins"]}
        for sel in c["sels"]:
            px, uv = ozr.featurize(rgbd, c["T"], tab, c["K"], sel=None if sel is None else np.array(sel, np.int32),
                                   interp=interp)
            e = check_against_restatements(c, interp, sel, px, uv, counts if sel is None else {},
                                           "%s interp=%d sel=%s" % (name, interp, sel))
            if e:
                worst[interp] = np.maximum(worst[interp], e[0])
    for interp in (0, 1):
        print("%s interp=%d: %s" % (name, interp, " ".join("%s %.2e" % kv for kv in zip(fc.CHANNELS, worst[interp]))))


def test_every_case_but_the_named_ones_is_in_the_float64_leg():
    assert len(F64_CASES) == len(CASES) - 1 and fc.NOT_IN_F64 == ("hsv_near_grey_taps",)


def test_hsv_set_matches_matplotlib(ozr):
    """the HSV edge colours, and quarter-weight mixes of them, against matplotlib (the bound of test_oracle.py)"""
    mc = pytest.importorskip("matplotlib.colors")
    fc.hsv_set_premise()
    mixes = [(a * np.float32(w) + b * np.float32(1 - w)) for a in fc.HSV_SET for b in fc.HSV_SET for w in (0.25, 0.5)]
    rgb = np.concatenate([fc.HSV_SET, np.array(mixes, np.float32)])
    got = ozr.rgb_to_hsv(rgb)
    assert np.allclose(got, mc.rgb_to_hsv(rgb).astype(np.float32), rtol=0, atol=1e-6)
    hsv, branch, wrap = rf.hsv_full(rgb)
    assert np.array_equal(got, hsv) and set(branch.tolist()) == {0, 1, 2, 3} and wrap.any()
    h64 = rf.hsv_full(rgb, np.float64)[0][:, 0]
    circ = np.abs(got[:, 0] - h64)
    assert np.minimum(circ, 1 - circ).max() < 1e-6            # hue 1.0 and hue 0 are the same hue


@pytest.mark.parametrize("name", [s[0] for s in fc.staging_cases()])
def test_staging_oracle_equals_restatement(ozr, name):
    _, img, depth = next(s for s in fc.staging_cases() if s[0] == name)
    want = rf.blur5_u8(img)
    assert np.array_equal(ozr.blur5_u8(img), want)
    assert fc.same_bits(ozr.pack_rgbd(ozr.u8_to_unit(want), depth), rf.pack_rgbd(rf.u8_to_unit(want), depth))
    if name == "all_255":
        assert (want == 255).all()
    if name == "half_rounds_up":
        assert want[4, 4, 0] == 1 and want[2, 2, 0] == 3      # sums 128 -> 1 (127 would give 0) and 36 * 20 + 3 = 723 -> 3


def test_filter_threshold_in_float64(ozr):
    """SPEC 3.5 on the filter-edge case: counts 20, 21, 19 of M = 200 at th = 10 -> kept, dropped, kept"""
    c = fc.filter_edge()
    rgbd, tab = oracle_frame_and_table(ozr, c)
    cnt = ozr.inconst_count(rgbd, c["T"], tab, c["K"])
    assert cnt.tolist() == [20, 21, 19]
    assert (cnt.astype(np.float64) * 100.0 <= 10.0 * 200).tolist() == [True, False, True]
