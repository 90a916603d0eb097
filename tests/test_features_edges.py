"""CPU side of the keypoint-feature edge tests (SPEC.md section 11): every case of tests/features_cases.py holds the edge it
is named after, and the forms added to tests/ref_features.py for the cases (describe_rows, smoothed_histogram,
match_matrix) equal the forms the existing tests use. Prints the premise figures."""
import numpy as np
import pytest

import features_cases as fc
import ref_features as rf

STAGES = (("detect", fc.detect_cases), ("describe", fc.describe_cases), ("match", fc.match_cases),
          ("hypotheses", fc.hypotheses_cases))


@pytest.mark.parametrize("stage,build", STAGES, ids=[s for s, _ in STAGES])
def test_every_premise_holds(stage, build):
    """Building asserts each premise; here: every named case exists once, and its figures are printed."""
    cases = build()
    assert sorted(c["name"] for c in cases) == sorted(fc.NAMES[stage])
    for c in cases:
        print(c["name"], c["premise"])


def test_sizes_that_take_another_path():
    """The sizes the cases are there for, read off the built cases."""
    d = {c["name"]: c for c in fc.detect_cases()}
    scans = ("d_scan_1024", "d_scan_1025", "d_scan_2049", "d_scan_3150")
    assert [d[k]["premise"]["blocks"] for k in scans] == [1024, 1025, 2049, 3150]
    assert [d[k]["premise"]["per_thread"] for k in scans] == [1, 2, 3, 4]
    assert (d["d_scan_3150"]["H"], d["d_scan_3150"]["W"], d["d_scan_3150"]["octaves"]) == (480, 640, 3)
    caps = {(c["cap"], len(c["want"]) - c["cap"]) for k, c in d.items() if k.startswith("d_cap")}
    assert caps == {(4096, 0), (4096, 1), (1, 0), (1, 1)}
    m = fc.match_cases()
    assert {c["n"] for c in m} >= {1, 32, 33, 64, 65, 127, 128, 129, 257, 4096}
    assert {len(c["B"]) for c in m} >= {127, 128, 129, 2047, 2048, 2049, 4097, 65536}
    assert {c["n"] for c in fc.hypotheses_cases()} >= {1, 255, 256, 257}


def test_a_32_bit_edge_test_would_decide_otherwise():
    """11.2's edge test with tr, det4 and both products wrapped to 32 bits changes the keypoints of the full-range pyramid
    and of the large-amplitude patterns: these cases notice what no natural frame does."""
    def wrap(v):
        return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31
    by = {c["name"]: c for c in fc.detect_cases()}
    c = by["d_random_full_range"]
    hs = fc.hessian(c["levels"], c["want"])
    lost = sum(1 for tr, det4 in hs if not (wrap(det4) > 0 and wrap(wrap(40 * wrap(tr)) * wrap(tr)) < wrap(121 * wrap(det4))))
    print("full-range pyramid: %d of %d keypoints lost to a 32-bit edge test" % (lost, len(hs)))
    assert lost > 0
    flips = 0
    for k in ("d_large_ratio_1", "d_large_ratio_10", "d_large_ratio_9p99"):
        p = by[k]["premise"]
        narrow = wrap(p["det4"]) > 0 and wrap(wrap(40 * wrap(p["tr"])) * wrap(p["tr"])) < wrap(121 * wrap(p["det4"]))
        flips += narrow != p["kept"]
    assert flips >= 1


def _frame(H, W, seed):
    """A frame the existing tests use, from their own helpers (test_features_gpu's blobs on a tilted plane with a step
    and holes); the cases' smooth_frame is the same image."""
    import test_features_gpu as tg
    img = tg._smooth(H, W, seed)
    assert np.array_equal(fc.smooth_frame(H, W, seed, 30), img)
    d, m = tg._depth_plane(H, W, seed)
    return img, d, m, tg.K_SMALL


def test_per_row_forms_equal_todays_featurize():
    """describe_rows on featurize's own keypoints gives featurize's rows, and orientation is the first arg-max of
    smoothed_histogram: the yardstick did not move."""
    seen = {"rows": 0, "ok": 0, "window": 0, "binned": 0}
    for H, W, seed in ((65, 97, 2), (120, 160, 3)):
        img, depth, mask, K = _frame(H, W, seed)
        tr = {}
        kps, bins, desc, frames, ok = rf.featurize(img, depth, mask, K, trace=tr)
        b2, d2, F2, ok2 = rf.describe_rows(tr["pyramid"], depth, K, kps)
        assert np.array_equal(b2, bins) and np.array_equal(d2, desc) and np.array_equal(ok2, ok)
        assert np.array_equal(F2.view(np.int64), frames.view(np.int64))
        for (o, s, y, x), b in zip(kps.tolist(), bins.tolist()):
            if b >= 0:
                gx, gy = rf.gradients(tr["pyramid"][o][s])
                assert int(np.argmax(rf.smoothed_histogram(gx, gy, s, y, x))) == b
                seen["binned"] += 1
        seen["rows"] += len(kps)
        seen["ok"] += int(ok.sum())
        seen["window"] += int((bins < 0).sum())
    print(seen)
    assert seen["rows"] >= 20 and seen["ok"] > 0 and seen["window"] > 0 and seen["binned"] > 0


def test_matrix_form_of_the_matcher_equals_match():
    rng = np.random.default_rng(3)
    B = rng.integers(0, 128, (300, 128)).astype(np.int8)
    A = rng.integers(0, 128, (40, 128)).astype(np.int8)
    A[:20] = np.clip(B[rng.integers(0, 300, 20)].astype(int) + rng.integers(-3, 4, (20, 128)), 0, 127).astype(np.int8)
    B[250], B[17] = B[100], B[100]                      # ties: the first minimum
    A[39] = B[100]
    ok = rng.random(40) < 0.8
    ok[39] = True
    for a, b in zip(rf.match_matrix(A, ok, B), rf.match(A, ok, B)):
        assert np.array_equal(a, b)
    assert rf.match_matrix(A, ok, B)[0][39] == 17
    for a, b in zip(rf.match_matrix(A, ok, B[:0]), rf.match(A, ok, B[:0])):
        assert np.array_equal(a, b)


def test_synthetic_pyramid_buffer_has_the_headers_layout():
    """Octaves back to back, [5][Ho][Wo] each, then two scratch planes of the frame."""
    levels = fc.random_levels(37, 53, 3, 1)
    buf = fc.pyramid_buffer(levels, 37, 53, 3)
    assert buf.dtype == np.int32 and len(buf) == 5 * (37 * 53 + 19 * 27 + 10 * 14) + 2 * 37 * 53
    assert buf[5 * 37 * 53 + 2 * 19 * 27 + 3 * 27 + 4] == levels[1][2, 3, 4]
