"""SPEC.md 8.10-8.12 on the device: ossid_bop_vsd_pairs against ossid_bop_vsd with every pair expanded into a row of its own
(bit-equal counts and errors -- no new reference is needed), its edge rows through the C ABI, ossid_bop_match against the
restatement tests/ref_bop_match.py (equal match and tp), and evaluate(..., multi_instance=True) / tools/eval_bop19.py
--multi_instance against the restatement's scores on a BOP folder whose targets have three instances."""
import os
import sys

import numpy as np
import pytest
import torch

import ref_bop_eval as rb
import ref_bop_match as rm
import ref_icp as ri
import ref_raster as rr
from ossid_code_amd import bop_eval, render, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAMETER = 0.1
GUARD = 64
KEYS = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "recall_vsd", "recall_mssd", "recall_mspd")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _camera(H, W):
    K = np.array(synth.CAM_K, dtype=np.float64)
    K[0] *= W / 640.0
    K[1] *= H / 480.0
    return K


def _perturbed(T, k):
    return ri.perturb(T, [0.2, 1.0, 0.4], 1.0 + k, np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0) * 0.002 * k)


SPOTS = [(-0.12, 0.0, 0.75), (0.0, 0.02, 0.7), (0.12, -0.02, 0.8), (0.03, -0.05, 0.65)]


@pytest.fixture(scope="module")
def world():
    """The level-1 mesh, four instance poses, and per frame size two frames with their own cameras."""
    V, F = rr.bump_mesh(1)
    gts = np.stack([rr.pose_at(t, axis=(0.3, 1.0, 0.2 + n), deg=25.0 + 30 * n) for n, t in enumerate(SPOTS)])
    out = {"V": V, "F": F, "gt": gts}
    for H, W in ((48, 64), (77, 123)):
        K = _camera(H, W)
        K2 = K.copy()
        K2[0, 0] *= 1.1
        K2[1, 1] *= 0.95
        K2[0, 2] += 1.5
        O = np.stack([synth.make_frame(42, H, W)[1], synth.make_frame(7, H, W)[1]])
        out[(H, W)] = (O, np.stack([K, K2]))
    return out


def _expanded(mesh, O, Ks, pe, pg, pairs, **kw):
    """The only way the single-instance entry point has: one row, two renders, per pair."""
    pairs = np.asarray(pairs)
    return bop_eval.vsd(mesh, DIAMETER, O, Ks, pe[pairs[:, 0]], pg[pairs[:, 1]], frame=pairs[:, 2].astype(np.int32), return_counts=True, **kw)


@pytest.mark.parametrize("hw", [(48, 64), (77, 123)])
def test_vsd_pairs_bit_equal_to_expanded_rows(hiplib, world, hw):
    """hw (77, 123) is 8's odd frame size 123 x 77 (the scalar-load path). A 3 x 4 group in frame 0, pairs of the second frame
    and camera, a pose behind the camera as estimate and as instance, then the same table shuffled, and P = 1."""
    O, Ks = world[hw]
    mesh = render.Mesh(world["V"], world["F"])
    pg = np.concatenate([world["gt"], rr.pose_at((0.05, 0.02, -0.75))[None]])          # row 4: behind the camera
    pe = np.stack([_perturbed(pg[0], 1), _perturbed(pg[1], 2), _perturbed(pg[2], 0), rr.pose_at((0.0, 0.0, -0.5))])
    group = [(e, g, 0) for e in range(3) for g in range(4)]
    pairs = np.array(group + [(0, 0, 1), (2, 2, 1), (1, 3, 1), (3, 0, 0), (0, 4, 1), (3, 4, 0), (2, 2, 0)], dtype=np.int32)
    err, counts = bop_eval.vsd_pairs(mesh, DIAMETER, O, Ks, pe, pg, pairs, return_counts=True)
    werr, wcounts = _expanded(mesh, O, Ks, pe, pg, pairs)
    print(counts.tolist())
    assert counts.dtype == np.int32 and counts.shape == (len(pairs), 12) and err.shape == (len(pairs), 10)
    assert np.array_equal(counts, wcounts) and _same_bits(err, werr)
    assert counts[:12, 0].min() > 0 and counts[[0, 5, 10], 1].min() > 0               # e = g pairs overlap
    assert counts[17, 0] == 0 and np.array_equal(err[17], np.ones(10))                 # both behind the camera: n_U = 0, e = 1
    assert counts[15, 1] == 0 and counts[16, 1] == 0 and np.array_equal(err[15], np.ones(10))
    assert np.array_equal(counts[18], counts[10]) and not np.array_equal(counts[12], counts[0])
    # a shuffled table gives the shuffled rows; so does every chunking
    order = np.random.default_rng(3).permutation(len(pairs))
    e2, c2 = bop_eval.vsd_pairs(mesh, DIAMETER, O, Ks, pe, pg, pairs[order], return_counts=True)
    assert np.array_equal(c2, counts[order]) and _same_bits(e2, err[order])
    for chunk in (1, 2, 256):
        e3, c3 = bop_eval.vsd_pairs(mesh, DIAMETER, O, Ks, pe, pg, pairs[order], return_counts=True, chunk=chunk)
        assert np.array_equal(c3, counts[order]) and _same_bits(e3, err[order]), chunk
    # P = 1, other taus and delta
    taus = [0.02, 0.3]
    e4, c4 = bop_eval.vsd_pairs(mesh, DIAMETER, O, Ks, pe, pg, [[1, 1, 1]], delta=0.004, taus=taus, return_counts=True)
    we4, wc4 = _expanded(mesh, O, Ks, pe, pg, [[1, 1, 1]], delta=0.004, taus=taus)
    assert c4.shape == (1, 4) and np.array_equal(c4, wc4) and _same_bits(e4, we4) and c4[0, 1] > 0


def _abi_pairs(hiplib, O, cams, ze, zg, pairs, diameter, delta, taus):
    dev = torch.device("cuda", 0)
    (Ne, H, W), Ng, P, T = ze.shape, len(zg), len(pairs), len(taus)
    t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (O, cams, ze, zg)]
    tab = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32)).to(dev)
    counts = torch.full((P * (T + 2) + GUARD,), -7, dtype=torch.int32, device=dev)
    errors = torch.full((P * T + GUARD,), -7.0, dtype=torch.float64, device=dev)
    tau = np.ascontiguousarray(taus, dtype=np.float64)
    rc = hiplib.fn("ossid_bop_vsd_pairs")(t[0].data_ptr(), t[1].data_ptr(), len(O), H, W, t[2].data_ptr(), Ne, t[3].data_ptr(), Ng,
                                          tab.data_ptr(), P, float(diameter), float(delta), tau.ctypes.data, T, counts.data_ptr(),
                                          errors.data_ptr(), hiplib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    c, e = counts.cpu().numpy(), errors.cpu().numpy()
    assert (c[P * (T + 2):] == -7).all() and (e[P * T:] == -7.0).all()                 # the guard words
    return c[:P * (T + 2)].reshape(P, T + 2), e[:P * T].reshape(P, T)


@pytest.mark.parametrize("hw", [(16, 20), (13, 17), (70, 64)])
@pytest.mark.parametrize("T", [1, 16])
def test_vsd_pairs_edge_rows_through_the_abi(hiplib, hw, T):
    """Made-up renders: rows whose indices leave the stacks or the frames give the zero row (counts 0, e = 1) and leave their
    neighbours as the restatement has them; nothing is written behind either output; two runs agree byte for byte."""
    H, W = hw
    rng = np.random.default_rng(H * 100 + T)
    Ne, Ng, Fr = 5, 7, 3
    O = (0.5 + rng.random((Fr, H, W))).astype(np.float32)
    O[rng.random(O.shape) < 0.2] = 0.0
    cams = np.array([[30.0, 31.0, W / 2.0, H / 2.0], [25.5, 24.0, 3.25, 4.5], [40.0, 40.0, W - 1.0, 0.0]], dtype=np.float32)
    zg = (0.6 + 0.8 * rng.random((Ng, H, W))).astype(np.float32)
    ze = (zg[:Ne] + rng.normal(0.0, 0.02, (Ne, H, W))).astype(np.float32)
    zg[rng.random(zg.shape) < 0.4] = 0.0
    ze[rng.random(ze.shape) < 0.4] = 0.0
    ze[4], zg[6] = 0.0, 0.0
    good = [(e, g, (e + g) % Fr) for e in range(Ne) for g in range(Ng)]
    big, small = 2 ** 31 - 1, -2 ** 31
    bad = [(-1, 0, 0), (Ne, 0, 0), (0, -1, 0), (0, Ng, 0), (0, 0, -1), (0, 0, Fr), (big, 0, 0), (0, big, 0), (0, 0, big),
           (small, small, small), (Ne, Ng, Fr)]
    pairs = []
    for n, row in enumerate(good):                                # a bad row after every third good one, and one first
        if n % 3 == 0:
            pairs.append(bad[(n // 3) % len(bad)])
        pairs.append(row)
    pairs = np.array(pairs, dtype=np.int64)
    is_bad = np.array([tuple(int(v) for v in r) in bad for r in pairs])
    assert is_bad[0] and is_bad.sum() == 12 and len(pairs) == 47
    taus = np.sort(rng.random(T) * 0.5) if T > 1 else np.array([0.2])
    counts, errors = _abi_pairs(hiplib, O, cams, ze, zg, pairs, 0.3, 0.015, taus)
    for p, (e, g, f) in enumerate(pairs):
        if is_bad[p]:
            assert not counts[p].any() and np.array_equal(errors[p], np.ones(T)), p
        else:
            wc, we = rb.vsd_from_renders(O[f], cams[f], ze[e], zg[g], 0.3, 0.015, taus)
            assert counts[p].tolist() == wc.tolist() and _same_bits(errors[p], we), p
    assert counts[~is_bad][:, 1].max() > 0 and not counts[-1].any()                   # (4, 6): both renders empty
    c2, e2 = _abi_pairs(hiplib, O, cams, ze, zg, pairs, 0.3, 0.015, taus)
    assert counts.tobytes() == c2.tobytes() and errors.tobytes() == e2.tobytes()


def test_pair_and_match_argument_checks_return_einval(hiplib):
    buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    taus = np.full(16, 0.1)
    tab = torch.zeros(12, dtype=torch.int32, device="cuda")
    args = (("O", p), ("cams", p + 4096), ("Fr", 1), ("H", 8), ("W", 8), ("ze", p + 8192), ("Ne", 2), ("zg", p + 16384), ("Ng", 2),
            ("pairs", tab.data_ptr()), ("P", 4), ("diam", 0.1), ("delta", 0.015), ("taus", taus.ctypes.data), ("T", 10),
            ("counts", p + 32768), ("errors", p + 65536), ("s", hiplib.stream()))
    fn = hiplib.fn("ossid_bop_vsd_pairs")
    call = lambda **kw: fn(*[kw.get(k, d) for k, d in args])  # noqa: E731
    assert call() == 0
    bad_taus = np.array([0.1, np.nan])
    for kw in ({"T": 0}, {"T": 17}, {"P": 0}, {"P": -3}, {"Fr": 0}, {"Ne": 0}, {"Ng": 0}, {"diam": 0.0}, {"diam": float("nan")},
               {"diam": float("inf")}, {"delta": -1.0}, {"delta": float("nan")}, {"taus": bad_taus.ctypes.data, "T": 2}, {"H": 0},
               {"W": -1}, {"H": 4097, "W": 4096}, {"O": None}, {"cams": None}, {"ze": None}, {"zg": None}, {"pairs": None},
               {"taus": None}, {"counts": None}, {"errors": None}):
        assert call(**kw) == -22, kw
    ints = torch.zeros(4096, dtype=torch.int32, device="cuda")
    ints[3:5] = 1                                                  # one group: pair_first, est_first, inst_first = 0, E = G = 1
    q = ints.data_ptr()
    dbl = torch.zeros(1024, dtype=torch.float64, device="cuda")
    d = dbl.data_ptr()
    margs = (("err", d), ("Ptot", 1), ("groups", q), ("Gr", 1), ("valid", q + 1024), ("Itot", 1), ("thr", d + 1024), ("T", 10),
             ("match", q + 2048), ("Etot", 1), ("tp", q + 8192), ("s", hiplib.stream()))
    mfn = hiplib.fn("ossid_bop_match")
    mcall = lambda **kw: mfn(*[kw.get(k, dflt) for k, dflt in margs])  # noqa: E731
    assert mcall() == 0
    for kw in ({"Gr": 0}, {"Itot": 0}, {"Ptot": -1}, {"Etot": -1}, {"T": 0}, {"T": 17}, {"err": None}, {"groups": None},
               {"valid": None}, {"thr": None}, {"match": None}, {"tp": None}):
        assert mcall(**kw) == -22, kw
    assert mcall(err=None, Ptot=0, match=None, Etot=0) == 0        # a call whose groups hold no estimate
    torch.cuda.synchronize()


def _tables(rng, sizes, T, all_nan=False):
    """Random tables with deliberate ties: errors and thresholds from one short list of values, NaN and +inf among them."""
    K = T + 2
    values = np.array([0.05, 0.1, 0.15, 0.2, 0.3, np.nan, np.inf])
    E, G = np.array([s[0] for s in sizes]), np.array([s[1] for s in sizes])
    err = rng.choice(values, size=(int((E * G).sum()), K), p=[0.2, 0.2, 0.2, 0.15, 0.15, 0.05, 0.05])
    if all_nan:
        err[:] = np.nan
    thr = rng.choice(values[:5], size=(len(sizes), K, 10))
    thr[0, 0, :2] = [np.inf, 0.0]
    valid = rng.random(int(G.sum())) < 0.8
    return err, E, G, valid, thr


def _abi_match(hiplib, err, E, G, valid, thr):
    dev = torch.device("cuda", 0)
    K = thr.shape[1]
    C = K * 10
    first = lambda n: np.concatenate([[0], np.cumsum(n)[:-1]])  # noqa: E731
    table = np.ascontiguousarray(np.stack([first(E * G), first(E), first(G), E, G], 1), dtype=np.int32)
    Etot = int(E.sum())
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (err.astype(np.float64), table, valid.astype(np.uint8), thr)]
    match = torch.full((Etot * C + GUARD,), -7, dtype=torch.int32, device=dev)
    tp = torch.full((C + GUARD,), -7, dtype=torch.int32, device=dev)
    rc = hiplib.fn("ossid_bop_match")(t[0].data_ptr() if len(err) else None, len(err), t[1].data_ptr(), len(E), t[2].data_ptr(),
                                      len(valid), t[3].data_ptr(), K - 2, match.data_ptr(), Etot, tp.data_ptr(), hiplib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    m, c = match.cpu().numpy(), tp.cpu().numpy()
    assert (m[Etot * C:] == -7).all() and (c[C:] == -7).all()                          # the guard words
    return m[:Etot * C].reshape(Etot, K, 10), c[:C].reshape(K, 10)


def _many(rng):
    small = [(int(rng.integers(0, 3)), int(rng.integers(1, 3))) for _ in range(1025)]
    small[0], small[500], small[1024] = (2, 63), (63, 1), (0, 2)
    return small


MATCH_CASES = {
    "one_group_T16": (lambda rng: [(64, 64)], 16, False),
    "two_groups_T1": (lambda rng: [(63, 64), (2, 63)], 1, False),
    "empty_group_T16": (lambda rng: [(1, 2), (0, 64), (64, 1), (2, 2), (1, 1)], 16, False),
    "many_groups_T1": (_many, 1, False),
    "all_nan_T1": (lambda rng: [(2, 2), (64, 63), (1, 1)], 1, True),
}


@pytest.mark.parametrize("case", sorted(MATCH_CASES))
def test_match_equals_the_restatement(hiplib, case):
    sizes, T, all_nan = MATCH_CASES[case]
    rng = np.random.default_rng(len(case) * 7 + T)
    err, E, G, valid, thr = _tables(rng, sizes(rng), T, all_nan)
    want_match, want_tp = rm.match_instances(err, E, G, valid, thr)
    match, tp = _abi_match(hiplib, err, E, G, valid, thr)
    print(case, "groups", len(E), "pairs", len(err), "matched", int((match >= 0).sum()), "of", match.size, "tp", int(tp.sum()))
    assert match.dtype == np.int32 and np.array_equal(match, want_match) and np.array_equal(tp, want_tp)
    if all_nan:
        assert (match == -1).all() and not tp.any()
    else:
        assert (match >= 0).any() and tp.sum() > 0 and int((match >= 0).sum()) > int(tp.sum())      # an invalid instance was matched
    m2, tp2 = _abi_match(hiplib, err, E, G, valid, thr)
    assert match.tobytes() == m2.tobytes() and tp.tobytes() == tp2.tobytes()
    # the Python entry hands the same tables on
    m3, tp3 = bop_eval.match_instances(err, E, G, valid, thr)
    assert np.array_equal(m3, want_match) and np.array_equal(tp3, want_tp) and m3.dtype == np.int32 and tp3.shape == (T + 2, 10)


def test_match_skips_a_group_row_that_leaves_the_tables(hiplib):
    """The device's own check: a group whose ranges do not fit is skipped whole, its estimates stay -1, its neighbours are
    matched as if it were not there."""
    dev = torch.device("cuda", 0)
    err = torch.zeros(4, 3, dtype=torch.float64, device=dev)
    thr = torch.ones(5, 3, 10, dtype=torch.float64, device=dev)
    valid = torch.ones(4, dtype=torch.uint8, device=dev)
    #          pair_first est_first inst_first E  G
    groups = [[0, 0, 0, 1, 1], [1, 1, 1, 65, 1], [1, 1, 1, 1, 0], [3, 1, 1, 2, 1], [1, 1, 1, 1, 3]]
    tab = torch.tensor(groups, dtype=torch.int32, device=dev)
    match = torch.full((3 * 30 + GUARD,), -7, dtype=torch.int32, device=dev)
    tp = torch.full((30 + GUARD,), -7, dtype=torch.int32, device=dev)
    rc = hiplib.fn("ossid_bop_match")(err.data_ptr(), 4, tab.data_ptr(), 5, valid.data_ptr(), 4, thr.data_ptr(), 1, match.data_ptr(), 3,
                                      tp.data_ptr(), hiplib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    m, c = match.cpu().numpy(), tp.cpu().numpy()
    assert (m[:30] == 0).all() and (m[30:60] == 0).all() and (m[60:90] == -1).all() and (m[90:] == -7).all()
    assert (c[:30] == 2).all() and (c[30:] == -7).all()


class _Scenes:
    """Three scenes of 64 x 48 with the level-1 object drawn three times each, in millimetres."""

    def __init__(self, root):
        V, F = rr.bump_mesh(1)
        self.V, self.F = V * 1000.0, F
        self.K = _camera(48, 64)
        scenes, self.poses = {}, {}
        for s, sid in enumerate((0, 1, 5)):
            poses = []
            for n in range(3):
                T = rr.pose_at(np.array(SPOTS[(n + s) % 4]) * 1000.0, axis=(0.3, 1.0, 0.2 + n + s), deg=25.0 + 30 * n + 10 * s)
                poses.append(T)
            depth = synth.make_frame(40 + s, 48, 64)[1].astype(np.float64) * 1000.0 + 150.0
            for T in poses:
                z = rr.render(self.V, self.F, T, self.K, (48, 64), pixel_offset=0.0, z_near=50.0)[0]
                depth = np.where((z > 0) & (z < depth), z, depth)
            scenes[sid] = (np.rint(depth), poses, [1.0, 0.6, 0.05 if s == 1 else 0.3])
            self.poses[sid] = poses
        self.targets = rm.write_bop_folder(root, self.V, self.F, 100.0, scenes, self.K)

    def results(self):
        """Per target: the ground truths slightly perturbed, one duplicate, one far-off row (best-scored in scene 5)."""
        out = []
        for sid, poses in self.poses.items():
            rows = []
            for n, T in enumerate(poses):
                est = ri.perturb(T, [0.2, 1.0, 0.4 + n], 1.5 * (n + 1), np.array([1.0, -1.0, 1.0]) * (1.0 + 2.0 * n))
                rows.append({"scene_id": sid, "im_id": 0, "obj_id": 1, "score": 0.9 - 0.1 * n, "pose": est})
            dup = dict(rows[0], score=0.85 if sid == 1 else 0.2)
            far = poses[1].copy()
            far[:3, 3] += [150.0, 0.0, 100.0]
            rows += [dup, {"scene_id": sid, "im_id": 0, "obj_id": 1, "score": 0.95 if sid == 5 else 0.1, "pose": far}]
            out += rows[::-1] if sid == 0 else rows
        for r in out:
            r["pose"] = r["pose"].copy()
            r["pose"][:3, 3] /= 1000.0                            # the pipeline's results are in metres
        return out


def test_multi_instance_evaluation_end_to_end(hiplib, tmp_path, capsys):
    from ossid_code_amd import pipeline
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_bop19
    sc = _Scenes(str(tmp_path / "data"))
    assert [t["inst_count"] for t in sc.targets] == [3, 3, 3]
    path = pipeline.save_results_bop(sc.results(), str(tmp_path), "ossid", "multi")
    ds = bop_eval.BopFolder(str(tmp_path / "data"), "multi", "test")
    results = bop_eval.read_results_csv(path)
    assert len(results) == 15
    got = bop_eval.evaluate(results, ds, multi_instance=True)
    wrows, want = rm.evaluate(ds, results, 15.0, 50.0)
    print({k: got[k] for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR")})
    for k in KEYS:
        assert got[k] == want[k], k
    assert np.array_equal(got["match"], want["match"]) and got["match"].shape == (9, 12, 10)
    assert got["targets"] == 3 and got["estimates"] == 9 and len(got["rows"]) == 9 and 0.0 < got["AR"] < 1.0
    for r, w in zip(got["rows"], wrows):
        assert (r["scene_id"], r["score"]) == (w["scene_id"], w["score"])
        assert _same_bits(r["vsd"], w["vsd"]) and _same_bits(r["mssd"], w["mssd"]) and _same_bits(r["mspd"], w["mspd"])
        assert np.asarray(r["vsd"]).shape == (3, 10)
    # scene 1 keeps the duplicate as rank 1: instance 0 is taken by rank 0, so at the tightest MSSD threshold it stays unmatched
    rows1 = [i for i, r in enumerate(got["rows"]) if r["scene_id"] == 1]
    assert [got["rows"][i]["score"] for i in rows1] == [0.9, 0.85, 0.8]
    assert got["match"][rows1[0], 10, 0] == 0 and got["match"][rows1[1], 10, 0] == -1
    # a stricter visibility bound takes instances out of the count; none supplied counts every instance
    strict = bop_eval.evaluate(results, ds, multi_instance=True, visib_gt_min=0.5)
    _r, wstrict = rm.evaluate(ds, results, 15.0, 50.0, visib_gt_min=0.5)
    assert all(strict[k] == wstrict[k] for k in KEYS) and strict["AR"] < got["AR"] and np.array_equal(strict["match"], got["match"])
    # the command line
    out = eval_bop19.main(["--multi_instance", "--result_filenames=" + path, "--datasets_path=" + str(tmp_path / "data")])[path]
    for k in KEYS:
        assert out[k] == want[k], k
    assert ("AR %.6f" % want["AR"]) in capsys.readouterr().out
    # without the flag the folder is refused as before
    with pytest.raises(ValueError):
        eval_bop19.main(["--result_filenames=" + path, "--datasets_path=" + str(tmp_path / "data")])
    with pytest.raises(ValueError):
        bop_eval.evaluate(results, ds)
