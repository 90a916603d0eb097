"""SPEC.md 8.10-8.12 (BOP-19 targets with several instances) on the CPU: the restatement tests/ref_bop_match.py against
greedy answers written out by hand, and the host side of ossid_code_amd/bop_eval.py -- the kept-estimate rule, the tables
instance_recall forms, its agreement with average_recall where every target has one instance, the folder reader, the
command line's flags, the refusals. instance_recall matches on the device; here the restatement's loop stands in through
its `matcher` argument, and tests/test_bop_match_gpu.py holds the kernel to that loop."""
import os
import re
import sys

import numpy as np
import pytest

import ref_bop_eval as rb
import ref_bop_match as rm
from ossid_code_amd import bop_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAM = {1: 100.0, 2: 50.0}
KEYS = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR", "recall_vsd", "recall_mssd", "recall_mspd")


def _match(err, thr=0.5):
    """err [E][G] as the only error kind, one threshold in every column -> match [E] of column 0 (all columns agree)."""
    err = np.asarray(err, dtype=np.float64)
    m = rm.match_group(err[:, :, None], np.full((1, 10), thr))
    assert (m == m[:, :, :1]).all()
    return m[:, 0, 0].tolist()


def test_greedy_answers_written_out():
    # both estimates fit instance 0: the better-ranked takes it, the other takes instance 1 or nothing. An optimal
    # assignment would pair e0-g1 and e1-g0 in the second table; BOP's rule is greedy and leaves e1 unmatched.
    assert _match([[0.1, 0.2], [0.05, 0.3]]) == [0, 1]
    assert _match([[0.1, 0.2], [0.05, 0.6]]) == [0, -1]
    # an error equal to the threshold bit for bit is not below it; one float below is
    th = bop_eval.THETAS[5]
    assert _match([[th]], th) == [-1] and _match([[np.nextafter(th, 0.0)]], th) == [0]
    # NaN and +inf are never below; they do not block the instance for a later estimate
    assert _match([[np.nan, 0.4], [np.inf, np.nan], [0.3, np.inf]]) == [1, -1, 0]
    assert _match([[np.nan, np.nan]], np.inf) == [-1] and _match([[np.inf]], np.inf) == [-1]
    # equal errors: the lowest g; the next estimate gets the next one
    assert _match([[0.2, 0.2, 0.2], [0.2, 0.2, 0.2], [0.2, 0.2, 0.2], [0.2, 0.2, 0.2]]) == [0, 1, 2, -1]
    # the smallest error wins, not the first fit
    assert _match([[0.4, 0.3, 0.1]]) == [2]
    # E = 0
    assert rm.match_group(np.zeros((0, 3, 2)), np.ones((2, 10))).shape == (0, 2, 10)
    # columns are independent: a looser threshold in column 9 matches what column 0 refuses
    thr = np.array([[0.1 * (j + 1) for j in range(10)]])
    m = rm.match_group(np.array([[[0.35, ], [0.75]]]).reshape(1, 2, 1), thr)
    assert m[0, 0].tolist() == [-1, -1, -1, 0, 0, 0, 0, 0, 0, 0]


def _row(key, score, errs):
    """errs [G]: the same figure as VSD at every tau, as MSSD / diameter and as MSPD / 100 px."""
    return {"scene_id": key[0], "im_id": key[1], "obj_id": key[2], "score": score, "vsd": [[v] * 10 for v in errs],
            "mssd": [v * DIAM.get(key[2], 1.0) for v in errs], "mspd": [v * 100.0 for v in errs]}


def _table():
    A, B, C = (1, 0, 1), (1, 0, 2), (2, 0, 1)
    targets = [{"scene_id": k[0], "im_id": k[1], "obj_id": k[2], "inst_count": n} for k, n in ((A, 2), (B, 1), (C, 2))]
    rows = [
        _row(A, 0.1, [0.9, 0.0]),      # a third row of a target with inst_count 2: the surplus, ignored though it fits instance 1
        _row(A, 0.9, [0.0, 0.9]),      # rank 0 (equal scores: input order): takes instance 0
        _row((9, 9, 9), 1.0, [0.0]),   # no target
        _row(A, 0.9, [0.0, 0.0]),      # rank 1: instance 0 is taken, instance 1 fits
        _row(C, 0.5, [0.0, 0.0]),      # matched to instance 0 (the lowest of equal errors), which is not valid: not counted
    ]                                  # B has no row: E = 0
    return targets, rows, {C: [False, True]}


@pytest.mark.parametrize("which", ["package", "restatement"])
def test_instance_recall_on_a_hand_made_table(which):
    targets, rows, valid = _table()
    if which == "package":
        got = bop_eval.instance_recall(rows, targets, DIAM, 640, valid=valid, matcher=rm.match_instances)
        assert got["targets"] == 3 and got["estimates"] == 3
    else:
        got = rm.instance_recall(rows, targets, DIAM, 640, valid)
    match = np.asarray(got["match"])
    assert match.shape == (3, 12, 10) and match.dtype == np.int32
    # rows of match: A's rank 0, A's rank 1, C's row; the same in every column
    assert (match == np.array([0, 1, 0])[:, None, None]).all()
    # two counted matches over 2 + 1 + 2 instances, in every column
    assert got["recall_mssd"] == [2 / 5.0] * 10 == got["recall_mspd"] and got["recall_vsd"] == [[2 / 5.0] * 10] * 10
    for k in ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR"):
        assert got[k] == pytest.approx(0.4, abs=1e-15), k
    # had the equal scores been ordered the other way, the (0, 0) row would take instance 0 and the (0, 0.9) row nothing:
    swapped = [rows[0], rows[3], rows[2], rows[1], rows[4]]
    other = (bop_eval.instance_recall(swapped, targets, DIAM, 640, valid=valid, matcher=rm.match_instances) if which == "package"
             else rm.instance_recall(swapped, targets, DIAM, 640, valid))
    assert (np.asarray(other["match"])[:2] == np.array([0, -1])[:, None, None]).all() and other["recall_mssd"] == [1 / 5.0] * 10
    # every instance valid by default: C's match counts
    full = (bop_eval.instance_recall(rows, targets, DIAM, 640, matcher=rm.match_instances) if which == "package"
            else rm.instance_recall(rows, targets, DIAM, 640))
    assert full["recall_mspd"] == [3 / 5.0] * 10 and np.array_equal(full["match"], match)


def test_tables_handed_to_the_matcher():
    """What instance_recall asks of match_instances: errors [e][g] row-major per group, E = min(rows, inst_count), G, the
    valid flags, and 8.8's own threshold expressions."""
    targets, rows, valid = _table()
    seen = {}

    def spy(err, E, G, val, thr):
        seen.update(err=np.array(err), E=list(E), G=list(G), valid=np.asarray(val).tolist(), thr=np.array(thr))
        return rm.match_instances(err, E, G, val, thr)
    bop_eval.instance_recall(rows, targets, DIAM, 1280, valid=valid, matcher=spy)
    assert seen["E"] == [2, 0, 2 - 1] and seen["G"] == [2, 1, 2] and seen["valid"] == [True, True, True, False, True]
    assert seen["err"].shape == (2 * 2 + 0 + 1 * 2, 12)
    assert seen["err"][:, 0].tolist() == [0.0, 0.9, 0.0, 0.0, 0.0, 0.0] and seen["err"][1, 10:].tolist() == [0.9 * 100.0, 0.9 * 100.0]
    thr = seen["thr"]
    assert thr.shape == (3, 12, 10)
    for j in range(10):
        th = bop_eval.THETAS[j]
        assert (thr[:, :10, j] == th).all() and thr[0, 10, j] == th * 100.0 and thr[1, 10, j] == th * 50.0
        assert thr[2, 11, j] == (5.0 * (j + 1)) * (1280 / 640.0)


def test_one_instance_everywhere_equals_average_recall():
    th = bop_eval.THETAS[5]

    def row(s, i, o, score, vsd, mssd, mspd):
        return {"scene_id": s, "im_id": i, "obj_id": o, "score": score, "vsd": [vsd] * 10, "mssd": mssd, "mspd": mspd}
    rng = np.random.default_rng(5)
    targets = [(1, 0, 1), (1, 1, 1), (1, 1, 2), (2, 5, 2)] + [(3, i, 1 + i % 2) for i in range(20)]
    rows = [row(1, 0, 1, 0.9, 0.0, 0.0, 0.0), row(1, 1, 1, 0.2, 0.0, 0.0, 0.0), row(1, 1, 1, 0.8, th, th * 100.0, 30.0),
            row(1, 1, 1, 0.8, 0.0, 0.0, 0.0),                  # an equal score later in the input: not the estimate
            row(1, 1, 2, 0.5, 2.0, 1e9, float("inf")), row(9, 9, 9, 1.0, 0.0, 0.0, 0.0)]
    for i in range(20):
        if i % 7 != 3:
            for _ in range(1 + i % 3):
                rows.append(row(3, i, 1 + i % 2, float(rng.integers(0, 3)), float(rng.random() * 0.6), float(rng.random() * 60.0),
                                float(rng.random() * 60.0)))
    rows[9]["vsd"] = [float("nan")] * 10
    for width in (640, 1280, 123):
        want = bop_eval.average_recall(rows, targets, DIAM, width)
        for tg in (targets, [{"scene_id": s, "im_id": i, "obj_id": o, "inst_count": 1} for s, i, o in targets]):
            got = bop_eval.instance_recall(rows, tg, DIAM, width, matcher=rm.match_instances)
            for k in KEYS + ("targets", "estimates"):
                assert got[k] == want[k], (k, width)
            assert set(got) == set(want) | {"match"} and got["match"].shape == (want["estimates"], 12, 10)
            assert set(np.unique(got["match"])) <= {-1, 0}
            ref = rm.instance_recall(rows, tg, DIAM, width)
            for k in KEYS:
                assert ref[k] == want[k], (k, width)
            assert np.array_equal(ref["match"], got["match"])
    assert 0.0 < want["AR"] < 1.0
    # no row of any target: every column empty, as average_recall has it
    none = bop_eval.instance_recall(rows[5:6], targets, DIAM, 640, matcher=rm.match_instances)
    want = bop_eval.average_recall(rows[5:6], targets, DIAM, 640)
    assert all(none[k] == want[k] for k in KEYS + ("targets", "estimates")) and none["match"].shape[0] == 0


class _Stub:
    """A dataset whose checks fire before any device work."""

    def __init__(self, targets, n_gt):
        self.targets, self.n_gt = targets, n_gt

    def model_info(self, obj_id):
        return {"diameter": 1.0}

    def gt_poses(self, scene_id, im_id, obj_id):
        return np.tile(np.eye(4), (self.n_gt, 1, 1))


def test_refusals():
    key = (1, 0, 1)
    tg = lambda n: [{"scene_id": 1, "im_id": 0, "obj_id": 1, "inst_count": n}]  # noqa: E731
    ok = bop_eval.instance_recall([_row(key, 1.0, [0.0] * 64)], tg(64), DIAM, 640, matcher=rm.match_instances)
    assert ok["recall_mssd"] == [1 / 64.0] * 10
    for fn in (lambda r, t: bop_eval.instance_recall(r, t, DIAM, 640, matcher=rm.match_instances),
               lambda r, t: rm.instance_recall(r, t, DIAM, 640)):
        with pytest.raises(ValueError):
            fn([_row(key, 1.0, [0.0] * 65)], tg(2))                       # G = 65
        with pytest.raises(ValueError):
            fn([_row(key, 1.0, [0.0])], tg(65))                          # inst_count = 65
        with pytest.raises(ValueError):
            fn([_row(key, 1.0, [0.0])], tg(0))
        with pytest.raises(ValueError):
            fn([_row(key, 1.0, [0.0])], tg(1) + tg(1))                   # a target listed twice
        with pytest.raises(ValueError):
            fn([_row(key, 1.0, [0.0])], [])
    with pytest.raises(ValueError, match=re.escape("(1, 0, 1)")):
        bop_eval.evaluate([], _Stub(tg(2), 65), multi_instance=True)     # names the target
    with pytest.raises(ValueError, match=re.escape("(1, 0, 1)")):
        bop_eval.evaluate([], _Stub(tg(65), 2), multi_instance=True)
    with pytest.raises(ValueError):
        bop_eval.evaluate([], _Stub(tg(1) + tg(1), 1), multi_instance=True)
    with pytest.raises(ValueError):                                       # rows of one target disagree about G
        bop_eval.instance_recall([_row(key, 1.0, [0.0, 0.1]), _row(key, 0.5, [0.0])], tg(2), DIAM, 640, matcher=rm.match_instances)
    with pytest.raises(ValueError):
        bop_eval.instance_recall([_row(key, 1.0, [0.0, 0.1])], tg(2), DIAM, 640, valid={key: [True]}, matcher=rm.match_instances)
    # the tables of match_instances are checked before the device is touched
    thr = np.ones((1, 3, 10))
    for kw in (dict(E=[65]), dict(G=[0]), dict(G=[65]), dict(E=[-1]), dict(E=[1, 1]), dict(thr=np.ones((1, 2, 10))),
               dict(thr=np.ones((1, 19, 10))), dict(thr=np.ones((1, 3, 9))), dict(err=np.zeros((3, 3))), dict(valid=[True])):
        args = dict(err=np.zeros((2, 3)), E=[1], G=[2], valid=[True, True], thr=thr)
        args.update(kw)
        with pytest.raises(ValueError):
            bop_eval.match_instances(**args)
    # the single-instance path refuses as before
    with pytest.raises(ValueError):
        bop_eval.average_recall([], tg(2), DIAM, 640)
    # vsd_pairs: the pair table is checked on the host first
    class HostMesh:
        device = "cpu"
    eye, depth, K = np.eye(4)[None], np.ones((4, 4), np.float32), np.array([[10.0, 0, 2], [0, 10.0, 2], [0, 0, 1]])
    for pairs in ([[1, 0, 0]], [[0, 1, 0]], [[0, 0, 1]], [[-1, 0, 0]], [[0, 0]], [[0.0, 0.0, 0.0]], np.zeros((0, 3), int)):
        with pytest.raises(ValueError):
            bop_eval.vsd_pairs(HostMesh(), 0.1, depth, K, eye, eye, pairs)
    for kw in (dict(chunk=0), dict(chunk=257), dict(taus=[]), dict(diameter=0.0), dict(delta=-1.0)):
        args = dict(mesh=HostMesh(), diameter=0.1, depth_obs=depth, cam_K=K, pose_est=eye, pose_gt=eye, pairs=[[0, 0, 0]])
        args.update(kw)
        with pytest.raises(ValueError):
            bop_eval.vsd_pairs(**args)


def _folder(tmp_path, with_gt_info=True):
    V, F = rb.prism_mesh()
    poses = [np.eye(4) for _ in range(4)]
    for n, T in enumerate(poses):
        T[:3, 3] = [10.0 * n, -5.0, 700.0 + n]
    scenes = {0: (np.full((6, 8), 900), poses[:3], [1.0, 0.05, 0.1]), 4: (np.full((6, 8), 900), poses[3:], [0.7])}
    K = [[100.0, 0, 4.0], [0, 100.0, 3.0], [0, 0, 1]]
    return poses, rm.write_bop_folder(str(tmp_path), V * 1000.0, F, 116.0, scenes, K, with_gt_info=with_gt_info)


def test_bop_folder_lists_every_instance(tmp_path):
    poses, targets = _folder(tmp_path)
    ds = bop_eval.BopFolder(str(tmp_path), "multi", "test")
    assert ds.targets == targets and [t["inst_count"] for t in targets] == [3, 1]
    assert np.array_equal(ds.gt_poses(0, 0, 1), np.stack(poses[:3])) and np.array_equal(ds.gt_poses(4, 0, 1), np.stack(poses[3:]))
    assert ds.gt_visib(0, 0, 1).tolist() == [1.0, 0.05, 0.1] and ds.gt_visib(4, 0, 1).tolist() == [0.7]
    with pytest.raises(ValueError):
        ds.gt_poses(0, 0, 2)
    # the single-instance reader keeps refusing the image that holds three
    with pytest.raises(ValueError):
        ds.gt_pose(0, 0, 1)
    assert np.array_equal(ds.gt_pose(4, 0, 1), poses[3])


def test_bop_folder_without_gt_info_supplies_no_visibility(tmp_path):
    _folder(tmp_path, with_gt_info=False)
    assert bop_eval.BopFolder(str(tmp_path), "multi", "test").gt_visib(0, 0, 1) is None


def test_command_line_flags(tmp_path, monkeypatch, capsys):
    from ossid_code_amd import pipeline
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_bop19
    _folder(tmp_path / "data")
    path = pipeline.save_results_bop([{"scene_id": 0, "im_id": 0, "obj_id": 1, "score": 1.0, "pose": np.eye(4)}], str(tmp_path),
                                     "m", "multi")
    calls = []

    def fake_evaluate(res, dataset, **kw):
        calls.append(kw)
        return {"AR_VSD": 0.5, "AR_MSSD": 0.25, "AR_MSPD": 0.75, "AR": 0.5, "targets": 2, "estimates": 1, "rows": [1],
                "match": np.zeros((1, 12, 10), np.int32)}
    monkeypatch.setattr(bop_eval, "evaluate", fake_evaluate)
    base = ["--result_filenames=" + path, "--datasets_path", str(tmp_path / "data")]
    eval_bop19.main(base)
    eval_bop19.main(base + ["--multi_instance"])
    out = eval_bop19.main(base + ["--multi_instance", "--visib_gt_min=0.25"])[path]
    assert calls == [{}, {"multi_instance": True, "visib_gt_min": 0.1}, {"multi_instance": True, "visib_gt_min": 0.25}]
    assert "match" not in out and "rows" not in out and out["AR"] == 0.5
    assert "AR_MSPD 0.750000" in capsys.readouterr().out


def test_header_declares_the_pair_and_match_entry_points():
    from ossid_code_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ossid_hip.h")).read(), flags=re.S)
    for name, nargs in (("ossid_bop_vsd_pairs", 18), ("ossid_bop_match", 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.exported_symbols() and len(_lib._PROTOS[name][1]) == nargs
    assert _lib.BOP_MAX_INSTANCES == bop_eval.MAX_INSTANCES == rm.MAX_INSTANCES == 64
    assert not [n for n in _lib.exported_symbols() if n.startswith("ossid_bop") and "workspace" in n]
