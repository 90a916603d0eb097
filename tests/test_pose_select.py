"""SPEC.md section 16 (distinct-pose selection) on the CPU: the restatement tests/ref_pose_select.py against answers written
out by hand (tests/pose_select_cases.py), the refusals scoring.select_instances makes before it touches the device, and the
header's declaration. tests/test_pose_select_gpu.py holds the kernel to the restatement."""
import os
import re

import numpy as np
import pytest

import pose_select_cases as pc
import ref_pose_select as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", sorted(pc.CASES))
def test_restatement_gives_the_answers_written_out(case):
    poses, scores, K, sep, syms, min_score, want_sel, want_owner = pc.CASES[case]
    sel, count, owner = rp.select(poses, scores, pc.POINTS, K, sep, syms, min_score)
    assert sel.dtype == owner.dtype == count.dtype == np.int32 and count.shape == (1,)
    assert sel.tolist() == want_sel and owner.tolist() == want_owner
    assert int(count[0]) == sum(v >= 0 for v in want_sel)


def test_the_threshold_is_met_exactly():
    """Every point of a pure translation by 0.25 has q = 0.0625 bit for bit: the two threshold cases differ by one ulp of sep."""
    poses = pc.CASES["threshold_equal"][0]
    D = rp.distances(poses, 0, pc.POINTS, np.eye(4)[None])
    assert D.tolist() == [0.0, 0.0625] and 0.25 * 0.25 == 0.0625 and pc.BELOW * pc.BELOW < 0.0625


def test_a_non_finite_pose_is_picked_and_owns_only_itself():
    poses = np.stack([pc.at(0.0), pc.at(0.01), pc.at(0.02)])
    poses[1, 0, 3] = np.nan
    sel, count, owner = rp.select(poses, [1, 3, 2], pc.POINTS, 3, 0.1)
    assert sel.tolist() == [1, 2, -1] and owner.tolist() == [1, 0, 1] and count.tolist() == [2]
    assert rp.distances(poses, 1, pc.POINTS, np.eye(4)[None]).tolist() == [np.inf] * 3


def test_wrapper_refusals_need_no_device():
    from ossid_code_amd import scoring
    T, s, P = np.tile(np.eye(4), (3, 1, 1)), np.ones(3, np.float32), pc.POINTS
    bad_pose = T.copy()
    bad_pose[1, 2, 3] = np.inf
    for kw in (dict(poses=np.eye(4)), dict(poses=np.zeros((3, 3, 4))), dict(poses=np.zeros((0, 4, 4)), scores=np.zeros(0)),
               dict(poses=bad_pose), dict(poses=T.astype(np.int64)), dict(scores=np.ones(2)), dict(scores=np.ones((3, 2))),
               dict(scores=np.ones((1, 3))), dict(scores=np.ones(3, np.int32)), dict(model_points=np.zeros((0, 3), np.float32)),
               dict(model_points=np.zeros((4, 2), np.float32)), dict(model_points=np.zeros(3, np.float32)),
               dict(max_instances=0), dict(max_instances=65), dict(max_instances=1.5), dict(sep=-0.1), dict(sep=np.inf),
               dict(sep=np.nan), dict(min_score=np.nan), dict(symmetries=np.eye(4)), dict(symmetries=np.zeros((0, 4, 4))),
               dict(symmetries=np.zeros((4097, 4, 4))), dict(symmetries=np.zeros((2, 3, 4))),
               dict(poses=np.zeros((65537, 4, 4)), scores=np.zeros(65537, np.float32))):
        args = dict(poses=T, scores=s, model_points=P, max_instances=2, sep=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            scoring.select_instances(**args)
    with pytest.raises(ValueError):
        rp.select(T, s, P, 65, 0.1)
    with pytest.raises(ValueError):
        rp.select(T, s, P, 2, -1.0)


def test_header_declares_the_selection_entry_point():
    from ossid_code_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ossid_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ossid_pose_select\s*\(", text)
    assert "ossid_pose_select" in _lib.exported_symbols() and len(_lib._PROTOS["ossid_pose_select"][1]) == 15
    assert _lib.SELECT_MAX_POSES == rp.MAX_POSES == 65536 and _lib.BOP_MAX_INSTANCES == rp.MAX_INSTANCES
    assert _lib.BOP_MAX_SYMMETRIES == rp.MAX_SYMMETRIES and _lib.ABI_VERSION == 6
    # caller-owned outputs only: no workspace, no size query
    assert not [n for n in _lib.exported_symbols() if "select" in n and n != "ossid_pose_select"]
