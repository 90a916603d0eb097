"""CPU checks of the dense pose refinement of PPF hypotheses (SPEC.md 6.9): the restatement tests/ref_ppf_refine.py moves
the best hypothesis to the truth on the asymmetric test scene, its correspondences equal a k-d tree query, the
DensePoseRefinement values, the header entries and the compat mapping."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_icp as ri
import ref_ppf as rp
import ref_ppf_refine as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def models():
    P, N = rp.object_model()
    return rp.Model(P, N, 0.03), rr.RefineModel(P, N)


def test_threshold_schedule(models):
    _m, rm = models
    thr = rr.thresholds(rm.D, rm.h)
    D = float(rm.D)
    assert [round(float(t) / D, 4) for t in thr] == [0.1, 0.05, 0.04, 0.04, 0.04]
    assert thr[2] == thr[3] == thr[4] == np.float32(2.0 * float(rm.h))


@pytest.mark.parametrize("k", range(len(rp.POSES)))
def test_restatement_refines_to_the_true_pose(models, k):
    """Unrefined, the best hypothesis is 0.007-0.018 D / 1.4-3.5 degrees off; refined, measured 0.0003-0.0006 D /
    0.07-0.15 degrees. Refines the three top-scored hypotheses and the one nearest the truth."""
    model, rm = models
    depth, K, mask, T = rp.scene(k)
    C = rp.depth2cloud(depth, mask, K)
    poses, _scores = rp.find(model, C)
    gaps = [ri.pose_gap(p, T) for p in poses]
    near = int(np.argmin([g[0] / float(model.D) / 0.1 + g[1] / 12.0 for g in gaps]))
    sel = sorted({0, 1, 2, near})
    _idx, S = rr.scene_points(C, rm.D)
    P, scores, pairs, steps, order = rr.refine(poses[sel], S, rm)
    assert np.all(np.diff(scores) <= 0) and sorted(order) == list(range(len(sel)))
    assert np.array_equal(scores, pairs / float(len(rm.idx)))
    dt, dr = rp.best_gap(P, T, model.D)
    assert dt <= 0.002 and dr <= 0.5, (dt, dr)
    i = [sel[o] for o in order].index(near)
    assert steps[i] == rr.REFINE_STEPS
    top = ri.pose_gap(P[0], T)                                   # the refined top score is the true pose here
    assert top[0] / float(model.D) <= 0.002 and top[1] <= 0.5, top


def test_restatement_correspondences_equal_a_kd_tree(models):
    from scipy.spatial import cKDTree
    _m, rm = models
    depth, K, mask, T = rp.scene(1)
    _idx, S = rr.scene_points(rp.depth2cloud(depth, mask, K), rm.D)
    Tp = ri.perturb(T, [0.2, 1.0, -0.3], 4.0, [0.003, -0.002, 0.001])
    thr = rr.thresholds(rm.D, rm.h)[1]
    si, mi, d2, X = rr.correspondences(Tp, S, rm.P, thr)
    dist, j = cKDTree(rm.P.astype(np.float64)).query(X.astype(np.float64), k=2)
    clear = (dist[:, 1] - dist[:, 0] > 1e-6) & (np.abs(dist[:, 0] - float(thr)) > 1e-6)
    want = np.nonzero(clear & (dist[:, 0] <= float(thr)))[0]
    got = np.isin(si, np.nonzero(clear)[0])
    assert len(want) > 500 and np.array_equal(si[got], want) and np.array_equal(mi[got], j[want, 0])


def test_dense_pose_refinement_values():
    from ossid_code_amd.ppf import PPFModel, dense_flag
    for v, want in (("true", True), ("TRUE", True), ("True", True), ("false", False), ("FaLsE", False), (True, True),
                    (False, False), (np.bool_(True), True)):
        assert dense_flag(v) is want
    for v in ("yes", "1", "", 1, 0, None, 0.0):
        with pytest.raises(ValueError, match="DensePoseRefinement"):
            dense_flag(v)
    m = PPFModel.__new__(PPFModel)                       # no model built: any device work would fail on missing state
    pc = np.zeros((10, 3))
    for v in ("true", "TRUE", True, "on"):
        with pytest.raises(ValueError, match="DensePoseRefinement"):
            m.find_surface_model(pc, DensePoseRefinement=v)
    with pytest.raises(ValueError, match="DensePoseRefinement"):
        m.find_hypotheses(np.zeros((4, 4), np.float32), np.ones((4, 4), bool), np.eye(3), DensePoseRefinement="true")


def test_header_declares_the_refine_entries():
    text = open(os.path.join(ROOT, "include", "ossid_hip.h")).read()
    for name in ("ossid_ppf_refine_grid_bytes", "ossid_ppf_refine_model_grid", "ossid_ppf_refine_workspace_bytes",
                 "ossid_ppf_refine", "ossid_ppf_refine_match"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    from ossid_code_amd import _lib
    assert "#define OSSID_PPF_MAX_REFINE_MODEL_POINTS %d" % _lib.PPF_MAX_REFINE_MODEL_POINTS in text
    assert "#define OSSID_PPF_MAX_REFINE_SCENE_POINTS %d" % _lib.PPF_MAX_REFINE_SCENE_POINTS in text


@pytest.mark.parametrize("dense", [True, False])
def test_compat_maps_the_refining_default(dense):
    code = ("import ossid_code_amd.compat as c; c.install(ppf=True%s)\n"
            "from zephyr.utils.halcon_wrapper import PPFModel\n"
            "print(PPFModel.__module__, PPFModel.__name__, PPFModel.DENSE_DEFAULT)\n"
            % (", ppf_dense_refinement=True" if dense else ""))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    want = "ossid_code_amd.ppf PPFModelDense true" if dense else "ossid_code_amd.ppf PPFModel false"
    assert out.stdout.strip() == want
