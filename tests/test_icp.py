"""CPU checks of the ICP refinement step (SPEC.md section 5): the numpy restatement tests/ref_icp.py against scipy, its
convergence on the asymmetric test scene, and the drop-in wiring (compat name, header entry, argument checks)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_icp as ri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_oracle_correspondences_equal_a_kd_tree_query():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(3)
    md = 0.01
    for n_src, n_q in ((700, 900), (2048, 2048), (50, 300)):
        Q = rng.uniform(0.0, 0.12, size=(n_q, 3)).astype(np.float32)
        src = rng.uniform(-0.01, 0.13, size=(n_src, 3)).astype(np.float32)
        si, qi, d2 = ri.correspondences(src, Q, md)
        dd, ii = cKDTree(Q.astype(np.float64)).query(src.astype(np.float64), k=2, distance_upper_bound=md)
        dist, idx = dd[:, 0], ii[:, 0]
        # f32 and f64 distances can only disagree at the threshold itself or between two near-equal candidates
        clear = (np.abs(dist - md) > 1e-5 * md) & ~(dd[:, 1] - dd[:, 0] < 1e-5 * md)
        ok = np.isfinite(dist) & (dist <= md)
        mine = np.zeros(n_src, dtype=bool)
        mine[si] = True
        assert np.array_equal(mine[clear], ok[clear])
        both = np.nonzero(mine & ok)[0]
        both = both[clear[both]]
        assert np.array_equal(qi[np.searchsorted(si, both)], idx[both])
        assert ok.sum() > 0


def test_oracle_ties_go_to_the_lowest_index():
    Q = np.array([[1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    si, qi, _ = ri.correspondences(np.zeros((1, 3), dtype=np.float32), Q, 2.0)
    assert list(si) == [0] and list(qi) == [0]


def test_kabsch_recovers_a_known_transform():
    rng = np.random.default_rng(0)
    s = rng.normal(size=(100, 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ri.rot([1, 2, 3], 40), [0.1, -0.2, 0.3]
    q = s @ T[:3, :3].T + T[:3, 3]
    assert np.abs(ri.kabsch(s, q) - T).max() < 1e-12
    mirrored = s * [1, 1, -1]                           # the reflection fix keeps det R = +1
    assert np.linalg.det(ri.kabsch(mirrored, s)[:3, :3]) > 0


def test_oracle_converges_on_the_noiseless_asymmetric_scene():
    """From 2.5-3 degrees and 4 mm off, the oracle reaches the same pose as from the true pose: the optimum of SPEC 5 on
    this scene (0.6 mm / 1.2 degrees from T_gt: the targets sit at the truncated pixel corners of SPEC 3.2)."""
    depth, K, T_gt, P = ri.scene()
    uv = ri.project_uv(T_gt, P, K)
    opt, _, _, _ = ri.icp(depth, uv, T_gt, K, P)
    for axis, deg, dt in (([1, 0.5, 0], 2.5, [0.003, -0.002, 0.002]), ([0, 1, 1], -3.0, [-0.002, 0.003, -0.002])):
        T0 = ri.perturb(T_gt, axis, deg, dt)
        T, fit, rmse, it = ri.icp(depth, uv, T0, K, P)
        dt_mm, da = ri.pose_gap(T, opt)
        assert dt_mm < 5e-5 and da < 0.15, (dt_mm, da)       # the stopping rule ends within 0.1 degree of it
        assert ri.pose_gap(T, T_gt)[0] < 1e-3
        assert ri.add_error(T, T_gt, P) < 0.3 * ri.add_error(T0, T_gt, P)
        assert fit == 1.0 and rmse < 1e-3 and 1 <= it <= 30


def test_compat_install_resolves_icp_refinement():
    code = ("import ossid_code_amd.compat as c; c.install();"
            "from zephyr.utils.icp import icpRefinement;"
            "from zephyr.utils import projectPointsUv;"
            "print('ok', icpRefinement.__module__, icpRefinement.__name__)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "ok ossid_code_amd.pipeline icpRefinement" in out.stdout


def test_header_declares_the_icp_entry():
    from ossid_code_amd import _lib
    text = open(os.path.join(ROOT, "include", "ossid_hip.h")).read()
    assert re.search(r"\bint ossid_icp_refine\(", text)
    assert int(re.search(r"#define\s+OSSID_ICP_MAX_POINTS\s+(\d+)", text).group(1)) == _lib.ICP_MAX_POINTS == 2048
    assert "ossid_icp_refine" in _lib.exported_symbols()


def test_icp_refinement_refuses_inpainting():
    from ossid_code_amd import pipeline
    with pytest.raises(ValueError, match="inpaint_depth=False"):
        pipeline.icpRefinement(np.zeros((4, 4), np.float32), np.zeros((3, 2), np.int64), np.eye(4), np.eye(3),
                               np.zeros((3, 3)), inpaint_depth=True)
