"""CPU checks of the PPF hypotheses step (SPEC.md section 6): the restatement tests/ref_ppf.py recovers the object on the
asymmetric test scene, the PLY reader, the drop-in's argument checks, the header entries and the compat mapping."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ref_ppf as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    P, N = rp.object_model()
    return rp.Model(P, N, 0.03)


@pytest.mark.parametrize("k", range(len(rp.POSES)))
def test_restatement_recovers_the_true_pose(model, k):
    """Mask = the object's box x1.2, background included. Measured: best hypothesis 0.007-0.018 D / 1.4-3.5 degrees."""
    depth, K, mask, T = rp.scene(k)
    poses, scores = rp.find(model, rp.depth2cloud(depth, mask, K))
    assert 0 < len(poses) <= 100 and np.all(np.diff(scores) <= 0)
    dt, dr = rp.best_gap(poses, T, model.D)
    assert dt <= 0.025 and dr <= 5.0, (dt, dr)


def test_restatement_sector_bins_are_twelve_degrees():
    tab = rp.tables(np.float32(0.01), np.float32(1.0))
    deg = np.arange(0.5, 360.0, 1.0)
    u, v = np.cos(np.deg2rad(deg)).astype(np.float32), np.sin(np.deg2rad(deg)).astype(np.float32)
    assert np.array_equal(rp.sector(u, v, tab), (deg // 12).astype(np.int64))


def _write_ply(path, V, Nrm, fmt):
    n = len(V)
    head = ["ply", "format %s 1.0" % fmt, "comment made by a test", "element vertex %d" % n,
            "property float x", "property float y", "property float z", "property float nx", "property float ny",
            "property float nz", "property uchar red", "property uchar green", "property uchar blue",
            "property float texture_u", "element face 2", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if fmt == "ascii":
            for p, q in zip(V, Nrm):
                f.write(("%r %r %r %r %r %r 10 20 30 0.5\n" % tuple(float(x) for x in (*p, *q))).encode())
            f.write(b"3 0 1 2\n4 0 1 2 3\n")
        else:
            dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                           ("r", "u1"), ("g", "u1"), ("b", "u1"), ("tu", "<f4")])
            a = np.zeros(n, dtype=dt)
            for i, k in enumerate(("x", "y", "z")):
                a[k], a["n" + k] = V[:, i], Nrm[:, i]
            f.write(a.tobytes())
            f.write(np.array([3], "u1").tobytes() + np.array([0, 1, 2], "<i4").tobytes())
            f.write(np.array([4], "u1").tobytes() + np.array([0, 1, 2, 3], "<i4").tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
def test_ply_round_trip(tmp_path, fmt):
    from ossid_code_amd.ppf import read_ply
    rng = np.random.default_rng(0)
    V = rng.normal(size=(50, 3)).astype(np.float32) * 100
    Nrm = rng.normal(size=(50, 3)).astype(np.float32)
    path = str(tmp_path / "m.ply")
    _write_ply(path, V, Nrm, fmt)
    P, N = read_ply(path)
    assert np.array_equal(P.astype(np.float32), V) and np.array_equal(N.astype(np.float32), Nrm)


def test_ply_without_normals_is_refused(tmp_path):
    from ossid_code_amd.ppf import read_ply
    path = tmp_path / "m.ply"
    path.write_text("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"
                    "end_header\n0 0 0\n")
    with pytest.raises(ValueError, match="nx ny nz"):
        read_ply(str(path))


def test_drop_in_refuses_before_device_work():
    from ossid_code_amd.ppf import PPFModel
    m = PPFModel.__new__(PPFModel)                      # no model built: any device work would fail on missing state
    pc = np.zeros((10, 3))
    with pytest.raises(ValueError, match="accepted: SceneSamplingDist"):
        m.find_surface_model(pc, SceneSamplingDistance=0.03)
    with pytest.raises(ValueError, match="DensePoseRefinement"):
        m.find_surface_model(pc, DensePoseRefinement='true')
    with pytest.raises(ValueError, match="normals"):
        PPFModel(np.zeros((10, 3)))


def test_header_declares_the_ppf_entries():
    text = open(os.path.join(ROOT, "include", "ossid_hip.h")).read()
    for name in ("ossid_ppf_sample", "ossid_ppf_sample_workspace_bytes", "ossid_ppf_model_table",
                 "ossid_ppf_model_table_words", "ossid_ppf_scene_normals", "ossid_ppf_vote",
                 "ossid_ppf_vote_workspace_bytes", "ossid_ppf_cluster"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    from ossid_code_amd import _lib
    assert "#define OSSID_PPF_MAX_MODEL_POINTS %d" % _lib.PPF_MAX_MODEL_POINTS in text
    assert "#define OSSID_PPF_MAX_SCENE_SAMPLES %d" % _lib.PPF_MAX_SCENE_SAMPLES in text


@pytest.mark.parametrize("flag", [True, False])
def test_compat_maps_ppf_only_when_asked(flag):
    code = ("import ossid_code_amd.compat as c; c.install(%s)\n"
            "try:\n    from zephyr.utils.halcon_wrapper import PPFModel; print('mapped', PPFModel.__module__)\n"
            "except ImportError:\n    print('absent')\n" % ("ppf=True" if flag else ""))
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == ("mapped ossid_code_amd.ppf" if flag else "absent")
