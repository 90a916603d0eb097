"""CPU tests of the model cloud from a mesh (SPEC.md section 9): the surface exists, the restatement
tests/ref_model_cloud.py has the properties the definition relies on, every cap is refused before any device work, and
ModelCloud.save writes the reference's npz. The kernels themselves are tested in tests/test_model_cloud_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import ref_model_cloud as rm
import ref_raster as rr
import ref_raster_color as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_mesh(level=1, colors=True):
    from ossid_code_amd import render
    V, F = rr.bump_mesh(level)
    return render.Mesh(V, F, device="cpu", colors=rc.axis_colors(V)[0] if colors else None)


def test_the_surface_exists():
    from ossid_code_amd import _lib, model_cloud
    for name in ("sample_model_cloud", "fps", "mesh_diameter", "ModelCloud"):
        assert hasattr(model_cloud, name)
    header = open(os.path.join(ROOT, "include", "ossid_hip.h")).read()
    for name in ("ossid_cloud_workspace_bytes", "ossid_cloud_votes", "ossid_cloud_weights", "ossid_cloud_candidates",
                 "ossid_cloud_fps", "ossid_mesh_diameter"):
        assert name in _lib.exported_symbols() and re.search(r"\b%s\s*\(" % name, header)
    assert "online_learning.py:303-311" in header
    assert (_lib.CLOUD_MAX_POINTS, _lib.CLOUD_MAX_CANDIDATES, _lib.MESH_DIAMETER_MAX_VERTICES) == \
        tuple(int(re.search(r"#define\s+%s\s+(\d+)" % k, header).group(1))
              for k in ("OSSID_CLOUD_MAX_POINTS", "OSSID_CLOUD_MAX_CANDIDATES", "OSSID_MESH_DIAMETER_MAX_VERTICES"))


def test_library_exports_the_cloud_entry_points(hiplib):
    for name in ("ossid_cloud_workspace_bytes", "ossid_cloud_votes", "ossid_cloud_weights", "ossid_cloud_candidates",
                 "ossid_cloud_fps", "ossid_mesh_diameter"):
        assert hasattr(hiplib.lib(), name), name
    ws = hiplib.lib().ossid_cloud_workspace_bytes
    assert ws(0) == 0 and ws(hiplib.RASTER_MAX_FACES + 1) == 0 and ws(1) >= 8 * (1 + 1 + 1024) and ws(1) % 8 == 0
    # OSSID_EINVAL (-22) before any launch: no device is touched
    assert hiplib.lib().ossid_cloud_fps(None, 8, 4, None, None, None) == -22
    assert hiplib.lib().ossid_mesh_diameter(None, 0, None, None) == -22


def test_r2_multipliers_are_odd_so_the_sequence_is_a_bijection():
    assert rm.R1 % 2 == 1 and rm.R2 % 2 == 1                    # odd: invertible modulo 2^32
    for m in (rm.R1, rm.R2):
        inv = pow(m, -1, 1 << 32)
        assert (m * inv) % (1 << 32) == 1
        k = np.arange(1 << 16, dtype=np.uint64)
        assert len(np.unique((k * np.uint64(m)) & np.uint64(0xFFFFFFFF))) == len(k)
    w0, u, v = rm.barycentric(32768)
    assert (w0 >= 0).all() and (u > 0).all() and (v > 0).all() and (u + v <= 1.0).all()
    assert np.array_equal((w0 + u) + v, np.ones(32768))         # multiples of 2^-33 below 2: the arithmetic is exact


def test_weights_and_strata_of_the_restatement():
    V, F = rr.bump_mesh(3)
    V32 = rm.f32_vertices(V)
    votes = np.ones((len(F), 2), dtype=np.int64)
    votes[::7] = 0                                              # some faces never seen
    w, P, nrm, usable = rm.weights(V32, F, votes)
    assert not usable[::7].any() and usable.sum() == len(F) - len(F[::7]) and not w[~usable].any() and not nrm[~usable].any()
    assert int(w.max()) == 1 << 32 and int(P[-1]) == sum(int(x) for x in w) < 1 << 54
    # the bound behind "under 2^54": at most 2^22 faces of weight at most 2^32
    from ossid_code_amd import _lib
    assert _lib.RASTER_MAX_FACES * (1 << 32) <= 1 << 54
    assert np.abs(np.sqrt((nrm[usable].astype(np.float64) ** 2).sum(1)) - 1.0).max() < 1e-6
    for K in (1, 7, 2048, 32768):
        tau = rm.strata(int(P[-1]), K)
        assert all(b > a for a, b in zip(tau, tau[1:])) and 0 <= tau[0] and tau[-1] < int(P[-1])
    pts, cn, col, face = rm.candidates(V32, F, rc.axis_colors(V)[0], votes, P, nrm, 2048)
    assert usable[face].all() and (np.diff(face) >= 0).all() and col.min() >= 0 and col.max() <= 1


def test_restated_fps_spreads_and_breaks_ties_to_the_lowest_index():
    g = np.arange(4, dtype=np.float32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    sel, rad = rm.fps(P, 8)
    assert sel[0] == 0 and rad[0] == np.inf and sel[1] == 63 and rad[1] == 27.0     # the opposite corner
    # 10 = min(|p|^2, |p - (3,3,3)|^2) at (0,1,3), (0,3,1), (1,0,3), ...: a tie, the lowest index wins
    assert sel[2] == 7 and rad[2] == 10.0
    assert (np.diff(rad[1:]) <= 0).all() and len(set(sel.tolist())) == 8


def test_caps_are_refused_before_any_device_work():
    from ossid_code_amd import model_cloud, render
    mesh = _cpu_mesh()
    bad = [dict(n_points=0), dict(n_points=4097), dict(n_points=2048, oversample=17), dict(oversample=0), dict(level=-1),
           dict(level=4), dict(view_size=15), dict(view_size=1025), dict(views_per_call=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            model_cloud.sample_model_cloud(mesh, **kw)
    with pytest.raises(ValueError, match="vertex colours"):
        model_cloud.sample_model_cloud(_cpu_mesh(colors=False))
    V, F = rr.bump_mesh(1)
    with pytest.raises(ValueError, match="no faces"):
        model_cloud.sample_model_cloud(render.Mesh(V, F[:0], device="cpu", colors=rc.axis_colors(V)[0]))
    Vn = V.copy()
    Vn[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        model_cloud.sample_model_cloud(render.Mesh(Vn, F, device="cpu", colors=rc.axis_colors(V)[0]))
    # inside the caps a mesh that is not on the GPU is an error, never a CPU computation
    with pytest.raises(RuntimeError, match="GPU only"):
        model_cloud.sample_model_cloud(mesh)
    P = np.zeros((8, 3), dtype=np.float32)
    for m in (0, 9, 4097):
        with pytest.raises(ValueError):
            model_cloud.fps(P, m)
    with pytest.raises(ValueError):
        model_cloud.fps(np.zeros((32769, 3), dtype=np.float32), 4)
    P[5, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        model_cloud.fps(P, 4)
    with pytest.raises(ValueError):
        model_cloud.mesh_diameter(np.zeros((262145, 3), dtype=np.float32))
    with pytest.raises(ValueError):
        model_cloud.mesh_diameter(np.zeros((0, 3), dtype=np.float32))


def test_save_round_trips_the_reference_keys(tmp_path):
    from ossid_code_amd import model_cloud
    rng = np.random.default_rng(0)
    pts, nrm, col = (torch.from_numpy(rng.random((64, 3)).astype(np.float32)) for _ in range(3))
    cloud = model_cloud.ModelCloud(pts, nrm, col, 0.125)
    assert len(cloud) == 64 and set(cloud.as_dict()) == {"model_points", "model_normals", "model_colors"}
    path = str(tmp_path / "model_cloud_01.npz")
    cloud.save(path)
    with np.load(path) as z:
        assert set(z.files) == {"model_points", "model_colors", "model_normals", "diameter"}
        for key, t in (("model_points", pts), ("model_colors", col), ("model_normals", nrm)):
            assert z[key].dtype == np.float64 and z[key].shape == (64, 3)
            assert np.array_equal(z[key].astype(np.float32), t.numpy())         # f32 -> f64 -> f32 is the identity
        assert float(z["diameter"]) == 0.125


def test_stream_takes_a_frames_own_cloud_as_it_is():
    from ossid_code_amd.stream import OnlineStream
    s = OnlineStream(None, None, None, meshes={})
    frame = {"obj_id": 3, "model_points": np.zeros((4, 3))}
    assert s._with_cloud(frame) is frame
    with pytest.raises(KeyError, match="no model_points"):
        s._with_cloud({"obj_id": 3})
    with pytest.raises(KeyError, match="no model_points"):
        OnlineStream(None, None, None)._with_cloud({"obj_id": 3})
