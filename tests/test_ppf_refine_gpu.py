"""Dense pose refinement of PPF hypotheses on the device (csrc/ppf_refine.hip, SPEC.md 6.9) against the numpy restatement
tests/ref_ppf_refine.py: samplings, correspondence sets (grid cell edges and exact ties included), poses after one step and
after the full run, scores and order, reproducibility, both call forms, the caps and bad arguments, and the stream."""
import types

import numpy as np
import pytest
import torch

import ref_icp as ri
import ref_ppf as rp
import ref_ppf_refine as rr
from ossid_code_amd import _lib, ppf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def obj(hiplib):
    P, N = rp.object_model()
    return P, N, rr.RefineModel(P, N), ppf.PPFModel(P, normals=N)


@pytest.fixture(scope="module")
def scenes(hiplib):
    return [rp.scene(k) for k in range(len(rp.POSES))]


def _np(t):
    return t.cpu().numpy()


def _src(depth, mask, K):
    return {"depth": torch.from_numpy(depth).cuda(), "mask": torch.from_numpy(mask.astype(np.uint8)).cuda(), "cam_K": K}


def _scene(dev, depth, mask, K):
    """The device's refinement scene sample of a frame -> (sample dict, host points)."""
    s = ppf._sample(dev.device, rr.REFINE_SAMPLING_REL, float(dev.D), _lib.PPF_MAX_REFINE_SCENE_POINTS,
                    **_src(depth, mask, K))
    n = int(_np(s["count"])[0])
    return s, _np(s["pts"])[:n]


def _refine(dev, s, poses, steps=rr.REFINE_STEPS, nh=None, NR=None):
    """ossid_ppf_refine on explicit poses -> host (poses, scores, pairs, steps done, status)."""
    R = dev.refine
    poses = torch.as_tensor(np.ascontiguousarray(poses), dtype=torch.float64).cuda()
    nh = int(poses.shape[0]) if nh is None else nh
    NR = NR or int(poses.shape[0])
    if poses.shape[0] < NR:
        poses = torch.cat([poses, torch.zeros(NR - poses.shape[0], 4, 4, dtype=torch.float64, device="cuda")]).contiguous()
    nh_t = torch.tensor([nh], dtype=torch.int32, device="cuda")
    cap = _lib.PPF_MAX_REFINE_SCENE_POINTS
    wsb = int(_lib.fn("ossid_ppf_refine_workspace_bytes")(cap, NR))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = [torch.empty(NR, 4, 4, dtype=torch.float64, device="cuda"), torch.empty(NR, dtype=torch.float64, device="cuda"),
           torch.empty(NR, dtype=torch.int32, device="cuda"), torch.empty(NR, dtype=torch.int32, device="cuda"),
           torch.empty(4, dtype=torch.int32, device="cuda")]
    rc = _lib.fn("ossid_ppf_refine")(s["pts"].data_ptr(), s["count"].data_ptr(), cap, R["grid"].data_ptr(),
                                     int(R["grid"].numel()), R["Mr"], poses.data_ptr(), nh_t.data_ptr(), NR, steps,
                                     float(dev.D), float(R["h"]), ws.data_ptr(), wsb, *[o.data_ptr() for o in out], None)
    assert rc == 0
    return [_np(o) for o in out]


def _match(dev, pts, count, poses, step, cap=None):
    """ossid_ppf_refine_match -> host int32 [len(poses), count] of matched model indices (-1: none)."""
    R = dev.refine
    cap = cap or _lib.PPF_MAX_REFINE_SCENE_POINTS
    S = torch.zeros(cap, 3, dtype=torch.float32, device="cuda")
    S[:count] = torch.from_numpy(np.ascontiguousarray(pts[:count], dtype=np.float32)).cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    T = torch.as_tensor(np.ascontiguousarray(poses), dtype=torch.float64).cuda()
    wsb = int(_lib.fn("ossid_ppf_refine_workspace_bytes")(cap, len(poses)))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    m = torch.empty(len(poses), cap, dtype=torch.int32, device="cuda")
    rc = _lib.fn("ossid_ppf_refine_match")(S.data_ptr(), cnt.data_ptr(), cap, R["grid"].data_ptr(), int(R["grid"].numel()),
                                           R["Mr"], T.data_ptr(), len(poses), R["steps"], step, float(dev.D),
                                           float(R["h"]), ws.data_ptr(), wsb, m.data_ptr(), None)
    assert rc == 0
    return _np(m)[:, :count]


def _ref_match(T, S, model, thr):
    si, mi, _d2, _X = rr.correspondences(T, S, model.P, thr)
    out = np.full(len(S), -1, dtype=np.int32)
    out[si] = mi
    return out


def _candidates(dev, depth, mask, K):
    r = dev._run(_src(depth, mask, K))
    n = ppf.check_info(r["info"], 0.05)[0]
    return r, _np(r["poses"])[:n]


def test_refinement_samplings_equal_the_restatement(obj, scenes):
    _P, _N, rm, dev = obj
    R = dev.refine
    assert R is not None and dev.refine_reason is None
    assert R["Mr"] == len(rm.idx) and R["h"] == rm.h and np.array_equal(_np(R["idx"]), rm.idx)
    assert np.array_equal(_np(R["points"]), rm.P) and np.array_equal(_np(R["normals"]), rm.N)
    for depth, K, mask, _T in scenes:
        s, S = _scene(dev, depth, mask, K)
        C = rp.depth2cloud(depth, mask, K)
        idx, Sr = rr.scene_points(C, rm.D)
        pix = np.flatnonzero(mask & (depth > 0))
        assert len(S) == len(idx) and np.array_equal(_np(s["idx"])[:len(S)], pix[idx]) and np.array_equal(S, Sr)


def test_correspondences_equal_the_brute_force(obj, scenes):
    _P, _N, rm, dev = obj
    thr = rr.thresholds(rm.D, rm.h)
    for k, (depth, K, mask, T) in enumerate(scenes):
        _s, S = _scene(dev, depth, mask, K)
        _r, cand = _candidates(dev, depth, mask, K)
        poses = np.concatenate([T[None], cand[:3], ri.perturb(T, [1.0, 0.2, 0.1], 6.0, [0.004, 0.0, -0.003])[None]])
        for step in range(rr.REFINE_STEPS):
            got = _match(dev, S, len(S), poses, step)
            for i, Tp in enumerate(poses):
                assert np.array_equal(got[i], _ref_match(Tp, S, rm, thr[step])), (k, step, i)


def test_correspondences_on_a_lattice_with_ties(hiplib):
    """Model points on a unit lattice, scene points at midpoints (exact ties between distinct model points), on lattice
    points, near the thresholds and far outside the box; identity pose, so the scene is the model frame exactly."""
    g = np.arange(10, dtype=np.float32)
    L = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.float32(2.0)
    N = np.tile(np.array([[0.0, 0.0, 1.0]], dtype=np.float32), (len(L), 1))
    dev = ppf.PPFModel(L.astype(np.float64), normals=N.astype(np.float64))
    rm = rr.RefineModel(L.astype(np.float64), N.astype(np.float64))
    assert dev.refine["Mr"] == len(rm.idx) == 1000
    rng = np.random.default_rng(3)
    thr = rr.thresholds(rm.D, rm.h)
    parts = [L[rng.integers(0, 1000, 300)] + np.float32(0.5) * np.eye(3, dtype=np.float32)[rng.integers(0, 3, 300)],
             L[rng.integers(0, 1000, 200)],
             (L[rng.integers(0, 1000, 400)] + rng.uniform(-1.5, 1.5, (400, 3))).astype(np.float32),
             np.array([[2.0 - float(t) * f, 5.0, 5.0] for t in thr for f in (1.0, 0.9999, 1.0001)], dtype=np.float32),
             np.array([[-50.0, 3.0, 3.0], [5.0, 5.0, 400.0], [11.0 + float(thr[0]), 4.0, 4.0]], dtype=np.float32)]
    S = np.concatenate(parts).astype(np.float32)
    I = np.eye(4)[None]
    for step in range(rr.REFINE_STEPS):
        got = _match(dev, S, len(S), I, step, cap=2048)[0]
        want = _ref_match(I[0], S, rm, thr[step])
        assert np.array_equal(got, want), step
    ties = _ref_match(I[0], S[:300], rm, thr[0])
    assert np.all(ties >= 0)


def _grown_grid_case(shift):
    """The lattice model and a scene at the acceptance edges of thresholds 0.2, 0.1, 0.08 (D = 2.0, smaller than the
    extent 9, so every level's own cell edge needs more than 32768 cells and is grown) -> (L, S, D, h, thr)."""
    g = np.arange(10, dtype=np.float32)
    off = np.array([2.0 + shift, 2.0, 2.0], dtype=np.float32)
    L = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + off).astype(np.float32)
    D = np.float32(2.0)
    h = rr.refine_step_h(rr.REFINE_SAMPLING_REL, D)
    thr = rr.thresholds(D, h, steps=3)
    assert [float(t) for t in thr] == [float(np.float32(v)) for v in (0.2, 0.1, 0.08)]
    rng = np.random.default_rng(11)
    dirs = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0]])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    M = L[rng.integers(0, 1000, 8)].astype(np.float64)
    edge = [m + float(t) * f * u for t in thr for f in (1.0 - 1e-6, 1.0, 1.0 + 1e-6) for u in dirs for m in M]
    mid = L[rng.integers(0, 1000, 100)] + np.float32(0.5) * np.eye(3, dtype=np.float32)[rng.integers(0, 3, 100)]
    far = off + np.array([[-50.0, 3.0, 3.0], [5.0, 5.0, 400.0], [9.0 + float(thr[0]), 4.0, 4.0], [4.0, -1e6, 4.0]], dtype=np.float32)
    S = np.concatenate([np.asarray(edge), mid, L[rng.integers(0, 1000, 60)], far]).astype(np.float32)
    return L, S, D, h, thr


@pytest.mark.parametrize("shift", [0.0, 3000.0], ids=["margin", "maxabs"])
def test_grown_levels_and_cell_edges_keep_the_brute_force_pairs(hiplib, shift):
    """Grid growth and the cell-edge margin of the refinement's levels, through ossid_ppf_refine_model_grid and
    ossid_ppf_refine_match at the C ABI: scene points at thr (1 - 1e-6, 1, 1 + 1e-6) from a model point along an axis, a
    face diagonal and the space diagonal, at midpoints (exact ties), on lattice points and far outside; shifted by 3000 the
    maxabs 2^-14 term dominates the cell edge. Every step's rows equal the brute force."""
    L, S, D, h, thr = _grown_grid_case(np.float32(shift))
    Mr = len(L)
    N = np.tile(np.array([[0.0, 0.0, 1.0]], dtype=np.float32), (Mr, 1))
    gb = int(_lib.fn("ossid_ppf_refine_grid_bytes")(Mr, 3, float(D), float(h)))
    assert gb > 0
    grid = torch.empty(gb, dtype=torch.uint8, device="cuda")
    pts, nrm = torch.from_numpy(L).cuda(), torch.from_numpy(N).cuda()
    assert _lib.fn("ossid_ppf_refine_model_grid")(pts.data_ptr(), nrm.data_ptr(), Mr, 3, float(D), float(h), grid.data_ptr(),
                                                  gb, None) == 0
    dev = types.SimpleNamespace(D=D, refine={"grid": grid, "Mr": Mr, "steps": 3, "h": h})
    model = types.SimpleNamespace(P=L)
    I = np.eye(4)
    d = (S[:, None, :] - L[None, :, :]).astype(np.float32)
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    n_ties = int(np.sum(np.sum(d2 == d2.min(axis=1, keepdims=True), axis=1) > 1))
    for step in range(3):
        want = _ref_match(I, S, model, thr[step])
        assert n_ties > 0 and np.any(want >= 0) and np.any(want < 0), step
        got = _match(dev, S, len(S), I[None], step, cap=2048)[0]
        assert np.array_equal(got, want), (step, np.flatnonzero(got != want)[:8])


def test_one_step_and_full_run_equal_the_restatement(obj, scenes):
    _P, _N, rm, dev = obj
    for depth, K, mask, T in scenes:
        s, S = _scene(dev, depth, mask, K)
        _r, cand = _candidates(dev, depth, mask, K)
        gaps = [ri.pose_gap(p, T) for p in cand]
        near = int(np.argmin([g[0] / float(rm.D) / 0.1 + g[1] / 12.0 for g in gaps]))
        for i in sorted({0, 1, near}):
            P1, _sc, pr1, st1, _ = _refine(dev, s, cand[i:i + 1], steps=1)
            T1, n1, d1 = rr.refine_one(cand[i], S, rm, steps=1)
            assert st1[0] == d1 == 1 and np.abs(P1[0] - T1).max() <= 1e-9
            assert pr1[0] == len(rr.correspondences(T1, S, rm.P, rr.thresholds(rm.D, rm.h, 1)[0])[0]) == n1
            P5, sc5, pr5, st5, status = _refine(dev, s, cand[i:i + 1])
            T5, n5, d5 = rr.refine_one(cand[i], S, rm)
            assert np.abs(P5[0] - T5).max() <= 1e-6 and pr5[0] == n5 and st5[0] == d5
            assert sc5[0] == n5 / float(len(rm.idx)) and list(status) == [0, len(S), 1, 0]
            R, R0 = P5[0][:3, :3], cand[i][:3, :3]          # the input is orthogonal to ~1e-7 (SPEC 6.5): the
            assert np.abs(R @ R.T - R0 @ R0.T).max() <= 1e-12     # update is rigid, R R^T stays as it was
            assert np.array_equal(P5[0][3], [0.0, 0.0, 0.0, 1.0])


def test_batch_rows_equal_single_calls_and_runs_are_bit_equal(obj, scenes):
    _P, _N, rm, dev = obj
    depth, K, mask, T = scenes[2]
    s, _S = _scene(dev, depth, mask, K)
    r, cand = _candidates(dev, depth, mask, K)
    singles = [_refine(dev, s, cand[i:i + 1]) for i in range(len(cand))]
    order = sorted(range(len(cand)), key=lambda i: (-int(singles[i][2][0]), i))
    a = [_np(t) for t in dev.find_hypotheses(depth, mask, K, DensePoseRefinement=True)]
    b = [_np(t) for t in dev.find_hypotheses(depth, mask, K, DensePoseRefinement="TRUE")]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    n = len(cand)
    assert np.array_equal(a[0][:n], np.array([singles[i][0][0] for i in order]))
    assert np.array_equal(a[1][:n], np.array([singles[i][1][0] for i in order]))
    assert np.all(np.diff(a[1][:n]) <= 0) and not a[0][n:].any() and not a[1][n:].any()
    assert np.array_equal(a[2], _np(r["info"])) and list(a[3]) == [0, len(_S), n, 0]
    batch = _refine(dev, s, cand, NR=100)
    assert np.array_equal(batch[0][:n], a[0][:n]) and np.array_equal(batch[3][:n], [singles[i][3][0] for i in order])
    dt, dr = rp.best_gap(a[0][:n], T, dev.D)
    assert dt <= 0.002 and dr <= 0.5, (dt, dr)
    top = ri.pose_gap(a[0][0], T)
    assert top[0] / float(dev.D) <= 0.002 and top[1] <= 0.5, top


def test_no_hypotheses_gives_an_empty_result(obj, scenes):
    _P, _N, _rm, dev = obj
    depth, K, mask, T = scenes[0]
    s, S = _scene(dev, depth, mask, K)
    P, sc, pr, st, status = _refine(dev, s, np.stack([T, T]), nh=0, NR=8)
    assert not P.any() and not sc.any() and not pr.any() and not st.any() and list(status) == [0, len(S), 0, 0]


def test_drop_in_in_millimetres_agrees_with_the_device_form(obj, scenes, tmp_path):
    P, N, _rm, dev = obj
    path = tmp_path / "obj_mm.ply"
    V = np.concatenate([P * 1000.0, N], 1).astype(np.float32)
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(V))
        f.write(b"".join(b"property float %s\n" % k for k in (b"x", b"y", b"z", b"nx", b"ny", b"nz")))
        f.write(b"end_header\n")
        f.write(V.tobytes())
    model = ppf.PPFModelDense(str(path))
    depth, K, mask, T = scenes[0]
    scene_pc = rp.depth2cloud(depth, mask, K).astype(np.float64)
    poses, scores, secs = model.find_surface_model(scene_pc * 1000.0)          # Halcon's default: refined
    assert poses.dtype == np.float64 and len(scores) == len(poses) > 0 and secs > 0 and np.all(np.diff(scores) <= 0)
    p0, s0, _ = model.find_surface_model(scene_pc * 1000.0, DensePoseRefinement="false")
    p1, s1, _ = ppf.PPFModel(str(path)).find_surface_model(scene_pc * 1000.0)
    assert np.array_equal(p0, p1) and np.array_equal(s0, s1)                   # 'false': unchanged PPF
    Tm = T.copy()
    Tm[:3, 3] *= 1000.0
    top = ri.pose_gap(poses[0], Tm)
    assert top[0] / float(model.D) <= 0.002 and top[1] <= 0.5, top
    dp, ds, _info, _st = [_np(t) for t in dev.find_hypotheses(depth, mask, K, DensePoseRefinement=True)]
    assert abs(ds[0] - scores[0]) <= 0.02
    Pm = poses[0].copy()
    Pm[:3, 3] /= 1000.0
    dt, dr = ri.pose_gap(Pm, dp[0])                                           # millimetres vs metres: same refined pose
    assert dt / float(dev.D) <= 0.001 and dr <= 0.3, (dt, dr)


def test_refinement_scene_over_its_cap_raises(obj):
    """A 0.9 m plane at 2 mm: ~4 800 PPF samples at SceneSamplingDist 0.1, ~120 000 refinement samples (cap 65 536)."""
    _P, _N, _rm, dev = obj
    g = np.arange(0.0, 0.9, 0.002, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    cloud = np.stack([X.ravel() - 0.45, Y.ravel() - 0.45, np.full(X.size, 0.8, np.float32)], 1)
    dev.find_surface_model(cloud, SceneSamplingDist=0.1)                       # the PPF scene itself is within its cap
    with pytest.raises(ValueError, match="DensePoseRefinement"):
        dev.find_surface_model(cloud, SceneSamplingDist=0.1, DensePoseRefinement=True)


def test_model_over_the_refinement_cap_holds_no_surface(hiplib):
    rng = np.random.default_rng(5)
    P = rng.uniform(0.0, 1.0, size=(60000, 3))
    N = rng.normal(size=(60000, 3))
    m = ppf.PPFModel(P, ModelSamplingDist=0.1, normals=N)
    assert m.refine is None and "16384" in m.refine_reason
    with pytest.raises(ValueError, match="DensePoseRefinement"):
        m.find_surface_model(P[:100], DensePoseRefinement="true")


def test_bad_arguments(obj, hiplib):
    _P, _N, _rm, dev = obj
    R = dev.refine
    t = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    p, gb = t.data_ptr(), int(R["grid"].numel())
    D, h, Mr = float(dev.D), float(R["h"]), R["Mr"]
    assert hiplib.fn("ossid_ppf_refine_grid_bytes")(0, 5, D, h) == 0
    assert hiplib.fn("ossid_ppf_refine_grid_bytes")(20000, 5, D, h) == 0
    assert hiplib.fn("ossid_ppf_refine_grid_bytes")(Mr, 0, D, h) == 0
    assert hiplib.fn("ossid_ppf_refine_workspace_bytes")(70000, 10) == 0
    assert hiplib.fn("ossid_ppf_refine_workspace_bytes")(1000, 0) == 0
    f = hiplib.fn("ossid_ppf_refine_model_grid")
    assert f(p, p, Mr, 5, D, h, p, 16, None) == -22
    assert f(None, p, Mr, 5, D, h, p, gb, None) == -22
    assert f(p, p, Mr, 5, -1.0, h, p, gb, None) == -22
    f = hiplib.fn("ossid_ppf_refine")
    ws = int(hiplib.fn("ossid_ppf_refine_workspace_bytes")(1024, 4))
    good = [p, p, 1024, R["grid"].data_ptr(), gb, Mr, p, p, 4, 5, D, h, p, ws, p, p, p, p, p, None]
    for i, bad in ((0, None), (2, 70000), (4, 16), (8, 0), (9, 17), (10, 0.0), (13, 8), (18, None)):
        args = list(good)
        args[i] = bad
        assert f(*args) == -22, i
    f = hiplib.fn("ossid_ppf_refine_match")
    good = [p, p, 1024, R["grid"].data_ptr(), gb, Mr, p, 4, 5, 0, D, h, p, ws, p, None]
    for i, bad in ((0, None), (9, 5), (9, -1), (13, 8), (14, None)):
        args = list(good)
        args[i] = bad
        assert f(*args) == -22, i


class _Args:
    dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0


def test_online_stream_with_refined_hypotheses(obj, scenes):
    from ossid_code_amd import dtoid, synth, zephyr
    from ossid_code_amd.stream import OnlineStream
    _P, _N, _rm, dev = obj
    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", _Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, _Args(), num_class=1), 0).to(0).eval()
    g = torch.Generator().manual_seed(1)
    limg = torch.rand(3, 3, 124, 124, generator=g)
    lmask = (torch.rand(3, 1, 124, 124, generator=g) > 0.5).float()
    depth, K, _mask, T = scenes[0]
    img, _bg = synth.make_frame(42)
    M = ri.model_points(T, 512)
    frame = {"img": img, "depth": depth, "cam_K": K, "limg": limg, "lmask": lmask, "obj_id": 1, "pose_gt": T,
             "model_points": M, "model_normals": M / np.linalg.norm(M, axis=1, keepdims=True),
             "model_colors": np.full_like(M, 0.5)}
    stream = OnlineStream(det, scorer, ds, confident_threshold=-1e30, ppf_models={1: dev},
                          ppf_kwargs={"DensePoseRefinement": True})
    results, _ = stream.run([frame], finetune_interval=100)
    r = results[0]
    assert "pose_hypos" not in frame and stream.times["ppf"] > 0
    assert r["n_hypos"] == len(r["ppf_hypos"]) >= 1
    assert min(np.abs(h - r["pred_pose"]).max() for h in r["ppf_hypos"]) == 0.0
    plain = OnlineStream(det, scorer, ds, confident_threshold=-1e30, ppf_models={1: dev})
    r0 = plain.run([dict(frame)], finetune_interval=100)[0][0]
    assert len(r0["ppf_hypos"]) == len(r["ppf_hypos"]) and not np.array_equal(r0["ppf_hypos"], r["ppf_hypos"])
