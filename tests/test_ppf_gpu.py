"""PPF pose hypotheses on the device (csrc/ppf.hip, SPEC.md section 6) against the numpy restatement tests/ref_ppf.py, stage
by stage: sampled indices, D, the model table, scene normals, per-reference peaks, poses and scores."""
import numpy as np
import pytest
import torch

import ref_icp as ri
import ref_ppf as rp
from ossid_code_amd import _lib, ppf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def obj(hiplib):
    P, N = rp.object_model()
    return P, N, rp.Model(P, N, 0.03), ppf.PPFModel(P, normals=N)


@pytest.fixture(scope="module")
def scenes(hiplib):
    return [rp.scene(k) for k in range(len(rp.POSES))]


def _np(t):
    return t.cpu().numpy()


def _stages(dev_model, depth, mask, K, **kw):
    return dev_model._run({"depth": torch.from_numpy(depth).cuda(), "mask": torch.from_numpy(mask.astype(np.uint8)).cuda(),
                           "cam_K": K}, **kw)


def _check_against_ref(ref, dev_model, depth, mask, K):
    """Every stage of one device run equals the restatement fed the device's normals."""
    r = _stages(dev_model, depth, mask, K)
    C = rp.depth2cloud(depth, mask, K)
    idx = rp.sample(C, rp.scene_valid(C), rp.F32(rp.F32(0.05) * ref.D))
    n = int(_np(r["sample"]["count"])[0])
    pix = np.flatnonzero(mask & (depth > 0))
    assert n == len(idx) and np.array_equal(_np(r["sample"]["idx"])[:n], pix[idx])
    S = C[idx]
    assert np.array_equal(_np(r["sample"]["pts"])[:n], S)
    Sn, Sok = _np(r["normals"])[:n], _np(r["normals_ok"])[:n].astype(bool)
    step = r["ref_step"]
    cands = rp.vote(ref, S, Sn, Sok, step)
    peaks = _np(r["peaks"])[:len(cands)]
    assert np.array_equal(peaks, np.array([c[1:] for c in cands], dtype=np.int32))
    cp = _np(r["cand_poses"])
    for j, (rr, m_r, al, cnt) in enumerate(cands):
        if cnt > 0:
            assert np.array_equal(cp[j], rp.pose(ref, m_r, al, S[rr], Sn[rr]))
    poses, scores = rp.cluster(ref, cands, S, Sn)
    info = _np(r["info"])
    assert info[0] == len(poses) and info[1] == n
    assert np.array_equal(_np(r["poses"])[:info[0]], poses) and np.array_equal(_np(r["scores"])[:info[0]], scores)
    return r, (S, Sn, Sok)


def test_model_sampling_diameter_and_table(obj):
    P, N, ref, dev = obj
    assert dev.D == ref.D and dev.h == ref.h                       # D exact
    assert np.array_equal(_np(dev.idx), ref.idx)
    assert np.array_equal(_np(dev.points), ref.P) and np.array_equal(_np(dev.normals), ref.N)
    assert dev.chunks == 2                                         # 1343 sampled points: two vote chunks
    off = _np(dev.offsets).astype(np.int64)
    nch = dev.chunks
    assert len(off) == ref.nkeys * nch + 1 and off[-1] == len(ref.entries)
    ent = _np(dev.entries)[:off[-1]].astype(np.uint32)
    slot_key = np.repeat(np.arange(ref.nkeys * nch) // nch, np.diff(off))
    slot_chunk = np.repeat(np.arange(ref.nkeys * nch) % nch, np.diff(off))
    assert np.array_equal(slot_chunk, (ent >> 5) // 1024)         # each entry in its reference point's chunk
    o_dev = np.lexsort((ent, slot_key))
    o_ref = np.lexsort((ref.entries, ref.keys))
    assert np.array_equal(slot_key[o_dev], ref.keys[o_ref]) and np.array_equal(ent[o_dev], ref.entries[o_ref])


def test_sampling_on_voxel_faces_and_duplicates(hiplib):
    """Points exactly on voxel faces (lattice multiples of h from lo), duplicates, non-finite and z <= 0 points."""
    rng = np.random.default_rng(11)
    h = np.float32(0.25)
    lat = rng.integers(0, 6, size=(3000, 3)).astype(np.float32) * h + np.float32(1.0)
    lat[::7] = lat[3::7][: len(lat[::7])]                         # duplicates
    lat[5::97, 2] = np.nan
    lat[9::89, 2] = -1.0
    C = np.concatenate([lat, lat[:200]])
    valid = rp.scene_valid(C)
    lo, D = rp.bounds(C, valid)
    rel = np.float32(h / D)
    want = rp.sample(C, valid, rp.F32(rel * D))
    dev = torch.device("cuda", 0)
    s = ppf._sample(dev, float(rel), float(D), 8192, points=torch.from_numpy(C).cuda())
    n = int(_np(s["count"])[0])
    assert n == len(want) and np.array_equal(_np(s["idx"])[:n], want)
    assert _np(s["stats"])[6] == D


def test_every_stage_equals_the_restatement(obj, scenes):
    _P, _N, ref, dev = obj
    worst = 0.0
    for depth, K, mask, _T in scenes:
        r, (S, Sn, Sok) = _check_against_ref(ref, dev, depth, mask, K)
        Rn, Rok = rp.scene_normals(S, r["h"])
        assert np.array_equal(Rok, Sok)
        a, b = Rn[Sok].astype(np.float64), Sn[Sok].astype(np.float64)
        ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), rp._dot(a, b))   # arccos near 1 would read f32 norms
        worst = max(worst, float(ang.max()))
    assert worst <= 1e-6, worst                                    # normals: within 1e-6 rad of numpy's eigh


def test_two_chunks_at_a_smaller_model_sampling(obj, scenes):
    P, N, _ref, _dev = obj
    ref = rp.Model(P, N, 0.02)
    dev = ppf.PPFModel(P, ModelSamplingDist=0.02, normals=N)
    assert dev.Ms == len(ref.idx) > 2048 and dev.chunks >= 3
    depth, K, mask, _T = scenes[1]
    _check_against_ref(ref, dev, depth, mask, K)


def test_recovers_the_true_pose(obj, scenes):
    _P, _N, ref, dev = obj
    for depth, K, mask, T in scenes:
        poses, scores, info = dev.find_hypotheses(depth, mask, K)
        n = ppf.check_info(info, 0.05)[0]
        assert 0 < n <= 100
        dt, dr = rp.best_gap(_np(poses)[:n], T, dev.D)
        assert dt <= 0.025 and dr <= 5.0, (dt, dr)


def test_two_runs_are_bit_equal_and_both_forms_agree(obj, scenes):
    _P, _N, _ref, dev = obj
    depth, K, mask, _T = scenes[2]
    a = [_np(t) for t in dev.find_hypotheses(depth, mask, K)]
    b = [_np(t) for t in dev.find_hypotheses(depth, mask, K)]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    C = rp.depth2cloud(depth, mask, K)
    c = dev._run({"points": torch.from_numpy(C).cuda()})
    assert np.array_equal(_np(c["poses"]), a[0]) and np.array_equal(_np(c["scores"]), a[1])
    assert np.array_equal(_np(c["info"]), a[2])


def test_drop_in_in_millimetres(obj, scenes, tmp_path):
    P, N, _ref, _dev = obj
    path = tmp_path / "obj_mm.ply"
    V = np.concatenate([P * 1000.0, N], 1).astype(np.float32)
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(V))
        f.write(b"".join(b"property float %s\n" % k for k in (b"x", b"y", b"z", b"nx", b"ny", b"nz")))
        f.write(b"end_header\n")
        f.write(V.tobytes())
    model = ppf.PPFModel(str(path))
    depth, K, mask, T = scenes[0]
    scene_pc = rp.depth2cloud(depth, mask, K).astype(np.float64)
    poses, scores, secs = model.find_surface_model(scene_pc * 1000.0, DensePoseRefinement='false', SceneSamplingDist=0.03,
                                                   RefPtRate=0.2)
    assert poses.dtype == np.float64 and poses.shape[1:] == (4, 4) and len(scores) == len(poses) > 0 and secs > 0
    assert np.all(np.diff(scores) <= 0)
    Tm = T.copy()
    Tm[:3, 3] *= 1000.0
    dt, dr = rp.best_gap(poses, Tm, model.D)
    assert dt <= 0.025 and dr <= 5.0, (dt, dr)                     # translations in mm
    assert 100.0 < float(model.D) < 200.0


def test_caps_and_bad_arguments(obj, scenes, hiplib):
    P, N, _ref, dev = obj
    with pytest.raises(ValueError, match="ModelSamplingDist"):
        ppf.PPFModel(P, ModelSamplingDist=0.005, normals=N)
    depth, K, _mask, _T = scenes[0]
    full = np.ones_like(depth, dtype=bool)
    with pytest.raises(ValueError, match="SceneSamplingDist"):
        dev.find_surface_model(rp.depth2cloud(depth, full, K), SceneSamplingDist=0.002)
    t = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    f = hiplib.fn("ossid_ppf_sample")
    assert f(None, None, 16, None, None, 0, 0, 1.0, 1.0, 0.0, 0.0, 0.05, 0.0, 16, p, 1 << 16, p, p, None, p, p, None) == -22
    assert f(p, None, 0, None, None, 0, 0, 1.0, 1.0, 0.0, 0.0, 0.05, 0.0, 16, p, 1 << 16, p, p, None, p, p, None) == -22
    assert f(p, None, 16, None, None, 0, 0, 1.0, 1.0, 0.0, 0.0, 0.05, 0.0, 16, p, 8, p, p, None, p, p, None) == -22
    assert hiplib.fn("ossid_ppf_model_table")(p, p, 5000, 0.01, 1.0, p, p, 1 << 30, p, 1 << 16, None) == -22
    assert hiplib.fn("ossid_ppf_scene_normals")(p, p, 9000, 0.01, p, p, None) == -22
    assert hiplib.fn("ossid_ppf_vote")(p, p, p, p, 8192, 5, p, p, 100, 0.01, 1.0, None, p, p, 1 << 16, p, p, None) == -22
    assert hiplib.fn("ossid_ppf_cluster")(p, p, p, 8192, 5, 100, 1.0, 0.1, 0, p, p, p, None) == -22


class _Args:
    dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0


def test_online_stream_with_ppf_hypotheses(obj, scenes):
    from ossid_code_amd import dtoid, synth, zephyr
    from ossid_code_amd.stream import OnlineStream
    P, N, _ref, dev = obj
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
    stream = OnlineStream(det, scorer, ds, confident_threshold=-1e30, ppf_models={1: dev})
    results, _ = stream.run([frame], finetune_interval=100)
    r = results[0]
    assert "pose_hypos" not in frame and stream.times["ppf"] > 0
    assert r["n_hypos"] == len(r["ppf_hypos"]) >= 1
    assert min(np.abs(h - r["pred_pose"]).max() for h in r["ppf_hypos"]) == 0.0
