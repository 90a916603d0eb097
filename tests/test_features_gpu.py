"""Keypoint-feature pose hypotheses on the device (csrc/features.hip, SPEC.md section 11) against the numpy restatement
tests/ref_features.py, stage by stage: scale space, keypoints, orientation bins, descriptors, frames (by their bits),
matches, candidate poses, clusters. The matcher tests are also the exact-integer check of the i8 matrix-core lane map."""
import numpy as np
import pytest
import torch

import ref_features as rf
import ref_icp as ri
import ref_ppf as rp
from ossid_code_amd import _lib, features, render

pytestmark = pytest.mark.gpu

K_SMALL = np.array([[143.0, 0.0, 80.3], [0.0, 143.5, 59.6], [0.0, 0.0, 1.0]])


def _np(t):
    return t.cpu().numpy()


def _pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = ri.rot(axis, deg), t
    return T


def _noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _smooth(H, W, seed, n=30):
    """Blobs of many sizes: keypoints in every octave, also next to the borders."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.full((H, W, 3), 120.0)
    for _ in range(n):
        cy, cx, sg = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.2, 7.0)
        f += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))[..., None] * rng.uniform(-100, 100, 3)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _depth_plane(H, W, seed, holes=True):
    """A tilted plane with a step (a depth discontinuity) and zero-depth holes; the mask has holes of its own."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (0.6 + 0.001 * xx + 0.0005 * yy + 0.1 * (xx > 0.7 * W)).astype(np.float32)
    m = np.ones((H, W), dtype=bool)
    if holes:
        d[rng.random((H, W)) < 0.02] = 0.0
        m[H // 3:H // 3 + 6, W // 4:W // 4 + 9] = False
        m[rng.random((H, W)) < 0.02] = False
    return d, m


@pytest.fixture(scope="module")
def small(hiplib):
    """The level-3 textured mesh, its 12-view model at S = 128 on the device and in the restatement, and a 160 x 120 frame."""
    V, F, C = rf.textured_mesh(3)
    mesh = render.Mesh(V, F, colors=C)
    R = render.view_grid(level=0)
    model = features.FeatureModel.from_mesh(mesh, K_SMALL, rotations=R, view_size=128)
    imgs, deps = render.render_color(mesh, model.view_poses, None, (128, 128), intrinsics=model.view_cams)
    dm, Fm = rf.model_features(_np(imgs), _np(deps), model.view_cams, model.view_poses)
    Tg = _pose([0.3, 1.0, 0.2], 25.0, [0.01, -0.005, 0.3])
    img, dep = render.render_color(mesh, Tg, K_SMALL, (120, 160))
    return {"mesh": mesh, "model": model, "dm": dm, "Fm": Fm, "D": rf.mesh_diameter(V), "img": _np(img), "depth": _np(dep)}


def _pyramid_levels(pyr, H, W):
    """The device buffer -> list per octave of int32 [5,Ho,Wo]."""
    out, off = [], 0
    for h, w in rf.octave_sizes(H, W):
        out.append(pyr[off:off + 5 * h * w].reshape(5, h, w))
        off += 5 * h * w
    return out


def _check_frame(img, depth, mask, K, **kw):
    """One device featurize equals the restatement in every stage -> (device dict, restatement tuple)."""
    f = features.featurize(img, depth, mask, K, **kw)
    tr = {}
    kps, bins, desc, frames, ok = rf.featurize(img, depth, mask, K, trace=tr, **{k: v for k, v in kw.items() if k == "contrast"})
    H, W = depth.shape
    lv = _pyramid_levels(_np(f["pyramid"]), H, W)
    assert len(lv) == len(tr["pyramid"])
    for a, b in zip(lv, tr["pyramid"]):
        assert np.array_equal(a, b)
    n = int(_np(f["count"])[0])
    assert n == len(kps) and int(_np(f["count"])[1]) == 0
    assert np.array_equal(_np(f["keypoints"])[:n], kps)
    assert np.array_equal(_np(f["bins"])[:n], bins)
    assert np.array_equal(_np(f["ok"])[:n].astype(bool), ok)
    assert np.array_equal(_np(f["descriptors"])[:n].view(np.int8), desc)
    assert np.array_equal(_np(f["frames"])[:n].view(np.int64), frames.view(np.int64))
    return f, (kps, bins, desc, frames, ok)


# ---- 1: scale space ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(65, 97), (120, 160), (20, 33)])
def test_pyramid_matches_the_restatement(hiplib, hw):
    H, W = hw
    img = _noise(H, W, 1)
    f = features.featurize(img, np.ones((H, W), np.float32), np.ones((H, W), bool), K_SMALL)
    ref = rf.pyramid(img)
    assert len(ref) == (2 if hw == (20, 33) else 3)
    lv = _pyramid_levels(_np(f["pyramid"]), H, W)
    assert len(lv) == len(ref)
    for a, b in zip(lv, ref):
        assert np.array_equal(a, b)


def test_rendered_frame_matches_the_restatement_in_every_stage(small):
    d = small["depth"]
    _f, (kps, _b, _d, _F, ok) = _check_frame(small["img"], d, d > 0, K_SMALL)
    assert len(kps) > 0 and ok.any()


# ---- 2, 3: keypoints, orientation, descriptors, frames ----------------------------------------------------------------------
def test_keypoints_descriptors_and_frames_with_holes_and_every_drop_rule(hiplib):
    seen = {"window": 0, "later": 0, "ok": 0}
    for hw, seed in (((65, 97), 2), ((120, 160), 3)):
        img = _smooth(hw[0], hw[1], seed)
        depth, mask = _depth_plane(hw[0], hw[1], seed)
        _f, (kps, bins, desc, frames, ok) = _check_frame(img, depth, mask, K_SMALL)
        seen["window"] += int((bins < 0).sum())
        seen["later"] += int(((bins >= 0) & ~ok).sum())
        seen["ok"] += int(ok.sum())
    assert seen["window"] > 0 and seen["later"] > 0 and seen["ok"] > 0


def test_descriptor_and_frame_drop_rules_each_fire(hiplib):
    """On a frame whose depth is a clean plane only the image border can drop a keypoint; with a step and holes in the
    depth, and the same image, further keypoints lose their frame: both rules are exercised and both match."""
    img = _smooth(120, 160, 3)
    plane, full = _depth_plane(120, 160, 3, holes=False)
    plane = np.full_like(plane, 0.7)
    _f, (_k, bins_a, _d, _F, ok_a) = _check_frame(img, plane, full, K_SMALL)
    depth, _m = _depth_plane(120, 160, 3)
    _f, (_k, bins_b, _d, _F, ok_b) = _check_frame(img, depth, full, K_SMALL)
    assert ((bins_a >= 0) & ~ok_a).sum() > 0                 # descriptor samples beyond the border
    assert (ok_a & ~ok_b).sum() > 0                          # frames lost to the depth


def test_noise_image_over_the_cap_writes_nothing_past_it(hiplib):
    H, W = 240, 320
    img = torch.from_numpy(_noise(H, W, 4)).cuda()
    depth, mask = torch.ones(H, W, device="cuda"), torch.ones(H, W, dtype=torch.uint8, device="cuda")
    pb = int(_lib.fn("ossid_feat_pyramid_bytes")(H, W, 3))
    pyr = torch.empty(pb // 4, dtype=torch.int32, device="cuda")
    st = _lib.stream()
    assert _lib.fn("ossid_feat_pyramid")(img.data_ptr(), H, W, 3, pyr.data_ptr(), pb, st) == 0
    wb = int(_lib.fn("ossid_feat_detect_workspace_bytes")(H, W, 3))
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    kps = torch.full((24, 4), -7, dtype=torch.int32, device="cuda")
    count = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert _lib.fn("ossid_feat_detect")(pyr.data_ptr(), H, W, 3, depth.data_ptr(), mask.data_ptr(), 192, 16, ws.data_ptr(), wb,
                                        kps.data_ptr(), count.data_ptr(), st) == 0
    ref = rf.detect(rf.pyramid(_np(img)), _np(depth), _np(mask))
    assert len(ref) > 16
    assert _np(count).tolist() == [len(ref), 1]
    assert np.array_equal(_np(kps)[:16], ref[:16]) and (_np(kps)[16:] == -7).all()
    # nothing further is computed: the later stages treat the frame as empty
    bins = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    desc = torch.full((16, 128), 9, dtype=torch.uint8, device="cuda")
    frames = torch.full((16, 4, 4), 5.0, dtype=torch.float64, device="cuda")
    ok = torch.full((16,), 3, dtype=torch.uint8, device="cuda")
    assert _lib.fn("ossid_feat_describe")(pyr.data_ptr(), H, W, 3, depth.data_ptr(), 100.0, 100.0, 160.0, 120.0, kps.data_ptr(),
                                          count.data_ptr(), 16, bins.data_ptr(), desc.data_ptr(), frames.data_ptr(),
                                          ok.data_ptr(), st) == 0
    assert (_np(bins) == -7).all() and (_np(desc) == 9).all() and (_np(frames) == 5.0).all() and (_np(ok) == 3).all()
    with pytest.raises(ValueError, match="contrast"):
        features.check_count(features.featurize(img, depth, mask, K_SMALL, max_keypoints=16))


def test_flat_image_has_no_keypoints(hiplib):
    img = np.full((65, 97, 3), 77, dtype=np.uint8)
    f, (kps, *_rest) = _check_frame(img, np.ones((65, 97), np.float32), np.ones((65, 97), bool), K_SMALL)
    assert len(kps) == 0 and _np(f["count"]).tolist() == [0, 0]


def _rotated_pattern(deg, S=96):
    """Anisotropic blobs (each with a clear gradient direction) rotated by `deg` about the image centre."""
    a = np.deg2rad(deg)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    u = np.cos(a) * (xx - S / 2) + np.sin(a) * (yy - S / 2)
    v = -np.sin(a) * (xx - S / 2) + np.cos(a) * (yy - S / 2)
    f = np.full((S, S), 110.0)
    for cu, cv, su, sv, amp in ((-14, -10, 2.0, 3.5, 90), (12, -12, 3.0, 1.8, -70), (-8, 14, 2.5, 4.5, 80), (15, 11, 4.0, 2.4, 100),
                                (0, 0, 1.6, 2.6, -90)):
        f += amp * np.exp(-((u - cu) ** 2 / (2 * su * su) + (v - cv) ** 2 / (2 * sv * sv)))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)[..., None].repeat(3, 2)


def test_all_36_orientation_bins_occur_and_match(hiplib):
    depth, mask = np.full((96, 96), 0.8, np.float32), np.ones((96, 96), bool)
    K = np.array([[400.0, 0, 48.0], [0, 400.0, 48.0], [0, 0, 1.0]])
    seen = set()
    for deg in range(0, 360, 10):
        _f, (_k, bins, _d, _F, ok) = _check_frame(_rotated_pattern(deg), depth, mask, K)
        seen |= set(int(b) for b in bins[ok])
    assert seen == set(range(36))


# ---- 4: matcher -------------------------------------------------------------------------------------------------------------
def _match(A, ok, B, cap=None, stream=None):
    cap = len(A) if cap is None else cap
    ds = torch.zeros(cap, 128, dtype=torch.uint8, device="cuda")
    ds[:len(A)] = torch.from_numpy(A.view(np.uint8)).cuda()
    oks = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    oks[:len(A)] = torch.from_numpy(ok.astype(np.uint8)).cuda()
    cnt = torch.tensor([len(A), 0], dtype=torch.int32, device="cuda")
    dm = torch.from_numpy(B.view(np.uint8)).cuda()
    return _np(features.match_descriptors(ds, oks, cnt, dm))[:len(A)]


def _ref_match(A, ok, B):
    best, d2, w = rf.match(A, ok, B)
    return np.stack([best, d2, w], 1).astype(np.int32)


@pytest.mark.parametrize("Nm", [1, 31, 33, 1000, 5000])
def test_matcher_equals_integer_arithmetic(hiplib, Nm):
    rng = np.random.default_rng(Nm)
    B = rng.integers(0, 128, (Nm, 128)).astype(np.int8)
    for Ns in (1, 31, 32, 33, 100):
        A = rng.integers(0, 128, (Ns, 128)).astype(np.int8)
        take = rng.integers(0, Nm, Ns // 2)                     # half of the scene rows sit near a model row
        A[:len(take)] = np.clip(B[take].astype(int) + rng.integers(-3, 4, (len(take), 128)), 0, 127).astype(np.int8)
        ok = np.ones(Ns, dtype=bool)
        assert np.array_equal(_match(A, ok, B), _ref_match(A, ok, B))


def test_matcher_ties_go_to_the_lowest_index_and_dropped_rows_are_skipped(hiplib):
    rng = np.random.default_rng(9)
    B = rng.integers(0, 128, (3000, 128)).astype(np.int8)
    B[2500], B[77], B[2100] = B[40], B[40], B[40]              # duplicates across staged tiles and workgroup chunks
    B[2999] = B[2998]
    A = np.stack([B[40], B[2998], B[5], rng.integers(0, 128, 128).astype(np.int8)])
    ok = np.array([True, True, False, True])
    got = _match(A, ok, B, cap=40)
    assert np.array_equal(got, _ref_match(A, ok, B))
    assert got[0].tolist() == [40, 0, 1024] and got[1].tolist() == [2998, 0, 1024] and got[2].tolist() == [-1, 0, 0]


def test_matcher_is_bit_reproducible_across_runs_and_streams(hiplib):
    rng = np.random.default_rng(10)
    A = rng.integers(0, 128, (100, 128)).astype(np.int8)
    B = rng.integers(0, 128, (5000, 128)).astype(np.int8)
    ok = rng.random(100) < 0.8
    a = _match(A, ok, B)
    b = _match(A, ok, B)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = _match(A, ok, B)
    side.synchronize()
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, _ref_match(A, ok, B))


def test_matcher_without_model_features_matches_nothing(hiplib):
    A = np.random.default_rng(1).integers(0, 128, (5, 128)).astype(np.int8)
    got = _match(A, np.ones(5, bool), np.zeros((0, 128), np.int8))
    assert (got == np.array([-1, 0, 0])).all()


# ---- 5, 6: hypotheses, clustering, end to end -------------------------------------------------------------------------------
def test_small_end_to_end_equals_the_restatement(small):
    model, d = small["model"], small["depth"]
    assert np.array_equal(_np(model.descriptors).view(np.int8), small["dm"])
    assert np.array_equal(_np(model.frames).view(np.int64), small["Fm"].view(np.int64))
    assert model.D == small["D"] and len(model) > 0
    tr = {}
    poses, scores = rf.find_hypotheses(small["img"], d, d > 0, K_SMALL, small["dm"], small["Fm"], small["D"], trace=tr)
    f = features.featurize(small["img"], d, d > 0, K_SMALL)
    r = model._hypotheses(f["descriptors"], f["frames"], f["ok"], f["count"])
    n = len(tr["keypoints"])
    assert np.array_equal(_np(r["match"])[:n], np.stack([tr["best"], tr["d2"], tr["w"]], 1))
    assert (tr["w"] > 0).sum() > 0
    assert np.array_equal(_np(r["cand_poses"])[:n].view(np.int64), tr["cand"].view(np.int64))
    info = _np(r["info"])
    assert info[0] == len(poses) > 0 and info[1] == n
    assert np.array_equal(_np(r["poses"])[:info[0]], poses) and np.array_equal(_np(r["scores"])[:info[0]], scores)
    assert (_np(r["poses"])[info[0]:] == 0).all()
    p2, s2, i2 = model.find_hypotheses(d, small["img"], d > 0, K_SMALL)
    assert np.array_equal(_np(p2), _np(r["poses"])) and np.array_equal(_np(s2), _np(r["scores"])) and np.array_equal(_np(i2), info)


def test_drop_ins_agree_with_the_device_form_and_ignore_mat_gt(small, tmp_path):
    model, d = small["model"], small["depth"].astype(np.float64)
    fx, fy, cx, cy = K_SMALL[0, 0], K_SMALL[1, 1], K_SMALL[0, 2], K_SMALL[1, 2]
    yy, xx = np.mgrid[0:120, 0:160]
    dist = d * np.sqrt(((xx - cx) / fx) ** 2 + ((yy - cy) / fy) ** 2 + 1.0)
    meta = {"camera_fx": fx, "camera_fy": fy, "camera_cx": cx, "camera_cy": cy, "camera_scale": 1.0}
    kp, feats, cloud, frames = features.featurizeScene(small["img"], dist, d > 0, meta, [11], [11])
    assert len(kp) == len(feats) == len(cloud) == len(frames) > 0 and np.array_equal(cloud, frames[:, :3, 3])
    poses, aux = model.match(feats, frames)
    poses_gt, _aux = model.match(feats, frames, np.eye(4))
    assert len(poses) > 0 and np.array_equal(poses, poses_gt)
    model.save(str(tmp_path / "m.npz"))
    again = features.FeatureModel.load(str(tmp_path / "m.npz"))
    assert np.array_equal(again.match(feats, frames)[0], poses)
    with pytest.raises(ValueError):
        features.featurizeScene(small["img"], dist, np.zeros((120, 160), bool), meta, [11], [11])


# ---- 7: full size -----------------------------------------------------------------------------------------------------------
def test_full_size_top_five_hold_a_useful_hypothesis(hiplib):
    """The level-5 mesh, 42 views at S = 256, three 640 x 480 frames at poses that are no grid view (in-plane rotation
    included): at least one of the top 5 lies within 0.1 D and 12 degrees of the truth (SPEC 6.6's basin)."""
    from ossid_code_amd import synth
    V, F, C = rf.textured_mesh(5)
    mesh = render.Mesh(V, F, colors=C)
    model = features.FeatureModel.from_mesh(mesh, synth.CAM_K, level=1, view_size=256)
    D = rf.mesh_diameter(V)
    assert model.D == D and len(model) > 100
    for k in range(len(rp.POSES)):
        Tg = rp.gt_pose(k)
        img, dep = render.render_color(mesh, Tg, synth.CAM_K, (480, 640))
        poses, scores, info = model.find_hypotheses(dep, img, dep > 0, synth.CAM_K)
        n = int(_np(info)[0])
        top = _np(poses)[:min(n, 5)]
        gaps = [ri.pose_gap(T, Tg) for T in top]
        print("pose %d: %d keypoints, %d hypotheses, top-5 gaps (t / D, deg): %s" % (
            k, int(_np(info)[1]), n, ", ".join("%.3f / %.1f" % (a / float(D), b) for a, b in gaps)))
        assert any(rf.useful(T, Tg, D) for T in top)


# ---- 8: the stream ----------------------------------------------------------------------------------------------------------
class _Args:
    dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0


class _Boxed:
    """The detector with its final box replaced by a given one: the chain stays the real one, the mask holds the object
    (an untrained DtoidNet boxes anything)."""

    def __init__(self, det, box):
        self.det, self.box = det, torch.tensor([box], dtype=torch.float32)

    def parameters(self):
        return self.det.parameters()

    def forwardTestTime(self, batch):
        out = dict(self.det.forwardTestTime(batch))
        out["final_bbox"], out["final_score"] = [self.box], [torch.ones(1)]
        return out


def test_online_stream_puts_feature_hypotheses_in_front_of_the_ppf_ones(small):
    from ossid_code_amd import dtoid, ppf, synth, zephyr
    from ossid_code_amd.stream import OnlineStream
    P, N = rp.object_model()
    ppf_model = ppf.PPFModel(P, normals=N)
    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", _Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, _Args(), num_class=1), 0).to(0).eval()
    g = torch.Generator().manual_seed(1)
    limg = torch.rand(3, 3, 124, 124, generator=g)
    lmask = (torch.rand(3, 1, 124, 124, generator=g) > 0.5).float()
    depth, K, _mask, T = rp.scene(0)
    img, _bg = synth.make_frame(42)
    color, dep = render.render_color(small["mesh"], T, K, (480, 640))
    img = np.where((_np(dep) > 0)[..., None], _np(color), img)          # the textured object in front of the background
    ys, xs = np.nonzero(_np(dep) > 0)
    det = _Boxed(det, [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1])
    M = ri.model_points(T, 512)
    frame = {"img": img, "depth": depth, "cam_K": K, "limg": limg, "lmask": lmask, "obj_id": 1, "pose_gt": T,
             "model_points": M, "model_normals": M / np.linalg.norm(M, axis=1, keepdims=True),
             "model_colors": np.full_like(M, 0.5)}
    fm = small["model"]
    plain = OnlineStream(det, scorer, ds, confident_threshold=-1e30, ppf_models={1: ppf_model})
    both = OnlineStream(det, scorer, ds, confident_threshold=-1e30, ppf_models={1: ppf_model}, feature_models={1: fm})
    only = OnlineStream(det, scorer, ds, confident_threshold=-1e30, feature_models={1: fm})
    rp_, rb, ro = (s.run([frame], finetune_interval=100)[0][0] for s in (plain, both, only))
    assert "sift" not in plain.times and "n_feature_hypos" not in rp_
    assert both.times["sift"] > 0 and both.times["ppf"] > 0 and "pose_hypos" not in frame
    nf = rb["n_feature_hypos"]
    print("feature hypotheses: %d, PPF hypotheses: %d" % (nf, len(rp_["ppf_hypos"])))
    assert nf >= 1
    assert rb["n_hypos"] == nf + len(rp_["ppf_hypos"]) == len(rb["ppf_hypos"])
    assert np.array_equal(rb["ppf_hypos"][nf:], rp_["ppf_hypos"])
    depth_m, mask = both._detection_mask(frame, det.forwardTestTime({
        "img": torch.from_numpy(np.ascontiguousarray(img)).cuda().permute(2, 0, 1).float().div_(255.0)[None],
        "obj_id": torch.tensor([1]), "limg": limg[None].cuda(), "lmask": lmask[None].cuda()}))
    poses, _s, info = fm.find_hypotheses(depth_m, img, mask, K)
    assert int(info[0]) == nf and np.array_equal(rb["ppf_hypos"][:nf], _np(poses)[:nf])
    assert ro["n_feature_hypos"] == nf and ro["n_hypos"] == nf and "ppf_hypos" not in ro


def test_stream_with_feature_models_only_falls_back_to_one_identity_pose(small):
    from ossid_code_amd import dtoid, synth, zephyr
    from ossid_code_amd.stream import OnlineStream
    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", _Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, _Args(), num_class=1), 0).to(0).eval()
    g = torch.Generator().manual_seed(1)
    limg = torch.rand(3, 3, 124, 124, generator=g)
    lmask = (torch.rand(3, 1, 124, 124, generator=g) > 0.5).float()
    depth, K, _mask, T = rp.scene(0)
    M = ri.model_points(T, 512)
    frame = {"img": np.full((480, 640, 3), 90, dtype=np.uint8), "depth": depth, "cam_K": K, "limg": limg, "lmask": lmask,
             "obj_id": 1, "pose_gt": T, "model_points": M, "model_normals": M / np.linalg.norm(M, axis=1, keepdims=True),
             "model_colors": np.full_like(M, 0.5)}
    only = OnlineStream(det, scorer, ds, confident_threshold=-1e30, feature_models={1: small["model"]})
    r = only.run([frame], finetune_interval=100)[0][0]
    assert r["n_feature_hypos"] == 0 and r["n_hypos"] == 1 and np.array_equal(r["pred_pose"], np.eye(4))
