"""batch producer, bbox/heat map, visibility mask + IoU, splat renderer, BOP csv.
CPU tests pin the numpy oracle (against the reference's own heatmapGaussain via the golden file) and the host-side csv
writer; GPU tests compare the kernels with the oracle."""
import csv
import os

import numpy as np
import pytest
import torch

import pipeline_cases as pc
import ref_pipeline as rpl
from oracle import pipeline_oracle as po
from ossid_code_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "dtoid_head.npz"))


def test_oracle_heatmap_matches_reference_golden():
    got = po.heatmap_gaussian(29, 39, 12.3, 7.9, np.sqrt(1.5))
    assert got.shape == (29, 39) and np.array_equal(got, G["gauss"])


def test_bop_csv_format(tmp_path):
    from ossid_code_amd.pipeline import save_results_bop
    pose = np.eye(4)
    pose[:3, 3] = [0.1, -0.2, 0.8]
    path = save_results_bop([{"scene_id": 2, "im_id": 5, "obj_id": 9, "pose": pose, "score": 21.5, "time": 0.3}],
                            str(tmp_path), "my_exp", "lmo")
    assert os.path.basename(path) == "my-exp_lmo-test.csv"
    rows = list(csv.DictReader(open(path)))
    assert list(rows[0].keys()) == ["scene_id", "im_id", "obj_id", "score", "R", "t", "time"]
    assert rows[0]["t"] == "100.0 -200.0 800.0" and rows[0]["R"].split(" ")[0] == "1.0" and rows[0]["score"] == "21.5"
    assert pose[2, 3] == 0.8                                  # caller's pose untouched


def _frame(seed=0):
    d = synth.make_scoring_inputs(N=2, M=900, seed=seed)
    rng = np.random.default_rng(seed)
    mask = np.zeros((480, 640), np.uint8)
    mask[150:331, 200:401] = 255
    mask[rng.random(mask.shape) < 0.3] = 0
    return d, mask


@pytest.mark.gpu
@pytest.mark.parametrize("out_hw", [None, (240, 320), (224, 224), (496, 656)])
def test_batch_producer_matches_oracle(hiplib, out_hw):
    from ossid_code_amd.pipeline import make_dtoid_sample
    d, mask = _frame()
    H, W = (480, 640) if out_hw is None else out_hw
    s = make_dtoid_sample(d["img"], d["depth"], mask, d["cam_K"], out_hw=out_hw, heatmap_hw=(29, 39))
    im, m, xyz = po.process_data(d["img"], mask / 255.0, d["depth"], d["cam_K"], H, W)
    assert s["img"].shape == (3, H, W) and s["xyz"].shape == (3, H, W) and s["mask"].shape == (1, H, W)
    # same size: a copy; resized: the same float32 formula in the same order with no fused multiply-add on either side
    # (SPEC.md 14.1), so bit for bit as well
    assert np.array_equal(s["img"].cpu().numpy(), im) and np.array_equal(s["mask"].cpu().numpy(), m)
    assert np.array_equal(s["xyz"].cpu().numpy(), xyz)
    box = po.mask_bbox(m[0])
    assert s["bbox_gt"].cpu().numpy().astype(int).tolist() == [box.tolist()]
    scale = 29.0 / H
    want = po.heatmap_gaussian(29, 39, (box[0] + box[2]) / 2.0 * scale, (box[1] + box[3]) / 2.0 * scale, np.sqrt(1.5))
    assert s["heatmap"].dtype == torch.float64 and np.allclose(s["heatmap"].cpu().numpy()[0], want, rtol=1e-12, atol=1e-15)


@pytest.mark.gpu
def test_empty_mask_gives_padding_label(hiplib):
    from ossid_code_amd.pipeline import make_dtoid_sample
    d, mask = _frame()
    s = make_dtoid_sample(d["img"], d["depth"], np.zeros_like(mask), d["cam_K"])
    assert float(s["bbox_gt"][0, 4]) == -1 and float(s["heatmap"].abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0, 1, 2])
def test_splat_renderer_and_visibility(hiplib, radius):
    from ossid_code_amd.pipeline import render_depth_points, visibility_and_iou
    d, _ = _frame(3)
    pose = d["pose_hypos"][0]
    H, W = 120, 160
    K = d["cam_K"].copy()
    K[:2] *= 0.25
    got = render_depth_points(pose, d["model_points"], K, (H, W), radius=radius).cpu().numpy()
    want = po.render_depth_points(pose, d["model_points"], K, H, W, radius)
    assert np.array_equal(got, want) and (got > 0).sum() > 20
    rng = np.random.default_rng(0)
    d_obs = np.where(rng.random((H, W)) < 0.1, 0, want + rng.normal(0, 0.01, (H, W))).astype(np.float32)
    gt = want > 0
    gtv = gt & (rng.random((H, W)) < 0.8)
    pm, vm, iou, iou_v = visibility_and_iou(d_obs, got, gt, gtv)
    wpm, wvm, wiou, wiou_v = po.visib_and_iou(d_obs, want, gt, gtv, 15 / 1000.0)
    assert np.array_equal(pm.cpu().numpy(), wpm) and np.array_equal(vm.cpu().numpy(), wvm)
    assert iou == wiou == 1.0 and abs(iou_v - wiou_v) < 1e-12


def test_det_results_and_expand_box(tmp_path):
    from ossid_code_amd import pipeline
    pipeline.save_det_results({(2, 7): [(5, 10, 20, 30, 40, 0.5), (6, 1, 2, 3, 4, 1.0)], (2, 8): [(5, 1, 2, 3, 4)]},
                              str(tmp_path))
    assert (tmp_path / "s000002_i000007.txt").read_text() == "obj_000005 0.500000 10 20 30 40\nobj_000006 1.000000 1 2 3 4\n"
    assert (tmp_path / "s000002_i000008.txt").read_text() == "obj_000005 1 2 3 4\n"
    # utils/__init__.py:11-16 restated independently
    x1, y1, x2, y2 = pipeline.expand_box(600, 10, 640, 50, 480, 640, 1.2)
    assert (x1, y1, x2, y2) == (620 - 24, 30 - 24, 639, 30 + 24)
    assert pipeline.expand_box(0, 0, 10, 10, 480, 640, 2.0)[:2] == (0, 0)


def test_template_view_selection_rules():
    """Rounded-linspace thinning at test time and nearest-rotation candidates at train time
    (datasets/dtoid_bop_dataset.py:294-318), checked against scipy's Rotation for the quaternion part."""
    from scipy.spatial.transform import Rotation
    from ossid_code_amd import pipeline
    rng = np.random.default_rng(0)
    rots = Rotation.random(40, random_state=1)
    bank = pipeline.TemplateBank.__new__(pipeline.TemplateBank)
    bank.n_local_test, bank.sample_from = 10, 5
    bank.img, bank.mask, bank.quats = {3: np.zeros((40, 1))}, {}, {3: rots.as_quat()}
    assert list(bank.test_views(3)) == list(np.linspace(0, 39, 10).round().astype(int))
    for _ in range(10):
        gt = Rotation.random(random_state=int(rng.integers(1 << 30)))
        q = gt.as_quat()
        want = np.argsort(2 * np.arccos(np.minimum(np.abs(rots.as_quat() @ q), 1 - 1e-7)), kind="stable")
        got = bank.nearest_views(3, gt.as_matrix())
        assert list(got[:5]) == list(want[:5])
        assert bank.train_view(3, gt.as_matrix(), rng) in want[:5]
        qq = pipeline._rotmat_to_quat(gt.as_matrix())
        assert min(np.abs(qq - q).max(), np.abs(qq + q).max()) < 1e-12


@pytest.mark.gpu
def test_pseudo_label_set_rows_are_d14_batches():
    import torch
    from ossid_code_amd import pipeline, synth
    d = synth.make_scoring_inputs(N=4, M=256, seed=3)
    g = torch.Generator().manual_seed(0)
    bank = pipeline.TemplateBank(n_local_test=4, sample_from=3)
    bank.add(1, (torch.rand(9, 124, 124, 3, generator=g) * 255).to(torch.uint8), torch.rand(9, 124, 124, generator=g) > 0.5,
             grid_quats=np.random.default_rng(0).normal(size=(9, 4)))
    mask = np.zeros((480, 640), np.float32)
    mask[100:200, 300:420] = 1
    for mode in ("train", "test"):
        ps = pipeline.PseudoLabelSet(bank, mode=mode)
        ps.add(1, 2, 3, d["img"], d["depth"], d["cam_K"], mask, 25.0, rot=np.eye(3))
        ps.add(1, 2, 4, d["img"], d["depth"], d["cam_K"], mask, 21.0)
        assert len(ps) == 2
        row = ps[0]
        ref = pipeline.make_dtoid_sample(d["img"], d["depth"], mask, d["cam_K"])
        for k in ("img", "xyz", "mask", "bbox_gt", "heatmap"):
            assert torch.equal(row[k], ref[k]), k
        assert row["bbox_gt"].tolist() == [[300.0, 100.0, 419.0, 199.0, 1.0]]
        assert row["gimg"].shape == (3, 124, 124) and row["gmask"].shape == (1, 124, 124)
        assert float(row["gimg"].max()) <= 1.0
        if mode == "train":
            assert row["limg"].shape == (3, 124, 124)
            batch = pipeline.collate([ps[0], ps[1]])
            assert batch["img"].shape == (2, 3, 480, 640) and batch["limg"].shape == (2, 3, 124, 124)
        else:
            assert row["limg"].shape == (4, 3, 124, 124) and row["lmask"].shape == (4, 1, 124, 124)
        m2 = np.zeros((480, 640), np.float32)
        m2[10:20, 30:50] = 1
        ps.updateZephyrMask(1, 2, 3, m2, 30.0)
        assert ps[0]["bbox_gt"].tolist() == [[30.0, 10.0, 49.0, 19.0, 1.0]] and ps[0]["zephyr_score"] == 30.0


# ---- the float32 oracle against the float64 restatement (tests/ref_pipeline.py) on the edge inputs ------------------------
RESIZE_SOURCES = [(480, 640), (37, 53), (1, 9), (9, 1)]
RESIZE_TARGETS = [(240, 320), (224, 224), (496, 656), (960, 1280), (480, 257), (37, 53), (481, 640), (1, 1), (3, 255), (5, 513)]


@pytest.mark.parametrize("src", RESIZE_SOURCES)
def test_oracle_resize_matches_float64(src):
    """po.resize_bilinear (float32, the order the kernel uses) against float64. The bound is derived, not tuned:
    |err| <= range * 4 * ulp32(max(Ho, Wo)) + 8 * 2^-24 * max|a|. The float32 source coordinate s carries up to a few
    ulp32(s) <= ulp32(max(Ho, Wo)) of error (the ratio's rounding times d + 1/2, the product's, the subtraction's), which
    moves a weight by as much and the result by that times the range of the four taps, once per axis; the four weight
    products, four tap products and three sums add at most 8 roundings of a value <= max|a|. At the dyadic ratios 1/2
    and 2 every float32 step is exact: equality, and the rounded image too (ties round half up)."""
    rng = np.random.default_rng(src[0] * 7 + src[1])
    a = rng.integers(0, 256, size=src + (3,), dtype=np.uint8)
    a[0, 0] = 0
    a[-1, -1] = 255
    for H, W in RESIZE_TARGETS:
        got, want = po.resize_bilinear(a, H, W), rpl.resize_bilinear(a, H, W)
        assert got.dtype == np.float32 and got.shape == want.shape == (H, W, 3)
        err = np.abs(got.astype(np.float64) - want).max()
        bound = 255.0 * 4 * float(np.spacing(np.float32(max(src)))) + 8 * 2.0 ** -24 * 255.0
        assert err <= bound, (src, (H, W), err, bound)
        if (H, W) == src or (src == (480, 640) and (H, W) in ((240, 320), (960, 1280))):
            assert np.array_equal(got, want), (src, (H, W))
            rounded = np.floor(got + np.float32(0.5))
            assert np.array_equal(rounded, rpl.round_half_up(want))
            if (H, W) == (240, 320):                           # a 2x2 mean: ties (x.5) exist and go up
                ties = want - np.floor(want) == 0.5
                assert ties.any() and np.array_equal(rounded[ties], want[ties] + 0.5)


def _resize_bound(a, src):
    """the bound of test_oracle_resize_matches_float64 for an array `a` resized from a source of size `src`"""
    a = np.asarray(a, np.float64)
    return (a.max() - a.min()) * 4 * float(np.spacing(np.float32(max(src)))) + 8 * 2.0 ** -24 * np.abs(a).max()


def test_oracle_process_data_matches_float64():
    """The whole producer on the GPU tests' size pairs: mask and xyz within the resize bound (xyz plus the three float32
    roundings of depth2xyz); the image differs from float64 by one grey level at the most, and only where the float64
    value lies within the resize bound of x.5, where the two roundings may fall on either side."""
    for (h, w), (H, W) in pc.PREP_PAIRS:
        if (h, w) == (480, 640):
            continue                                           # the resize itself is covered above at this size
        img, depth, mask, K = pc.prep_frame(h, w)
        im, m, xyz = po.process_data(img, mask, depth, K, H, W)
        wim, wm, wxyz = rpl.process_data(img, mask, depth, K, H, W)
        assert im.shape == (3, H, W) and m.shape == (1, H, W) and xyz.shape == (3, H, W)
        assert im.dtype == m.dtype == xyz.dtype == np.float32
        src_xyz = rpl.depth2xyz(depth, K)
        assert np.abs(m - wm).max() <= _resize_bound(mask, (h, w))
        assert np.abs(xyz - wxyz).max() <= _resize_bound(src_xyz, (h, w)) + 4 * 2.0 ** -24 * np.abs(src_xyz).max()
        levels = np.abs(im.astype(np.float64) * 255 - wim * 255)
        assert levels.max() <= 1 + 1e-4
        if (H, W) != (h, w):
            raw = np.moveaxis(rpl.resize_bilinear(img, H, W), 2, 0)
            flipped = levels > 0.5
            assert (np.abs(raw - np.floor(raw) - 0.5)[flipped] <= _resize_bound(img, (h, w))).all()
        else:
            assert levels.max() < 1e-4 and np.array_equal(m[0], mask)


def test_oracle_box_and_heatmap_match_float64():
    for name, mask in pc.bbox_masks().items():
        assert tuple(int(v) for v in po.mask_bbox(mask)) == rpl.mask_bbox(mask), name
    assert rpl.mask_bbox(pc.bbox_masks()["all_zero"]) == (1 << 30, 1 << 30, -1, -1, -1)
    assert rpl.mask_bbox(pc.bbox_masks()["signed_and_tiny_values"]) == (1, 2, 3, 4, 1)
    assert rpl.mask_bbox(pc.bbox_masks()["sixteenth_wave"]) == (0, 1, 51, 39, 1)
    for mask, hh, hw, scale in pc.heat_cases():
        box = rpl.mask_bbox(mask)
        want = rpl.heatmap(box, hh, hw, scale, np.sqrt(1.5))
        got = po.heatmap_gaussian(hh, hw, (box[0] + box[2]) / 2.0 * scale, (box[1] + box[3]) / 2.0 * scale, np.sqrt(1.5))
        assert got.shape == (hh, hw) and np.allclose(got, want, rtol=1e-12, atol=1e-15)
    assert not rpl.heatmap(rpl.EMPTY_BOX, 5, 7, 1.0, 1.0).any()


@pytest.mark.parametrize("radius", [0, 1, 8])
def test_oracle_splat_matches_float64(radius):
    pts = pc.splat_points()
    got = po.render_depth_points(pc.EYE, pts, pc.K_EDGE, pc.EH, pc.EW, radius)
    assert got.dtype == np.float32 and np.array_equal(got, rpl.splat(pc.EYE, pts, pc.K_EDGE, pc.EH, pc.EW, radius))
    if radius == 0:
        _check_splat_r0(got)
    rnd = pc.splat_random()
    got = po.render_depth_points(pc.EYE, rnd, pc.K_EDGE, 11, 23, radius)
    assert np.array_equal(got, rpl.splat(pc.EYE, rnd, pc.K_EDGE, 11, 23, radius)) and (got > 0).sum() > 20


def _check_splat_r0(img):
    """what the edge points of pc.splat_points() must give at radius 0, stated by hand (floor, not truncation)"""
    img = np.asarray(img)
    want = np.zeros((pc.EH, pc.EW))
    want[11, 0] = want[12, 39] = want[13, 39] = 100.0          # u_f = 0.0 -> column 0; 39.0 and 39.5 -> 39; -0.5 and 40.0 off
    want[0, 21] = want[23, 22] = want[23, 23] = 200.0          # v_f = 0.0 -> row 0; 23.0 and 23.5 -> 23; -0.5 and 24.0 off
    want[23, 39] = 400.0                                       # (39.5, 23.5): the last pixel
    want[5, 10] = want[3, 30] = 50.0                           # the nearer of two points wins, in either order
    want[0, 0] = pc.Z_NEXT32                                   # z' = 1e-6 dropped, the next float kept
    assert np.array_equal(img, want)                           # nothing else: negative, NaN, inf, |u_f| >= 1e9, off-image


def test_splat_floor_convention_single_points():
    """u_f = -0.5 floors to -1: off the image at radius 0, column 0 written at radius 1 (SPEC.md 14.3)."""
    for fn in (po.render_depth_points, rpl.splat):
        p = np.array([pc.point(-0.5, 5.0, 100.0)], np.float32)
        assert not fn(pc.EYE, p, pc.K_EDGE, pc.EH, pc.EW, 0).any()
        img = fn(pc.EYE, p, pc.K_EDGE, pc.EH, pc.EW, 1)
        assert (img[4:7, 0] == 100.0).all() and (img > 0).sum() == 3
        p = np.array([pc.point(5.0, -0.5, 100.0)], np.float32)
        assert not fn(pc.EYE, p, pc.K_EDGE, pc.EH, pc.EW, 0).any()
        img = fn(pc.EYE, p, pc.K_EDGE, pc.EH, pc.EW, 1)
        assert (img[0, 4:7] == 100.0).all() and (img > 0).sum() == 3
        img = fn(pc.EYE, np.array([pc.point(pc.EW - 0.5, pc.EH - 0.5, 7.0)], np.float32), pc.K_EDGE, pc.EH, pc.EW, 8)
        assert (img[pc.EH - 9:, pc.EW - 9:] == 7.0).all() and (img > 0).sum() == 81
        assert not fn(pc.EYE, np.zeros((0, 3), np.float32), pc.K_EDGE, pc.EH, pc.EW, 1).any()


@pytest.mark.parametrize("hw", [(480, 640), (37, 53), (3, 5)])
def test_oracle_visibility_matches_float64(hw):
    d_obs, d_pred, gt, gtv = pc.visib_frame(*hw)
    for delta in (pc.DELTA, 15 / 1000.0):
        pm, vm, iou, iou_v = po.visib_and_iou(d_obs, d_pred, gt, gtv, delta)
        wpm, wvm, c = rpl.visibility(d_obs, d_pred, gt, gtv, np.float32(delta))
        assert np.array_equal(pm, wpm) and np.array_equal(vm, wvm)
        assert iou == rpl.ratio(c[0], c[1]) and iou_v == rpl.ratio(c[2], c[3])
        assert 0 < iou < 1 and 0 < iou_v < 1 and c[0] != c[1] and c[2] != c[3] and pm.sum() != vm.sum()
    on_edge = (d_pred > 0) & (d_obs > 0) & (d_pred - d_obs == np.float32(pc.DELTA))
    assert on_edge.any() or hw == (3, 5)                       # pixels exactly at delta exist: <= and < differ here


def test_oracle_visibility_edge_row():
    d_obs, d_pred, want_pm, want_vm = pc.visib_edge_row()
    for pm, vm in (po.visib_and_iou(d_obs, d_pred, want_pm, want_vm, pc.DELTA)[:2],
                   rpl.visibility(d_obs, d_pred, None, None, pc.DELTA)[:2]):
        assert np.array_equal(pm, want_pm) and np.array_equal(vm, want_vm)
    assert np.isnan(rpl.ratio(0, 0)) and rpl.visibility(d_obs, d_pred, None, None, pc.DELTA)[2] == (0, 5 - 1, 0, 2)


def _meta(K):
    return {"camera_fx": K[0, 0], "camera_fy": K[1, 1], "camera_cx": K[0, 2], "camera_cy": K[1, 2]}


def test_oracle_projection_edges_match_float64(ozr):
    """The truncating projection (SPEC.md 3.2) on points built to land on its edges: the C oracle, the float32 numpy
    restatement (tests/ref_featurize.py) and the float64 restatement agree on every pixel and count."""
    import ref_featurize as rf
    pts, depth = pc.proj_case()
    T = pc.EYE[None]
    uv = ozr.project_uv(T, pts, pc.K_EDGE)
    want, _ = rpl.project(T, pts, pc.K_EDGE)
    assert np.array_equal(uv, want) and np.array_equal(uv, rf.project(T, pts, pc.K_EDGE)[3])
    n = len(pc.PU_EDGES)
    assert uv[0, :n, 0].tolist() == [-1, 0, 0, 39, 40] and uv[0, n:2 * n, 1].tolist() == [-1, 0, 0, 23, 24]
    assert uv[0, -4:].tolist() == [[-1, -1], [0, 0], [-1, -1], [-1, -1]]      # z' = 1e-6, the next float, 0, negative
    nrm, col = pc.model_table_inputs(len(pts))
    rgbd = ozr.pack_rgbd(pc.rgb_frame(), depth)
    tab = ozr.prep_model(pts, nrm, col)
    cnt = ozr.inconst_count(rgbd, T.astype(np.float32), tab, pc.K_EDGE, margin=pc.MARGIN)
    want_cnt = rpl.inconst_count(depth, T, pts, pc.K_EDGE, pc.MARGIN)
    assert np.array_equal(cnt, want_cnt)
    # by hand: u_f = -0.5 (rows 11, 0 -> column 0 / row 0 hold 101), u_f = 0.0, v_f = -0.5 and 0.0, (39.99, -0.5),
    # (-0.5, -0.5), one float past the margin, and u_f = 39.99 on column 39
    assert cnt.tolist() == [9]
    T2, pts2, depth2 = pc.proj_case_near()
    uv2 = ozr.project_uv(T2[None], pts2, pc.K_EDGE)
    assert np.array_equal(uv2, rpl.project(T2[None], pts2, pc.K_EDGE)[0]) and np.array_equal(uv2, rf.project(T2[None], pts2, pc.K_EDGE)[3])
    assert uv2[0].tolist() == [[-1, -1], [0, 0], [25, 12], [-1, -1]]


def test_mask_fraction_cases_match_float64():
    pts, T, mask, frac = pc.mask_filter_case()
    assert np.array_equal(rpl.mask_fraction(mask, T, pts, pc.K_EDGE), frac)
    assert ((frac > 0.5) == [True, False, False, False, False]).all()


def test_oracle_add_adi_chunking_is_invisible():
    T, gt, P = pc.pose_case(3, 300)
    for sym in (False, True):
        a, b = rpl.add_adi(T, gt, P, sym, chunk=64), rpl.add_adi(T, gt, P, sym, chunk=1000)
        assert np.allclose(a, b, rtol=1e-14, atol=0) and a[0] == 0.0 and (a[1:] > 0).all()
    est = np.einsum("nij,mj->nmi", T[:, :3, :3], P) + T[:, None, :3, 3]
    ref = P @ gt[:3, :3].T + gt[:3, 3]
    want = np.linalg.norm(est[:, :, None, :] - ref[None, None, :, :], axis=-1).min(-1).mean(1)
    assert np.allclose(rpl.add_adi(T, gt, P, True), want, rtol=1e-12, atol=1e-15)


def test_wrappers_refuse_mismatched_shapes_before_any_launch():
    """Host side only: every refusal comes before the device is touched, so this runs without one."""
    from ossid_code_amd import pipeline, scoring
    img, depth, mask, K = pc.prep_frame(8, 12)
    eye, P = np.eye(4), np.zeros((5, 3))
    meta = _meta(K)
    bad = [
        ("depth_pred", lambda: pipeline.visibility_and_iou(depth, depth[:4])),
        ("depth_obs", lambda: pipeline.visibility_and_iou(depth.ravel(), depth.ravel())),
        ("gt_mask", lambda: pipeline.visibility_and_iou(depth, depth, gt_mask=mask[:, :5])),
        ("gt_mask_visib", lambda: pipeline.visibility_and_iou(depth, depth, gt_mask_visib=mask.T)),
        ("img", lambda: pipeline.make_dtoid_sample(img[:4], depth, mask, K)),
        ("img", lambda: pipeline.make_dtoid_sample(img[..., 0], depth, mask, K)),
        ("mask", lambda: pipeline.make_dtoid_sample(img, depth, mask[:, :6], K)),
        ("depth", lambda: pipeline.make_dtoid_sample(img, depth[None], mask, K)),
        ("cam_K", lambda: pipeline.make_dtoid_sample(img, depth, mask, np.eye(4))),
        ("out_hw", lambda: pipeline.make_dtoid_sample(img, depth, mask, K, out_hw=(0, 5))),
        ("heatmap_hw", lambda: pipeline.make_dtoid_sample(img, depth, mask, K, heatmap_hw=(29, 0))),
        ("model_points", lambda: pipeline.render_depth_points(eye, np.zeros((5, 4)), K, (8, 12))),
        ("model_points", lambda: pipeline.render_depth_points(eye, np.zeros(15), K, (8, 12))),
        ("pose", lambda: pipeline.render_depth_points(np.eye(3), P, K, (8, 12))),
        ("pose", lambda: pipeline.render_depth_points(np.tile(eye, (2, 1, 1)), P, K, (8, 12))),
        ("cam_K", lambda: pipeline.render_depth_points(eye, P, K[:2], (8, 12))),
        ("hw", lambda: pipeline.render_depth_points(eye, P, K, (8, -1))),
        ("radius", lambda: pipeline.render_depth_points(eye, P, K, (8, 12), radius=9)),
        ("radius", lambda: pipeline.render_depth_points(eye, P, K, (8, 12), radius=-1)),
        ("pose_hypos", lambda: scoring.pose_errors(np.zeros((3, 3, 4)), eye, P)),
        ("pose_hypos", lambda: scoring.pose_errors(np.zeros(16), eye, P)),
        ("pose_gt", lambda: scoring.pose_errors(eye[None], eye[None], P)),
        ("model_points", lambda: scoring.pose_errors(eye[None], eye, P.T)),
        ("model_points", lambda: scoring.pose_errors(eye[None], eye, P[:0])),
        ("model_points", lambda: scoring.pose_errors(eye[None], eye, np.zeros((6401, 3)), symmetric=True)),
        ("model_points", lambda: scoring.filterHypoByMask(P.T, meta, eye[None], mask)),
        ("pose_hypos", lambda: scoring.filterHypoByMask(P, meta, np.zeros((2, 4, 3)), mask)),
        ("mask", lambda: scoring.filterHypoByMask(P, meta, eye[None], mask[None])),
    ]
    for name, call in bad:
        with pytest.raises(ValueError, match=name):
            call()
    assert scoring.ADI_MAX_POINTS == 6400
