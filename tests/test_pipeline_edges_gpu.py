"""GPU tests (pytest -m gpu) of the frame-side kernels at their edges (SPEC.md section 14): the sample producer, the box
and heat map, the point splat, the visibility mask with its IoUs (csrc/pipeline.hip), ADD / ADI and the truncating
projection behind projectPointsUv / inconst_count / featurize / filterHypoByMask (csrc/zephyr.hip). Each kernel goes
against the float32 oracle bit for bit and against the float64 restatement (tests/ref_pipeline.py) on inputs built so
that both must agree exactly (tests/pipeline_cases.py); tests/test_pipeline.py pins oracle and restatement to each other
without a GPU. No case here makes a kernel read or write out of bounds: every refused call is refused before a launch."""
import numpy as np
import pytest
import torch

import pipeline_cases as pc
import ref_featurize as rf
import ref_pipeline as rpl
from oracle import pipeline_oracle as po
from test_pipeline import _check_splat_r0, _meta

pytestmark = pytest.mark.gpu

EINVAL = -22
SIGMA = float(np.sqrt(1.5))


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


# ---- sample producer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", pc.PREP_PAIRS, ids=["%dx%d-%dx%d" % (s + d) for s, d in pc.PREP_PAIRS])
def test_sample_producer_equals_oracle_bit_for_bit(hiplib, src, dst):
    """Widths below, at and above one 256-thread row chunk, mixed up / down scaling, one axis unchanged, a one-pixel
    source axis, a one-pixel target. Neither side fuses a multiply-add: equality, not a tolerance."""
    from ossid_code_amd.pipeline import make_dtoid_sample
    img, depth, mask, K = pc.prep_frame(*src)
    H, W = dst
    hh, hw = (29, 39) if H >= 29 else (max(H // 2, 1), max(W // 2, 1))
    s = make_dtoid_sample(img, depth, mask, K, out_hw=None if dst == src else dst, heatmap_hw=(hh, hw))
    im, m, xyz = po.process_data(img, mask, depth, K, H, W)
    assert s["img"].shape == (3, H, W) and s["xyz"].shape == (3, H, W) and s["mask"].shape == (1, H, W)
    assert np.array_equal(s["img"].cpu().numpy(), im)
    assert np.array_equal(s["mask"].cpu().numpy(), m)
    assert np.array_equal(s["xyz"].cpu().numpy(), xyz)
    box = rpl.mask_bbox(m[0])                                  # from the ORACLE's resized mask
    assert s["bbox_gt"].cpu().numpy().astype(np.int64).tolist() == [list(box)]
    want = rpl.heatmap(box, hh, hw, float(hh) / float(H), SIGMA)
    assert s["heatmap"].dtype == torch.float64 and s["heatmap"].shape == (1, hh, hw)
    assert np.allclose(s["heatmap"].cpu().numpy()[0], want, rtol=1e-12, atol=1e-15)


# ---- box and heat map, through the C entry ---------------------------------------------------------------------------------
def _bbox_heat(hiplib, mask, hh=0, hw=0, scale=1.0, heat=True, sentinel=-777):
    m = _cuda(mask)
    box = torch.full((5,), sentinel, dtype=torch.int32, device="cuda")
    hm = torch.full((max(hh * hw, 1),), -5.0, dtype=torch.float64, device="cuda") if heat else None
    rc = hiplib.fn("ossid_mask_bbox_heatmap")(m.data_ptr(), mask.shape[0], mask.shape[1], hh, hw, float(scale), SIGMA,
                                              box.data_ptr(), None if hm is None else hm.data_ptr(), hiplib.stream())
    torch.cuda.synchronize()
    return rc, box.cpu().numpy().tolist(), None if hm is None else hm.cpu().numpy()


@pytest.mark.parametrize("name", sorted(pc.bbox_masks()))
def test_bbox_edges(hiplib, name):
    mask = pc.bbox_masks()[name]
    rc, box, hm = _bbox_heat(hiplib, mask, 3, 4, 0.5)
    assert rc == 0 and tuple(box) == rpl.mask_bbox(mask)
    assert np.allclose(hm.reshape(3, 4), rpl.heatmap(tuple(box), 3, 4, 0.5, SIGMA), rtol=1e-12, atol=1e-15)
    if name == "all_zero":
        assert box == [1 << 30, 1 << 30, -1, -1, -1] and not hm.any()


@pytest.mark.parametrize("case", range(len(pc.heat_cases())))
def test_heatmap_sizes(hiplib, case):
    mask, hh, hw, scale = pc.heat_cases()[case]
    rc, box, hm = _bbox_heat(hiplib, mask, hh, hw, scale)
    assert rc == 0 and tuple(box) == rpl.mask_bbox(mask)
    assert np.allclose(hm.reshape(hh, hw), rpl.heatmap(tuple(box), hh, hw, scale, SIGMA), rtol=1e-12, atol=1e-15)
    assert 0.0 <= hm.min() and hm.max() <= 1.0


def test_bbox_without_heatmap_and_refused_sizes(hiplib):
    mask = pc.bbox_masks()["fewer_pixels_than_threads"]
    rc, box, _ = _bbox_heat(hiplib, mask, 0, 0, heat=False)             # heatmap = NULL: the box only, sizes ignored
    assert rc == 0 and box == [2, 1, 5, 3, 1]
    for hh, hw in ((0, 4), (-1, 4), (3, 0)):                            # refused without launching: nothing is written
        rc, box, hm = _bbox_heat(hiplib, mask, hh, hw)
        assert rc == EINVAL and box == [-777] * 5 and (hm == -5.0).all()


# ---- splat -----------------------------------------------------------------------------------------------------------------
def _splat(pts, hw=(pc.EH, pc.EW), radius=0, pose=pc.EYE):
    from ossid_code_amd.pipeline import render_depth_points
    return render_depth_points(pose, pts, pc.K_EDGE, hw, radius=radius).cpu().numpy()


@pytest.mark.parametrize("radius", [0, 1, 8])
def test_splat_edges(hiplib, radius):
    pts = pc.splat_points()
    got = _splat(pts, radius=radius)
    assert got.dtype == np.float32
    assert np.array_equal(got, po.render_depth_points(pc.EYE, pts, pc.K_EDGE, pc.EH, pc.EW, radius))
    assert np.array_equal(got, rpl.splat(pc.EYE, pts, pc.K_EDGE, pc.EH, pc.EW, radius))
    if radius == 0:
        _check_splat_r0(got)
    rnd = pc.splat_random(257)                                 # two blocks of points; 11 x 23 = 253 pixels, not a multiple of 256
    got = _splat(rnd, (11, 23), radius)
    assert np.array_equal(got, po.render_depth_points(pc.EYE, rnd, pc.K_EDGE, 11, 23, radius))
    assert np.array_equal(got, rpl.splat(pc.EYE, rnd, pc.K_EDGE, 11, 23, radius))


def test_splat_floor_convention_and_limits(hiplib):
    """u_f = -0.5 floors to -1 (the projection truncates it to 0 instead: test_projection_edges)."""
    p = np.array([pc.point(-0.5, 5.0, 100.0)], np.float32)
    assert not _splat(p, radius=0).any()
    img = _splat(p, radius=1)
    assert (img[4:7, 0] == 100.0).all() and (img > 0).sum() == 3
    p = np.array([pc.point(5.0, -0.5, 100.0)], np.float32)
    assert not _splat(p, radius=0).any()
    img = _splat(p, radius=1)
    assert (img[0, 4:7] == 100.0).all() and (img > 0).sum() == 3
    img = _splat(np.array([pc.point(pc.EW - 0.5, pc.EH - 0.5, 7.0)], np.float32), radius=8)
    assert (img[pc.EH - 9:, pc.EW - 9:] == 7.0).all() and (img > 0).sum() == 81
    assert not _splat(np.zeros((0, 3), np.float32), radius=1).any()          # M = 0: an all-zero image
    # radius 9: refused by the entry point before a launch (the output keeps its sentinel), and by the wrapper
    T, P = _cuda(np.eye(4, dtype=np.float32)), _cuda(p)
    z = torch.zeros(pc.EH * pc.EW, dtype=torch.int32, device="cuda")
    out = torch.full((pc.EH, pc.EW), -5.0, dtype=torch.float32, device="cuda")
    rc = hiplib.fn("ossid_render_depth_points")(T.data_ptr(), P.data_ptr(), 1, 100.0, 100.0, 0.0, 0.0, pc.EH, pc.EW, 9,
                                                z.data_ptr(), out.data_ptr(), hiplib.stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and bool((out == -5.0).all())
    with pytest.raises(ValueError, match="radius"):
        _splat(p, radius=9)


# ---- visibility and IoU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(480, 640), (37, 53), (3, 5)])
def test_visibility_and_iou_sizes(hiplib, hw):
    """480 x 640 is more than the 1024 x 256 pixels one pass of the launch covers: the grid-strided second pass runs.
    The ground-truth masks are independent of the prediction, so no ratio is 1; many pixels lie exactly at delta."""
    from ossid_code_amd.pipeline import visibility_and_iou
    d_obs, d_pred, gt, gtv = pc.visib_frame(*hw)
    wpm, wvm, c = rpl.visibility(d_obs, d_pred, gt, gtv, pc.DELTA)
    opm, ovm, oiou, oiou_v = po.visib_and_iou(d_obs, d_pred, gt, gtv, pc.DELTA)
    dob, dpr = _cuda(d_obs), _cuda(d_pred)                    # the same device buffers for both calls
    first = visibility_and_iou(dob, dpr, gt, gtv, delta=pc.DELTA)
    again = visibility_and_iou(dob, dpr, gt, gtv, delta=pc.DELTA)
    for pm, vm, iou, iou_v in (first, again):                  # the counters are cleared on each call
        assert pm.dtype == torch.bool and pm.shape == hw
        assert np.array_equal(pm.cpu().numpy(), wpm) and np.array_equal(vm.cpu().numpy(), wvm)
        assert np.array_equal(pm.cpu().numpy(), opm) and np.array_equal(vm.cpu().numpy(), ovm)
        assert iou == c[0] / c[1] and iou_v == c[2] / c[3]
        assert iou == oiou and iou_v == oiou_v and 0 < iou < 1 and 0 < iou_v < 1
    # one mask without the other: nan for the missing ratio only
    _, _, iou, iou_v = visibility_and_iou(dob, dpr, gt_mask=gt, delta=pc.DELTA)
    assert iou == c[0] / c[1] and np.isnan(iou_v)
    _, _, iou, iou_v = visibility_and_iou(dob, dpr, gt_mask_visib=gtv, delta=pc.DELTA)
    assert np.isnan(iou) and iou_v == c[2] / c[3]
    pm, vm, iou, iou_v = visibility_and_iou(dob, dpr, delta=pc.DELTA)
    assert np.isnan(iou) and np.isnan(iou_v) and np.array_equal(vm.cpu().numpy(), wvm)
    # the default delta (15 mm as float32)
    pm, vm, iou, iou_v = visibility_and_iou(dob, dpr, gt, gtv)
    wpm, wvm, c = rpl.visibility(d_obs, d_pred, gt, gtv, np.float32(15 / 1000.0))
    assert np.array_equal(vm.cpu().numpy(), wvm) and iou == c[0] / c[1] and iou_v == c[2] / c[3]


def test_visibility_edge_row_and_empty_union(hiplib):
    from ossid_code_amd.pipeline import visibility_and_iou
    d_obs, d_pred, want_pm, want_vm = pc.visib_edge_row()
    pm, vm, iou, iou_v = visibility_and_iou(d_obs, d_pred, want_pm, want_vm, delta=pc.DELTA)
    assert np.array_equal(pm.cpu().numpy(), want_pm) and np.array_equal(vm.cpu().numpy(), want_vm)
    assert iou == 1.0 and iou_v == 1.0
    none = np.zeros((1, 7), bool)
    pm, vm, iou, iou_v = visibility_and_iou(d_obs, d_pred, none, none, delta=pc.DELTA)
    assert iou == 0.0 and iou_v == 0.0                         # empty intersection, non-empty union
    zero = np.zeros((3, 5), np.float32)
    pm, vm, iou, iou_v = visibility_and_iou(zero + 0.7, zero, np.zeros((3, 5), bool), np.zeros((3, 5), bool))
    assert not pm.any() and not vm.any() and np.isnan(iou) and np.isnan(iou_v)      # an all-empty union


# ---- ADD / ADI -----------------------------------------------------------------------------------------------------------------
def test_pose_errors_sizes_and_lds_thresholds(hiplib):
    """ADI keeps the ground-truth cloud in dynamic LDS, 24 bytes a point: M = 2048 is exactly 48 KiB, 2049 the first size
    past it, 2730 / 2731 straddle 64 KiB, 6400 (150 KiB) is the largest accepted. The largest runs first and the smaller
    ones after it in the same process: the LDS attribute is set once per function. Against float64, at the 1e-10
    relative of the existing test (the kernel sums 256 partial sums by butterfly, numpy pairwise: both within M * 2^-53)."""
    from ossid_code_amd.scoring import pose_errors
    for M in pc.ADI_SIZES:
        T, gt, P = pc.pose_case(3, M)
        for symmetric in (True, False):
            got = pose_errors(T, gt, P, symmetric=symmetric)
            want = rpl.add_adi(T, gt, P, symmetric)
            assert got.dtype == np.float64 and got.shape == (3,)
            assert np.allclose(got, want, rtol=1e-10, atol=1e-13), (M, symmetric, got, want)
            assert (got[1:] > 0).all()
            if symmetric:
                assert got[0] < 1e-12
            else:
                assert got[0] == 0.0                            # the ground truth itself: exactly 0
    T, gt, P = pc.pose_case(70000, 4)                          # more hypotheses than a 16-bit grid axis holds
    got = pose_errors(T, gt, P)
    assert got.shape == (70000,) and got[0] == 0.0
    assert np.allclose(got, rpl.add_adi(T, gt, P, False), rtol=1e-10, atol=1e-13)
    assert pose_errors(T[:0], gt, P).shape == (0,) and pose_errors(T[:0], gt, P, symmetric=True).shape == (0,)


def test_pose_errors_refuses_more_points_than_lds_holds(hiplib):
    from ossid_code_amd.scoring import pose_errors
    T, gt, P = pc.pose_case(2, 6401)
    dT, dG, dP = _cuda(T), _cuda(gt), _cuda(P)
    err = torch.full((2,), -5.0, dtype=torch.float64, device="cuda")
    rc = hiplib.fn("ossid_pose_errors")(dT.data_ptr(), dG.data_ptr(), dP.data_ptr(), 2, 6401, 1, err.data_ptr(),
                                        hiplib.stream())
    torch.cuda.synchronize()
    assert rc == EINVAL and bool((err == -5.0).all())
    with pytest.raises(ValueError, match="model_points"):
        pose_errors(T, gt, P, symmetric=True)
    assert pose_errors(T, gt, P, symmetric=False).shape == (2,)           # ADD has no such limit


# ---- the truncating projection ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def z(hiplib):
    from ossid_code_amd import zephyr
    return zephyr


def _featurizer_all(z, ozr, T, pts, depth, margin):
    """projectPointsUv, inconst_count and featurize (both interp values) on the GPU, each bit for bit against the C
    oracle; returns uv [N,M,2] and the counts"""
    nrm, col = pc.model_table_inputs(len(pts))
    rgb = pc.rgb_frame()
    dev = torch.device("cuda", 0)
    rgbd = z.stage_frame(rgb, depth, dev)
    tab = z.stage_model(pts, nrm, col, dev)
    rgbd_o, tab_o = ozr.pack_rgbd(rgb, depth), ozr.prep_model(pts, nrm, col)
    assert np.array_equal(rgbd.cpu().numpy(), rgbd_o) and np.array_equal(tab.cpu().numpy(), tab_o)
    T32 = T.astype(np.float32)
    dT = _cuda(T32)
    cam = tuple(float(np.float32(v)) for v in (pc.K_EDGE[0, 0], pc.K_EDGE[1, 1], pc.K_EDGE[0, 2], pc.K_EDGE[1, 2]))
    uv = z.projectPointsUv(T, pts, _meta(pc.K_EDGE))
    assert uv.dtype == np.int64 and np.array_equal(uv, ozr.project_uv(T, pts, pc.K_EDGE))
    cnt = z.inconst_count(rgbd, dT, tab, cam, margin=margin).cpu().numpy()
    assert np.array_equal(cnt, ozr.inconst_count(rgbd_o, T32, tab_o, pc.K_EDGE, margin=margin))
    px_rf, uv_rf, cnt_rf = rf.featurize(rgbd_o, T32, pts, nrm, col, pc.K_EDGE)      # float32 numpy, its margin is 0.02
    assert np.array_equal(z.inconst_count(rgbd, dT, tab, cam).cpu().numpy(), cnt_rf) and np.array_equal(uv, uv_rf)
    for interp in (0, 1):
        px, fuv = z.featurize(rgbd, dT, tab, cam, interp=interp)
        px_o, uv_o = ozr.featurize(rgbd_o, T32, tab_o, pc.K_EDGE, interp=interp)
        assert np.array_equal(fuv.cpu().numpy(), uv_o) and np.array_equal(fuv.cpu().numpy(), uv)
        assert np.array_equal(px.cpu().numpy(), px_o) and (interp or np.array_equal(px_o, px_rf))
    return uv, cnt


def test_projection_edges(z, ozr):
    """u_f in (-1, 0) truncates to pixel 0 and is in the frame (SPEC.md 3.2); the splat floors the same point off it."""
    pts, depth = pc.proj_case()
    T = pc.EYE[None]
    uv, cnt = _featurizer_all(z, ozr, T, pts, depth, pc.MARGIN)
    assert np.array_equal(uv, rpl.project(T, pts, pc.K_EDGE)[0]) and np.array_equal(uv, rf.project(T, pts, pc.K_EDGE)[3])
    n = len(pc.PU_EDGES)
    assert uv[0, :n, 0].tolist() == [-1, 0, 0, 39, 40] and uv[0, n:2 * n, 1].tolist() == [-1, 0, 0, 23, 24]
    assert uv[0, -4:].tolist() == [[-1, -1], [0, 0], [-1, -1], [-1, -1]]      # z' = 1e-6, the next float, 0, negative
    assert np.array_equal(cnt, rpl.inconst_count(depth, T, pts, pc.K_EDGE, pc.MARGIN)) and cnt.tolist() == [9]
    T2, pts2, depth2 = pc.proj_case_near()                     # one pose 1e-6 in front of the camera
    uv2, cnt2 = _featurizer_all(z, ozr, T2[None], pts2, depth2, pc.MARGIN)
    assert np.array_equal(uv2, rpl.project(T2[None], pts2, pc.K_EDGE)[0])
    assert np.array_equal(uv2, rf.project(T2[None], pts2, pc.K_EDGE)[3])
    assert uv2[0].tolist() == [[-1, -1], [0, 0], [25, 12], [-1, -1]]
    assert np.array_equal(cnt2, rpl.inconst_count(depth2, T2[None], pts2, pc.K_EDGE, pc.MARGIN)) and cnt2.tolist() == [2]


def test_filter_hypo_by_mask_threshold_and_truncation(z):
    from ossid_code_amd.scoring import filterHypoByMask
    pts, T, mask, frac = pc.mask_filter_case()
    meta = _meta(pc.K_EDGE)
    got = filterHypoByMask(pts, meta, T, mask, th=0.5)
    assert got.dtype == bool and got.tolist() == [True, False, False, False, False]    # 0.75 kept; exactly 0.5 not
    assert np.array_equal(got, rpl.mask_fraction(mask, T, pts, pc.K_EDGE) > 0.5)
    assert filterHypoByMask(pts, meta, T, mask, th=0.25).tolist() == [True, True, False, False, False]
    assert filterHypoByMask(pts, meta, T[:0], mask).shape == (0,)


def test_filter_hypo_by_mask_more_hypotheses_than_one_launch_takes(z):
    from ossid_code_amd.scoring import filterHypoByMask
    pts, _, mask, _ = pc.mask_filter_case()
    N = 65536 + 3
    T = pc.many_poses(N)
    meta = _meta(pc.K_EDGE)
    got = filterHypoByMask(pts, meta, T, mask, th=0.2)
    parts = [filterHypoByMask(pts, meta, T[i:i + 30000], mask, th=0.2) for i in range(0, N, 30000)]
    assert got.shape == (N,) and np.array_equal(got, np.concatenate(parts))
    assert np.array_equal(got, rpl.mask_fraction(mask, T, pts, pc.K_EDGE) > 0.2) and 0 < got.sum() < N
    uv = z.projectPointsUv(T, pts, meta)                       # the same chunking behind projectPointsUv
    assert np.array_equal(uv, rpl.project(T, pts, pc.K_EDGE)[0])
