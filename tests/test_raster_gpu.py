"""csrc/raster.hip against the restatement tests/ref_raster.py (SPEC.md section 7), through the C ABI: bit equality of
the depth image and of the contractual statistics -- no tolerance and no pixel left out --, the wave-cooperative path
where it must run, batches, reproducibility, capture, and the Renderer / OnlineStream wiring."""
import numpy as np
import pytest
import torch

import ref_icp as ri
import ref_ppf as rp
import ref_raster as rr
from ossid_code_amd import synth

pytestmark = pytest.mark.gpu

HW = (480, 640)
NEAR, NEARER = (0.03, 0.02, 0.12), (0.0, 0.02, 0.07)


def _poses():
    """name -> pose: the three of ref_ppf, near (fills the frame), nearer (z_near drops triangles), half out of the frame,
    behind the camera."""
    out = {"p%d" % k: rp.gt_pose(k) for k in range(3)}
    out.update(near=rr.pose_at(NEAR), nearer=rr.pose_at(NEARER), half_out=rr.pose_at((0.41, 0.06, 0.75)),
               behind=rr.pose_at((0.05, 0.02, -0.75)))
    return out


def _raster(hiplib, V, F, poses, K, hw, offset=0.5, z_near=0.05, scale=1.0, stream=None):
    """ossid_raster_depth on host arrays -> (depth f32 [N,H,W], stats int32 [N,4]) as numpy."""
    dev = torch.device("cuda", 0)
    v = torch.from_numpy((np.asarray(V, dtype=np.float64) * scale).astype(np.float32)).to(dev).contiguous()
    f = torch.from_numpy(np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)).to(dev)
    T = torch.from_numpy(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).astype(np.float32)).to(dev).contiguous()
    N, (H, W) = int(T.shape[0]), hw
    need = int(hiplib.fn("ossid_raster_workspace_bytes")(len(v), len(f), N))
    assert need == 16 * N * len(v)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    depth = torch.full((N, H, W), -1.0, dtype=torch.float32, device=dev)
    stats = torch.full((N, 4), -1, dtype=torch.int32, device=dev)
    k = [float(np.float32(x)) for x in (K[0][0], K[1][1], K[0][2], K[1][2])]
    rc = hiplib.fn("ossid_raster_depth")(v.data_ptr(), len(v), f.data_ptr() if len(f) else None, len(f), T.data_ptr(), N, *k, H,
                                         W, float(offset), float(z_near), ws.data_ptr(), need, depth.data_ptr(),
                                         stats.data_ptr(), hiplib.stream() if stream is None else stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return depth.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("offset", [0.0, 0.5])
@pytest.mark.parametrize("level", [0, 1, 3, 5])
def test_bit_equal_to_the_restatement(hiplib, level, offset):
    V, F = rr.bump_mesh(level)
    poses = _poses()
    got, stats = _raster(hiplib, V, F, np.stack(list(poses.values())), synth.CAM_K, HW, offset)
    for i, (name, T) in enumerate(poses.items()):
        want, _count, wstats = rr.render(V, F, T, synth.CAM_K, HW, pixel_offset=offset)
        print("level %d offset %.1f %-8s pixels %6d stats %s" % (level, offset, name, (want > 0).sum(), stats[i].tolist()))
        assert np.array_equal(got[i], want), (name, int((got[i] != want).sum()))
        assert stats[i, :3].tolist() == wstats.tolist(), name
        if name == "behind":
            assert not got[i].any() and stats[i, 0] == len(F)
        else:
            assert got[i].any()


def test_odd_frame_size_and_single_pose(hiplib):
    H, W = 123, 77
    K = synth.CAM_K.copy()
    K[0] *= W / 640.0
    K[1] *= H / 480.0
    V, F = rr.bump_mesh(3)
    for T in (rp.gt_pose(0), rr.pose_at((0.01, 0.01, 0.12))):
        for offset in (0.0, 0.5):
            got, stats = _raster(hiplib, V, F, T, K, (H, W), offset)
            want, _c, wstats = rr.render(V, F, T, K, (H, W), pixel_offset=offset)
            assert want.any() and np.array_equal(got[0], want) and stats[0, :3].tolist() == wstats.tolist()


def test_large_triangle_path_runs_where_it_must(hiplib):
    V, F = rr.bump_mesh(0)
    _d, stats = _raster(hiplib, V, F, rr.pose_at(NEAR), synth.CAM_K, HW)
    assert stats[0, 3] > 0, stats
    V, F = rr.bump_mesh(5)
    _d, stats = _raster(hiplib, V, F, rp.gt_pose(0), synth.CAM_K, HW)
    assert stats[0, 3] == 0 and stats[0, 2] > 0, stats


def test_full_size_mesh(hiplib):
    """Level 7: 655 360 triangles, one pose."""
    V, F = rr.bump_mesh(7)
    assert len(F) == 655360
    got, stats = _raster(hiplib, V, F, rp.gt_pose(0), synth.CAM_K, HW, 0.5)
    want, _c, wstats = rr.render(V, F, rp.gt_pose(0), synth.CAM_K, HW, pixel_offset=0.5)
    assert np.array_equal(got[0], want) and stats[0, :3].tolist() == wstats.tolist()
    print("level 7 stats", stats[0].tolist())


def test_contract_corners_on_the_device(hiplib):
    """The CPU test's corners through the kernel: ownership on exact samples, degenerate / unusable triangles, F = 0,
    the millimetre scale, and refusals before any launch."""
    K1 = np.array([[100.0, 0, 0], [0, 100.0, 0], [0, 0, 1]])
    hw = (16, 16)
    sq = np.array([[0.02, 0.02, 1.0], [0.06, 0.02, 1.0], [0.06, 0.06, 1.0], [0.02, 0.06, 1.0]])
    bad = np.vstack([sq, [[np.nan, 0.0, 1.0]], [[0.0, 0.0, -1.0]], [[0.0, 0.0, 0.05]], [[np.inf, 0.0, 1.0]], [[1e30, 0.0, 1.0]]])
    faces = [[0, 1, 2], [0, 2, 3], [0, 1, 1], [0, 1, 4], [0, 1, 5], [0, 1, 6], [0, 1, 7], [0, 1, 8], [0, 3, 2]]
    for offset in (0.0, 0.5, 1.0):
        got, stats = _raster(hiplib, bad, faces, np.eye(4), K1, hw, offset)
        want, _c, wstats = rr.render(bad, faces, np.eye(4), K1, hw, pixel_offset=offset)
        assert np.array_equal(got[0], want) and stats[0, :3].tolist() == wstats.tolist() == [5, 1, 3]
    got, stats = _raster(hiplib, bad, faces, np.eye(4), K1, hw, 0.0)
    ref = np.zeros(hw, np.float32)
    ref[3:7, 3:7] = 1.0
    assert np.array_equal(got[0], ref)
    got, stats = _raster(hiplib, sq, np.zeros((0, 3), np.int32), np.eye(4), K1, hw)
    assert not got.any() and not stats.any()
    got, _s = _raster(hiplib, sq * 1000.0, faces[:2], np.eye(4), K1, hw, 0.0, scale=0.001)
    want, _c, _w = rr.render(sq * 1000.0, faces[:2], np.eye(4), K1, hw, pixel_offset=0.0, scale=0.001)
    assert np.array_equal(got[0], want) and want.any()
    # refusals: OSSID_EINVAL before any device work
    fn, wsb = hiplib.fn("ossid_raster_depth"), hiplib.fn("ossid_raster_workspace_bytes")
    assert wsb(0, 1, 1) == 0 and wsb(1, -1, 1) == 0 and wsb(1, 1, 0) == 0 and wsb(1, 1, 257) == 0
    assert wsb((1 << 22) + 1, 1, 1) == 0 and wsb(1, (1 << 22) + 1, 1) == 0 and wsb(3, 0, 2) == 96
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")        # all-zero vertices, faces and transform: nothing drawn
    p = buf.data_ptr()
    args = (("v", p), ("V", 3), ("f", p + 1024), ("F", 1), ("T", p + 2048), ("N", 1), ("fx", 1.0), ("fy", 1.0), ("cx", 0.0),
            ("cy", 0.0), ("H", 4), ("W", 4), ("o", 0.5), ("zn", 0.05), ("ws", p + 4096), ("wb", 48), ("out", p + 8192),
            ("st", None), ("s", hiplib.stream()))
    call = lambda **kw: fn(*[kw.get(k, d) for k, d in args])  # noqa: E731
    assert call() == 0
    for kw in ({"V": 0}, {"F": -1}, {"N": 0}, {"N": 257}, {"H": 0}, {"H": 4097, "W": 4096}, {"o": 1.5}, {"o": -0.1},
               {"o": float("nan")}, {"zn": -1.0}, {"zn": float("inf")}, {"wb": 47}, {"ws": None}, {"out": None}, {"v": None},
               {"f": None}, {"T": None}, {"ws": p + 4100}):
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()


def test_batch_repeat_and_capture(hiplib):
    from ossid_code_amd import render
    V, F = rr.bump_mesh(3)
    mesh = render.Mesh(V, F)
    poses = np.stack([rp.gt_pose(k % 3) for k in range(8)])
    for k in range(8):
        poses[k, :3, 3] += [0.01 * k, -0.005 * k, 0.02 * k]
    poses[7] = rr.pose_at(NEAR)
    batch, bstats = render.render_depth(mesh, poses, synth.CAM_K, HW, return_stats=True)
    again = render.render_depth(mesh, poses, synth.CAM_K, HW)
    assert batch.shape == (8, 480, 640) and batch.is_cuda and torch.equal(batch, again)
    for k in range(8):
        one, st = render.render_depth(mesh, poses[k], synth.CAM_K, HW, return_stats=True)
        assert one.shape == (480, 640) and torch.equal(one, batch[k]) and torch.equal(st, bstats[k])
    # poses as a device tensor give the same image
    assert torch.equal(render.render_depth(mesh, torch.from_numpy(poses).cuda(), synth.CAM_K, HW), batch)
    # the call only enqueues: it can be captured on a side stream and replayed
    T = torch.from_numpy(poses[:2]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        render.render_depth(mesh, T, synth.CAM_K, HW)          # warm-up outside the capture (workspace allocation)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = render.render_depth(mesh, T, synth.CAM_K, HW)
    for _ in range(2):
        out.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, batch[:2])


def _write_ply_mm(path, V, F):
    head = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(V), "property float x", "property float y",
            "property float z", "element face %d" % len(F), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        f.write((V * 1000.0).astype("<f4").tobytes())
        rows = np.zeros(len(F), dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
        rows["n"], rows["i"] = 3, F
        f.write(rows.tobytes())


def test_renderer_drop_in_end_to_end(hiplib, tmp_path):
    from ossid_code_amd import pipeline, render
    from ossid_code_amd.hostutil import K2meta
    V, F = rr.bump_mesh(3)
    path = str(tmp_path / "obj_000001.ply")
    _write_ply_mm(path, V, F)
    r = render.Renderer(K2meta(synth.CAM_K))
    r.addObject(1, path, pose=np.eye(4), mm2m=True)
    r.obj_nodes[1].matrix = rp.gt_pose(0)
    color, depth = r.render(depth_only=True)
    assert color is None and isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == HW
    Vmm, Fr = render.read_ply_mesh(path)
    want = render.render_depth(render.Mesh(Vmm, Fr, scale=0.001), rp.gt_pose(0), synth.CAM_K, HW).cpu().numpy()
    assert np.array_equal(depth, want) and 0.6 < depth[depth > 0].min() < depth.max() < 0.9          # metres
    ref, _c, _s = rr.render(Vmm, Fr, rp.gt_pose(0), synth.CAM_K, HW, scale=0.001)
    assert np.array_equal(depth, ref)
    # the pose follows the node
    r.obj_nodes[1].matrix = rp.gt_pose(1)
    assert np.array_equal(r.render(depth_only=True)[1],
                          render.render_depth(r._mesh(1), rp.gt_pose(1), synth.CAM_K, HW).cpu().numpy())
    # two objects share the image: the nearest positive depth
    r.addObject(2, path, pose=rr.pose_at((-0.08, 0.02, 0.6)), mm2m=True)
    both = r.render(depth_only=True)[1]
    a = render.render_depth(r._mesh(1), rp.gt_pose(1), synth.CAM_K, HW).cpu().numpy()
    b = render.render_depth(r._mesh(2), r.obj_nodes[2].matrix, synth.CAM_K, HW).cpu().numpy()
    far = np.float32(np.inf)
    merged = np.minimum(np.where(a > 0, a, far), np.where(b > 0, b, far))
    assert np.array_equal(both, np.where(np.isinf(merged), np.float32(0), merged)) and ((a > 0) & (b > 0)).any()
    # the visibility step takes the drop-in's output
    scene_depth = ri.render_into(synth.make_frame(42)[1], rp.gt_pose(0), synth.CAM_K)
    pm, vm, _i, _iv = pipeline.visibility_and_iou(scene_depth, depth)
    assert int(pm.sum()) == int((depth > 0).sum()) and 0 < int(vm.sum()) <= int(pm.sum())


def test_online_stream_renders_the_mesh(hiplib):
    from ossid_code_amd import dtoid, pipeline, render, zephyr
    from ossid_code_amd.stream import OnlineStream

    class _Args:
        dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0

    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", _Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, _Args(), num_class=1), 0).to(0).eval()
    g = torch.Generator().manual_seed(1)
    limg = torch.rand(3, 3, 124, 124, generator=g)
    lmask = (torch.rand(3, 1, 124, 124, generator=g) > 0.5).float()
    frames = []
    for f in range(3):
        d = synth.make_scoring_inputs(64, 512, seed=200 + f)
        d.update(limg=limg, lmask=lmask, obj_id=1, pose_gt=d["pose_hypos"][0].copy())
        frames.append(d)
    mesh = render.Mesh(*rr.bump_mesh(4))
    stream = OnlineStream(det, scorer, ds, confident_threshold=-1e30, meshes={1: mesh})
    results, _ = stream.run(frames, finetune_interval=100)
    assert set(stream.times) == {"detect", "pose_err", "score", "pseudo_label"}
    for r, fr in zip(results, frames):
        pred = render.render_depth(mesh, r["pred_pose"], fr["cam_K"], HW, pixel_offset=0.0)
        want = pipeline.visibility_and_iou(fr["depth"], pred)[1]
        assert r["pred_mask_visib"].dtype == torch.bool and torch.equal(r["pred_mask_visib"], want)
        assert int(pred.gt(0).sum()) > 0
        assert r["sample"] is not None and r["sample"]["mask"].shape == (1, 480, 640)
    # on the asymmetric scene, rendered at the true pose, the mesh mask is the object's mask
    depth, K, T, pts = ri.scene()
    ana = ri.render_into(np.zeros(HW, np.float32), T, K)
    mesh5 = render.Mesh(*rr.bump_mesh(5))
    pred = render.render_depth(mesh5, T, K, HW, pixel_offset=0.0)
    visible = (ana > 0) & (depth == ana)
    _pm, _vm, iou, iou_v = pipeline.visibility_and_iou(depth, pred, gt_mask=ana > 0, gt_mask_visib=visible)
    splat = pipeline.render_depth_points(T, pts, K, HW, radius=1)
    _pm, _vm, iou_s, iou_vs = pipeline.visibility_and_iou(depth, splat, gt_mask=ana > 0, gt_mask_visib=visible)
    print("IoU with the analytic mask at T_gt: mesh %.5f (visible %.5f), splat of 2048 points %.5f (visible %.5f)"
          % (iou, iou_v, iou_s, iou_vs))
    assert iou >= 0.995
