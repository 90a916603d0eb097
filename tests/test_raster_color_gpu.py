"""ossid_raster_color and ossid_template_reduce (csrc/raster.hip) against the restatement tests/ref_raster_color.py
(SPEC.md 7.11-7.13), through the C ABI: bit equality of colour, depth, winning face and the contractual statistics -- no
tolerance and no pixel left out --, equality of the depth with ossid_raster_depth's, real ties, both walks, capture."""
import numpy as np
import pytest
import torch

import ref_ppf as rp
import ref_raster as rr
import ref_raster_color as rc
from ossid_code_amd import synth
from test_raster_gpu import HW, NEAR, _poses, _raster

pytestmark = pytest.mark.gpu


def _cams_of(K, n):
    return np.tile(np.array([K[0][0], K[1][1], K[0][2], K[1][2]], dtype=np.float32), (n, 1))


def _color(hiplib, V, F, C, poses, cams, hw, offset=0.5, z_near=0.05, stream=None, want_face=True):
    """ossid_raster_color on host arrays -> (color u8 [N,H,W,3], depth f32 [N,H,W], face int32 [N,H,W], stats int32 [N,4])."""
    dev = torch.device("cuda", 0)
    v = torch.from_numpy(np.asarray(V, dtype=np.float64).astype(np.float32)).to(dev).contiguous()
    f = torch.from_numpy(np.ascontiguousarray(F, dtype=np.int32).reshape(-1, 3)).to(dev)
    c = torch.from_numpy(np.ascontiguousarray(C, dtype=np.uint8)).to(dev)
    T = torch.from_numpy(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).astype(np.float32)).to(dev).contiguous()
    N, (H, W) = int(T.shape[0]), hw
    k = torch.from_numpy(np.ascontiguousarray(cams, dtype=np.float32).reshape(N, 4)).to(dev)
    need = int(hiplib.fn("ossid_raster_color_workspace_bytes")(len(v), len(f), N, H, W))
    assert need == 16 * N * len(v) + 8 * N * H * W
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    color = torch.full((N, H, W, 3), 77, dtype=torch.uint8, device=dev)
    depth = torch.full((N, H, W), -1.0, dtype=torch.float32, device=dev)
    face = torch.full((N, H, W), -7, dtype=torch.int32, device=dev)
    stats = torch.full((N, 4), -1, dtype=torch.int32, device=dev)
    rc_ = hiplib.fn("ossid_raster_color")(v.data_ptr(), len(v), f.data_ptr() if len(f) else None, len(f), c.data_ptr(),
                                          T.data_ptr(), N, k.data_ptr(), H, W, float(offset), float(z_near), ws.data_ptr(), need,
                                          color.data_ptr(), depth.data_ptr(), face.data_ptr() if want_face else None,
                                          stats.data_ptr(), hiplib.stream() if stream is None else stream)
    assert rc_ == 0, rc_
    torch.cuda.synchronize()
    return color.cpu().numpy(), depth.cpu().numpy(), face.cpu().numpy(), stats.cpu().numpy()


def _same(got, want, name):
    (gc, gd, gf, gs), (wc, wd, wf, ws) = got, want
    assert np.array_equal(gd, wd), (name, "depth", int((gd != wd).sum()))
    assert np.array_equal(gf, wf), (name, "face", int((gf != wf).sum()))
    assert np.array_equal(gc, wc), (name, "colour", int((gc != wc).any(-1).sum()))
    assert gs[:3].tolist() == ws.tolist(), (name, gs.tolist(), ws.tolist())


@pytest.mark.parametrize("offset", [0.0, 0.5])
@pytest.mark.parametrize("level", [0, 1, 3, 5])
def test_bit_equal_to_the_restatement(hiplib, level, offset):
    V, F = rr.bump_mesh(level)
    C, _k = rc.axis_colors(V)
    poses = _poses()
    P = np.stack(list(poses.values()))
    color, depth, face, stats = _color(hiplib, V, F, C, P, _cams_of(synth.CAM_K, len(P)), HW, offset)
    only_depth, dstats = _raster(hiplib, V, F, P, synth.CAM_K, HW, offset)
    assert np.array_equal(depth, only_depth) and np.array_equal(stats, dstats)            # the depth-only entry, same call
    for i, (name, T) in enumerate(poses.items()):
        want = rc.render(V, F, C, T, synth.CAM_K, HW, pixel_offset=offset)
        print("level %d offset %.1f %-8s pixels %6d stats %s" % (level, offset, name, (want[1] > 0).sum(), stats[i].tolist()))
        _same((color[i], depth[i], face[i], stats[i]), want, name)
        if name == "behind":
            assert not color[i].any() and (face[i] == -1).all() and stats[i, 0] == len(F)
        else:
            assert color[i].any()


def test_odd_frame_size_and_a_camera_per_pose(hiplib):
    H, W = 123, 77
    V, F = rr.bump_mesh(3)
    C, _k = rc.axis_colors(V)
    poses = [rp.gt_pose(0), rr.pose_at((0.01, 0.01, 0.12)), rp.gt_pose(1), rp.gt_pose(0)]
    # the frame's camera scaled to it, then three cameras of other focal lengths (fy = 1.25 fx) aimed near each object
    cams = np.array([[572.4114 * W / 640, 573.57043 * H / 480, 325.2611 * W / 640, 242.04899 * H / 480],
                     [60.0, 75.0, 36.75, 47.75], [300.0, 375.0, 56.0, 62.125], [900.0, 1125.0, -75.5, 11.5]], dtype=np.float32)
    for offset in (0.0, 0.5):
        color, depth, face, stats = _color(hiplib, V, F, C, np.stack(poses), cams, (H, W), offset)
        for i, T in enumerate(poses):
            want = rc.render(V, F, C, T, rc.cam_matrix(*[float(x) for x in cams[i]]), (H, W), pixel_offset=offset)
            assert want[1].any()
            _same((color[i], depth[i], face[i], stats[i]), want, i)
    # face_id is optional
    c2, d2, f2, _s = _color(hiplib, V, F, C, np.stack(poses), cams, (H, W), 0.5, want_face=False)
    assert np.array_equal(c2, color) and np.array_equal(d2, depth) and (f2 == -7).all()


def test_full_size_mesh_depth_equals_the_depth_entry(hiplib):
    """Level 7: 655 360 triangles, one pose; the depth of the colour entry is the depth-only entry's, bit for bit."""
    V, F = rr.bump_mesh(7)
    C, _k = rc.axis_colors(V)
    color, depth, face, stats = _color(hiplib, V, F, C, rp.gt_pose(0), _cams_of(synth.CAM_K, 1), HW)
    only_depth, dstats = _raster(hiplib, V, F, rp.gt_pose(0), synth.CAM_K, HW)
    assert np.array_equal(depth, only_depth) and np.array_equal(stats, dstats) and depth.any()
    assert np.array_equal(face >= 0, depth > 0) and face.max() < len(F) and color[depth > 0].any()


def test_real_ties_resolve_to_the_lowest_face_and_reproducibly(hiplib):
    V, F = rr.bump_mesh(3)
    C, _k = rc.axis_colors(V)
    poses = np.stack([rp.gt_pose(0), rr.pose_at(NEAR), rp.gt_pose(2), rr.pose_at((0.41, 0.06, 0.75))])
    cams = _cams_of(synth.CAM_K, len(poses))
    # the same faces twice: every sample of the second copy ties with the first
    F2 = np.concatenate([F, F])
    # two coincident copies of the surface with different colours, the second copy listed first
    V2, C2 = np.concatenate([V, V]), np.concatenate([C, 255 - C])
    F3 = np.concatenate([F + len(V), F])
    for Vx, Fx, Cx in ((V, F2, C), (V2, F3, C2)):
        got = _color(hiplib, Vx, Fx, Cx, poses, cams, HW)
        for i in range(len(poses)):
            want = rc.render(Vx, Fx, Cx, poses[i], synth.CAM_K, HW)
            _same(tuple(g[i] for g in got), want, i)
            assert got[2][i].max() < len(F)                                   # the lower index of every tied pair
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            again = _color(hiplib, Vx, Fx, Cx, poses, cams, HW, stream=side.cuda_stream)
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
        for i in range(len(poses)):                                           # another batch split
            one = _color(hiplib, Vx, Fx, Cx, poses[i], cams[i:i + 1], HW)
            assert all(np.array_equal(a[0], b[i]) for a, b in zip(one, got))
    single = _color(hiplib, V, F, C, poses, cams, HW)
    doubled = _color(hiplib, V, F2, C, poses, cams, HW)
    assert all(np.array_equal(a, b) for a, b in zip(single[:3], doubled[:3]))


def test_both_walks_give_the_restatements_colours(hiplib):
    V, F = rr.bump_mesh(0)
    C, _k = rc.axis_colors(V)
    T = rr.pose_at(NEAR)
    got = _color(hiplib, V, F, C, T, _cams_of(synth.CAM_K, 1), HW)
    want = rc.render(V, F, C, T, synth.CAM_K, HW)
    _same(tuple(g[0] for g in got), want, "near")
    assert got[3][0, 3] > 0, got[3]                             # the wave-cooperative walk ran
    V, F = rr.bump_mesh(5)
    C, _k = rc.axis_colors(V)
    got = _color(hiplib, V, F, C, rp.gt_pose(0), _cams_of(synth.CAM_K, 1), HW)
    want = rc.render(V, F, C, rp.gt_pose(0), synth.CAM_K, HW)
    _same(tuple(g[0] for g in got), want, "p0")
    assert got[3][0, 3] == 0 and got[3][0, 2] > 0, got[3]


def test_capture_and_replay_with_new_poses(hiplib):
    from ossid_code_amd import render
    V, F = rr.bump_mesh(3)
    C, _k = rc.axis_colors(V)
    mesh = render.Mesh(V, F, colors=C)
    sets = [np.stack([rp.gt_pose(0), rp.gt_pose(1)]), np.stack([rp.gt_pose(2), rr.pose_at(NEAR)]),
            np.stack([rr.pose_at((0.41, 0.06, 0.75)), rp.gt_pose(0)])]
    cam_sets = [_cams_of(synth.CAM_K, 2), _cams_of(synth.CAM_K, 2) * np.float32(0.5), _cams_of(synth.CAM_K, 2)]
    eager = [[t.clone() for t in render.render_color(mesh, p, None, HW, intrinsics=k, return_face_id=True, return_stats=True)]
             for p, k in zip(sets, cam_sets)]
    # cam_K and per-pose intrinsics that repeat it are the same call
    by_K = render.render_color(mesh, sets[0], synth.CAM_K, HW, return_face_id=True, return_stats=True)
    assert all(torch.equal(a, b) for a, b in zip(by_K, eager[0]))
    assert torch.equal(by_K[1], render.render_depth(mesh, sets[0], synth.CAM_K, HW))
    one = render.render_color(mesh, sets[0][1], synth.CAM_K, HW)
    assert one[0].shape == (480, 640, 3) and torch.equal(one[0], by_K[0][1]) and torch.equal(one[1], by_K[1][1])
    T = torch.from_numpy(sets[0]).to("cuda", torch.float32)
    Kd = torch.from_numpy(cam_sets[0]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        render.render_color(mesh, T, None, HW, intrinsics=Kd, return_face_id=True, return_stats=True)   # workspace allocation
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = render.render_color(mesh, T, None, HW, intrinsics=Kd, return_face_id=True, return_stats=True)
    for k in (1, 2, 0):
        T.copy_(torch.from_numpy(sets[k]))
        Kd.copy_(torch.from_numpy(cam_sets[k]))
        for t in out:
            t.fill_(3)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager[k])), k


@pytest.mark.parametrize("T", [31, 124])
@pytest.mark.parametrize("s", [1, 2, 4])
def test_template_reduce_equals_the_restatement(hiplib, s, T):
    rng = np.random.default_rng(10 * s + T)
    N, S = 3, s * T
    color = rng.integers(0, 256, size=(N, S, S, 3)).astype(np.uint8)
    depth = np.where(rng.random((N, S, S)) < 0.6, rng.random((N, S, S)).astype(np.float32) + 0.1, np.float32(0))
    depth[0] = 0                                                 # nothing covered
    depth[1, :S // 2] = 1.0                                      # cells fully covered
    c, d = torch.from_numpy(color).cuda(), torch.from_numpy(depth).cuda()
    img = torch.full((N, 3, T, T), -1.0, device="cuda")
    mask = torch.full((N, 1, T, T), -1.0, device="cuda")
    fn = hiplib.fn("ossid_template_reduce")
    assert fn(c.data_ptr(), d.data_ptr(), N, T, s, img.data_ptr(), mask.data_ptr(), hiplib.stream()) == 0
    torch.cuda.synchronize()
    for n in range(N):
        wi, wm = rc.box_reduce(color[n], depth[n], s)
        assert np.array_equal(img[n].cpu().numpy(), wi) and np.array_equal(mask[n].cpu().numpy(), wm)
    assert not img[0].any() and not mask[0].any() and (mask[1, 0, :T // 2 - 1] == 1).all()


def test_refusals_before_any_launch(hiplib):
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    fn = hiplib.fn("ossid_raster_color")
    args = (("v", p), ("V", 3), ("f", p + 1024), ("F", 1), ("c", p + 2048), ("T", p + 3072), ("N", 1), ("k", p + 4096), ("H", 4),
            ("W", 4), ("o", 0.5), ("zn", 0.05), ("ws", p + 8192), ("wb", 48 + 128), ("col", p + 16384), ("dep", p + 20480),
            ("face", None), ("st", None), ("s", hiplib.stream()))
    call = lambda **kw: fn(*[kw.get(k, d) for k, d in args])  # noqa: E731
    assert call() == 0                         # all-zero vertices, faces, transform and camera: nothing drawn
    for kw in ({"V": 0}, {"F": -1}, {"N": 0}, {"N": 257}, {"H": 0}, {"H": 4097, "W": 4096}, {"o": 1.5}, {"o": float("nan")},
               {"zn": -1.0}, {"zn": float("nan")}, {"wb": 48 + 127}, {"ws": None}, {"ws": p + 8196}, {"col": None},
               {"dep": None}, {"v": None}, {"f": None}, {"c": None}, {"T": None}, {"k": None}):
        assert call(**kw) == -22, kw
    red = hiplib.fn("ossid_template_reduce")
    rargs = (("c", p), ("d", p + 4096), ("N", 1), ("T", 4), ("s", 2), ("img", p + 8192), ("mask", p + 16384), ("st", hiplib.stream()))
    rcall = lambda **kw: red(*[kw.get(k, d) for k, d in rargs])  # noqa: E731
    assert rcall() == 0
    for kw in ({"s": 0}, {"s": 9}, {"T": 0}, {"T": 513}, {"N": 0}, {"N": 257}, {"c": None}, {"d": None}, {"img": None},
               {"mask": None}):
        assert rcall(**kw) == -22, kw
    torch.cuda.synchronize()
