"""The model cloud from a mesh on the device (csrc/model_cloud.hip, SPEC.md section 9) against the numpy restatement
tests/ref_model_cloud.py -- bit for bit, stage by stage, each stage restated from the previous stage's KERNEL output --
and against ground truths that are not this code: the analytic ellipsoid and bump of ref_icp, a reversed mesh, a hidden
inner shell, the planes of the faces, numpy's brute-force diameter."""
import numpy as np
import pytest
import torch

import ref_icp as ri
import ref_model_cloud as rm
import ref_raster as rr
import ref_raster_color as rc

pytestmark = pytest.mark.gpu


def _same(a, b):
    """Bit equality of two arrays (tensors are copied to the host)."""
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ints(t):
    return [int(x) for x in (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).reshape(-1)]


def _mesh(V, F):
    from ossid_code_amd import render
    C = rc.axis_colors(V)[0]
    return C, render.Mesh(V, F, colors=C)


def _face_ids(mesh, info, S):
    """The kernel's own face-id images of every view of `info`, int32 numpy [n,S,S]."""
    from ossid_code_amd import render
    R = info["rotations"]
    poses = np.tile(np.eye(4), (len(R), 1, 1))
    poses[:, :3, :3], poses[:, 2, 3] = R, info["distance"]
    _c, _d, fid = render.render_color(mesh, poses, None, (S, S), 0.5, info["z_near"], intrinsics=info["intrinsics"],
                                      return_face_id=True)
    return fid.cpu().numpy()


def _check_fps_properties(points, sel, rad):
    """radius[1:] never grows, and every candidate lies within radius[M-1] of a pick: f32, the kernel's expression, formed
    by torch's separately rounded elementwise kernels on the device."""
    P = points if torch.is_tensor(points) else torch.from_numpy(np.asarray(points, dtype=np.float32)).cuda()
    rad_h = rad.cpu().numpy()
    assert rad_h[0] == np.inf and (np.diff(rad_h[1:]) <= 0).all()
    picks = P[sel.long()]
    near = torch.full((len(P),), float("inf"), device=P.device)
    for a in range(0, len(picks), 512):
        q = picks[a:a + 512]
        dx, dy, dz = (P[:, None, c] - q[None, :, c] for c in range(3))
        near = torch.minimum(near, ((dx * dx + dy * dy) + dz * dz).min(1).values)
    assert float(near.max()) <= float(rad_h[-1])


# ---- stage by stage ----------------------------------------------------------------------------------------------------------
S1 = 128


@pytest.fixture(scope="module")
def staged(hiplib):
    """bump_mesh(2), level-1 grid (42 views) at 128 x 128, K = 2048, M = 256, run with two chunkings."""
    from ossid_code_amd import model_cloud
    V, F = rr.bump_mesh(2)
    C, mesh = _mesh(V, F)
    kw = dict(n_points=256, oversample=8, level=1, view_size=S1, return_info=True)
    cloud, info = model_cloud.sample_model_cloud(mesh, views_per_call=5, **kw)
    cloud2, info2 = model_cloud.sample_model_cloud(mesh, views_per_call=42, **kw)
    return V, F, C, mesh, cloud, info, cloud2, info2


def test_votes_equal_the_restatement_whatever_the_chunking(staged):
    from ossid_code_amd import render
    V, F, C, mesh, cloud, info, cloud2, info2 = staged
    assert info["votes"].dtype == torch.int32 and tuple(info["votes"].shape) == (len(F), 2)
    assert torch.equal(info["votes"], info2["votes"])
    assert np.array_equal(info["rotations"], render.view_grid(1)) and len(info["rotations"]) == 42
    assert np.array_equal(info["centres"], rm.camera_centres(info["rotations"], info["distance"]))
    V32 = mesh.vertices.cpu().numpy()
    assert _same(V32, rm.f32_vertices(V))
    r = float(np.sqrt((V32.astype(np.float64) ** 2).sum(1).max()))
    assert info["distance"] == 4.0 * r and info["z_near"] == r
    fid = _face_ids(mesh, info, S1)
    want = rm.votes(fid, V32, F, info["centres"])
    assert np.array_equal(info["votes"].cpu().numpy().astype(np.int64), want)
    assert int(want.sum()) == int((fid >= 0).sum()) > 42 * 1000
    # wound outwards: seen from the front; where the two solids overlap faces are hidden
    assert (want[:, 0] >= want[:, 1]).all() and (want.sum(1) == 0).any()
    for k in ("model_points", "model_normals", "model_colors"):
        assert _same(getattr(cloud, k), getattr(cloud2, k))


def test_weights_prefix_and_normals_equal_the_restatement(staged):
    V, F, C, mesh, cloud, info = staged[:6]
    V32 = mesh.vertices.cpu().numpy()
    w, P, nrm, usable = rm.weights(V32, F, info["votes"].cpu().numpy())
    assert _ints(info["weights"]) == _ints(w) and _ints(info["prefix"]) == _ints(P)
    assert _same(info["face_normals"], nrm)
    assert usable.any() and not usable.all() and max(_ints(w)) == 1 << 32


def test_candidates_equal_the_restatement(staged):
    V, F, C, mesh, cloud, info = staged[:6]
    V32 = mesh.vertices.cpu().numpy()
    cand = info["candidates"]
    assert tuple(cand["points"].shape) == (2048, 3)
    pts, cn, col, face = rm.candidates(V32, F, C, info["votes"].cpu().numpy(), info["prefix"].cpu().numpy().astype(np.uint64),
                                       info["face_normals"].cpu().numpy(), 2048)
    assert _same(cand["face"], face) and _same(cand["points"], pts) and _same(cand["normals"], cn) and _same(cand["colors"], col)
    assert (info["votes"].cpu().numpy().sum(1)[face] > 0).all()                 # visible faces only


def test_selection_and_radius_equal_the_restatement(staged):
    V, F, C, mesh, cloud, info = staged[:6]
    pts = info["candidates"]["points"]
    sel, rad = rm.fps(pts.cpu().numpy(), 256)
    assert _same(info["selection"], sel) and _same(info["radius"], rad)
    _check_fps_properties(pts, info["selection"], info["radius"])
    idx = info["selection"].long()
    assert _same(cloud.model_points, pts[idx]) and _same(cloud.model_normals, info["candidates"]["normals"][idx])
    assert _same(cloud.model_colors, info["candidates"]["colors"][idx])
    assert cloud.model_points.dtype == torch.float32 and cloud.model_points.is_cuda and len(cloud) == 256
    assert cloud.diameter == rm.diameter(mesh.vertices.cpu().numpy())[1]


def test_end_to_end_equals_the_restatement_rendering_itself(hiplib):
    from ossid_code_amd import model_cloud
    V, F = rr.bump_mesh(1)
    C, mesh = _mesh(V, F)
    cloud, info = model_cloud.sample_model_cloud(mesh, n_points=64, oversample=8, level=0, view_size=64, return_info=True)
    want = rm.sample(V, F, C, info["rotations"], info["intrinsics"], info["distance"], info["z_near"], 64, 64, 512)
    assert np.array_equal(info["votes"].cpu().numpy().astype(np.int64), want["votes"])
    assert _ints(info["weights"]) == _ints(want["weights"]) and _ints(info["prefix"]) == _ints(want["prefix"])
    assert _same(info["face_normals"], want["face_normals"])
    for k in ("points", "normals", "colors", "face"):
        assert _same(info["candidates"][k], want[k]), k
    assert _same(info["selection"], want["selection"]) and _same(info["radius"], want["radius"])
    for k in ("model_points", "model_normals", "model_colors"):
        assert _same(getattr(cloud, k), want[k]), k


def test_all_defaults_from_the_votes_onward(hiplib):
    from ossid_code_amd import model_cloud
    V, F = rr.bump_mesh(5)
    C, mesh = _mesh(V, F)
    cloud, info = model_cloud.sample_model_cloud(mesh, return_info=True)
    assert len(info["rotations"]) == 162 and tuple(info["candidates"]["points"].shape) == (32768, 3) and len(cloud) == 2048
    V32 = mesh.vertices.cpu().numpy()
    votes = info["votes"].cpu().numpy()
    w, P, nrm, usable = rm.weights(V32, F, votes)
    assert _ints(info["weights"]) == _ints(w) and _ints(info["prefix"]) == _ints(P) and _same(info["face_normals"], nrm)
    pts, cn, col, face = rm.candidates(V32, F, C, votes, P, nrm, 32768)
    for k, ref in (("points", pts), ("normals", cn), ("colors", col), ("face", face)):
        assert _same(info["candidates"][k], ref), k
    sel, rad = rm.fps(pts, 2048)
    assert _same(info["selection"], sel) and _same(info["radius"], rad)
    assert _same(cloud.model_points, pts[sel]) and _same(cloud.model_normals, cn[sel]) and _same(cloud.model_colors, col[sel])


# ---- FPS alone -----------------------------------------------------------------------------------------------------------------
def _fps_case(P, M):
    from ossid_code_amd import model_cloud
    sel, rad = model_cloud.fps(P, M)
    want_sel, want_rad = rm.fps(P, M)
    assert _same(sel, want_sel) and _same(rad, want_rad)
    _check_fps_properties(P, sel, rad)
    return sel, rad


def test_fps_on_a_lattice_full_of_ties(hiplib):
    g = np.arange(16, dtype=np.float32) * np.float32(0.125)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    sel, rad = _fps_case(P, 512)
    assert len(set(_ints(sel))) == 512


def test_fps_at_the_caps(hiplib):
    P = np.random.default_rng(3).normal(size=(32768, 3)).astype(np.float32)
    sel, rad = _fps_case(P, 4096)
    assert len(set(_ints(sel))) == 4096


@pytest.mark.parametrize("K,M", [(1, 1), (2, 2), (300, 300), (1025, 1025), (1024, 64), (2049, 64), (4097, 64), (8193, 64),
                                 (16385, 64), (31999, 7)])
def test_fps_sizes_around_every_per_lane_count(hiplib, K, M):
    """K = 1, M = K (every point is picked; with duplicates), and the sizes at which a lane starts to own 2, 4, 8, 16, 32
    candidates."""
    P = np.random.default_rng(K).normal(size=(K, 3)).astype(np.float32)
    if K >= 300:
        P[K // 2] = P[5]                                                        # a duplicate: its tmp is 0 from pick 5 on
    sel, rad = _fps_case(P, M)
    if (K, M) == (1, 1):
        assert _ints(sel) == [0] and rad.cpu().numpy()[0] == np.inf


# ---- ground truths that are not this code -----------------------------------------------------------------------------------
def test_reversed_faces_give_the_same_cloud_with_outward_normals(hiplib):
    from ossid_code_amd import model_cloud
    V, F = rr.ellipsoid_mesh(3)
    kw = dict(n_points=256, oversample=8, level=1, view_size=128, return_info=True)
    cloud, info = model_cloud.sample_model_cloud(_mesh(V, F)[1], **kw)
    rev, info_r = model_cloud.sample_model_cloud(_mesh(V, F[:, [0, 2, 1]])[1], **kw)
    vt, vr = info["votes"].cpu().numpy(), info_r["votes"].cpu().numpy()
    assert np.array_equal(vt[:, ::-1], vr) and (vt[:, 0] >= vt[:, 1]).all() and vt.any()     # g, and with it t, changes sign
    assert _same(cloud.model_points, rev.model_points) and _same(cloud.model_colors, rev.model_colors)
    assert _same(info["candidates"]["points"], info_r["candidates"]["points"])
    for c in (cloud, rev):
        p, n = c.model_points.cpu().numpy().astype(np.float64), c.model_normals.cpu().numpy().astype(np.float64)
        assert ((n * (p / ri.AXES ** 2)).sum(1) > 0).all()                      # n . grad(x^2/a^2 + y^2/b^2 + z^2/c^2)
        assert np.abs(np.sqrt((n * n).sum(1)) - 1.0).max() < 1e-6


def test_a_shell_inside_the_ellipsoid_is_never_sampled(hiplib):
    from ossid_code_amd import model_cloud
    Ve, Fe = rr.ellipsoid_mesh(3)
    Vi, Fi = rr.icosphere(1)
    V = np.concatenate([Ve, 0.005 * Vi])                                         # the ellipsoid's smallest half-axis is 0.02
    F = np.concatenate([Fe, Fi + np.int32(len(Ve))])
    cloud, info = model_cloud.sample_model_cloud(_mesh(V, F)[1], n_points=256, oversample=8, level=1, view_size=128,
                                                 return_info=True)
    votes = info["votes"].cpu().numpy()
    assert not votes[len(Fe):].any() and votes[:len(Fe)].any()
    assert int(info["candidates"]["face"].max()) < len(Fe) and not any(_ints(info["weights"])[len(Fe):])


def test_against_the_two_analytic_solids_and_the_planes_of_the_faces(hiplib):
    """bump_mesh(3). (a) No candidate lies deeper inside the OTHER solid than the mesh's longest edge L: a face is kept
    iff one of its samples is seen, that sample is not inside the other solid, every point of the face is within L of it,
    and depth is 1-Lipschitz. Depth inside the bump is exact (a sphere); depth inside the ellipsoid is bounded from above
    by the distance to the surface along the gradient direction, so the assertion is no weaker than the statement.
    (b) Every candidate lies in the plane of its face: |n . (p - p0)| <= 2^-24 sum_i |n_i p_i| + 2^-47 r -- the f32
    rounding of each coordinate (half an ulp, 2^-24 relative) projected on the unit normal; the second term covers taking
    the rounded p in the first (2^-48 r) and the f64 rounding of the barycentric sum and of this very check (a few
    2^-53 r), r the largest vertex norm."""
    from ossid_code_amd import model_cloud
    V, F = rr.bump_mesh(3)
    C, mesh = _mesh(V, F)
    cloud, info = model_cloud.sample_model_cloud(mesh, n_points=1024, oversample=8, level=2, view_size=256, return_info=True)
    V32 = mesh.vertices.cpu().numpy()
    P64 = V32.astype(np.float64)
    edges = np.concatenate([P64[F[:, a]] - P64[F[:, b]] for a, b in ((0, 1), (1, 2), (2, 0))])
    L = float(np.sqrt((edges ** 2).sum(1)).max())
    p = info["candidates"]["points"].cpu().numpy().astype(np.float64)
    face = info["candidates"]["face"].cpu().numpy()
    votes = info["votes"].cpu().numpy()
    nE = len(F) // 2                                                             # faces [0, nE): ellipsoid, the rest: bump
    hidden = votes.sum(1) == 0
    assert hidden[:nE].any() and hidden[nE:].any() and not hidden[face].any()    # the test bites: parts of both are inside
    on_e = face < nE
    assert on_e.any() and (~on_e).any()
    depth_in_bump = ri.BUMP_R - np.sqrt(((p[on_e] - ri.BUMP_C) ** 2).sum(1))
    print("deepest ellipsoid candidate inside the bump: %.3e, L = %.3e" % (depth_in_bump.max(), L))
    assert depth_in_bump.max() <= L
    q = p[~on_e]
    lvl = ((q / ri.AXES) ** 2).sum(1) - 1.0
    q, lvl = q[lvl < 0], lvl[lvl < 0]
    n = q / ri.AXES ** 2
    n /= np.sqrt((n * n).sum(1))[:, None]
    A, B = ((n / ri.AXES) ** 2).sum(1), 2.0 * (q * n / ri.AXES ** 2).sum(1)
    t = (-B + np.sqrt(B * B - 4.0 * A * lvl)) / (2.0 * A)
    print("deepest bump candidate inside the ellipsoid: %.3e (of %d inside)" % (t.max(initial=0.0), len(q)))
    assert len(q) == 0 or t.max() <= L
    # (b)
    g, p0, _p1, _p2 = rm.face_cross(V32, F)
    nh = g[face] / np.sqrt((g[face] ** 2).sum(1))[:, None]
    r = float(np.sqrt((P64 ** 2).sum(1).max()))
    resid = np.abs((nh * (p - p0[face])).sum(1))
    tol = 2.0 ** -24 * np.abs(nh * p).sum(1) + 2.0 ** -47 * r
    print("plane residual / tolerance, worst: %.3f" % (resid / tol).max())
    assert (resid <= tol).all()
    # the cloud's normals are the faces', turned outwards: along the analytic gradient of the solid the face belongs to
    pc, nc = cloud.model_points.cpu().numpy().astype(np.float64), cloud.model_normals.cpu().numpy().astype(np.float64)
    fc = face[info["selection"].cpu().numpy()]
    grad = np.where((fc < nE)[:, None], pc / ri.AXES ** 2, pc - ri.BUMP_C)
    assert ((nc * grad).sum(1) > 0).all()


# ---- diameter --------------------------------------------------------------------------------------------------------------------
def test_diameter_equals_brute_force(hiplib):
    from ossid_code_amd import model_cloud, render
    P = np.random.default_rng(11).normal(size=(1000, 3))
    assert model_cloud.mesh_diameter(P) == rm.diameter(P.astype(np.float32))[1] > 0
    V, F = rr.icosphere(4)
    assert len(V) == 2562
    mesh = render.Mesh(V * np.array([0.05, 0.035, 0.02]), F)
    d = model_cloud.mesh_diameter(mesh)
    assert d == rm.diameter(mesh.vertices.cpu().numpy())[1] and abs(d - 0.1) < 1e-6
    assert model_cloud.mesh_diameter(np.array([[0.3, -1.0, 2.0]])) == 0.0


# ---- the stream ----------------------------------------------------------------------------------------------------------------
def test_stream_builds_an_objects_cloud_once(hiplib):
    from ossid_code_amd import model_cloud
    from ossid_code_amd.stream import OnlineStream
    V, F = rr.bump_mesh(1)
    C, mesh = _mesh(V, F)
    s = OnlineStream(None, None, None, meshes={4: mesh})
    a = s._with_cloud({"obj_id": 4, "img": 1})
    b = s._with_cloud({"obj_id": 4, "img": 2})
    want = model_cloud.sample_model_cloud(mesh)
    for k, t in want.as_dict().items():
        assert a[k] is b[k] and a[k].dtype == np.float32 and a[k].shape == (2048, 3) and _same(a[k], t)
    assert a["img"] == 1 and b["img"] == 2 and len(s._clouds) == 1
    own = {"obj_id": 4, "model_points": np.zeros((3, 3))}
    assert s._with_cloud(own) is own


def test_stream_scores_a_frame_without_a_cloud_as_the_same_frame_with_it(hiplib):
    from ossid_code_amd import dtoid, model_cloud, synth, zephyr
    from ossid_code_amd.stream import OnlineStream

    class Args:
        dataset, no_valid_proj, no_valid_depth, inconst_ratio_th, interp = "HSVD_diff_uv_norm", True, True, 100, 0

    torch.manual_seed(0)
    det = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    ds = zephyr.ScoreDataset([], "", "lmo", Args(), mode="test")
    scorer = synth.random_pn2_state(zephyr.PointNet2SSG(ds.dim_point, Args(), num_class=1), 0).to(0).eval()
    V, F = rr.bump_mesh(2)
    C, mesh = _mesh(V, F)
    g = torch.Generator().manual_seed(1)
    d = synth.make_scoring_inputs(16, 512, seed=200)
    d.update(limg=torch.rand(3, 3, 124, 124, generator=g), lmask=(torch.rand(3, 1, 124, 124, generator=g) > 0.5).float(),
             obj_id=1, pose_gt=d["pose_hypos"][0].copy())
    bare = {k: v for k, v in d.items() if k not in ("model_points", "model_normals", "model_colors")}
    cloud = model_cloud.sample_model_cloud(mesh)
    full = dict(bare, **{k: v.cpu().numpy() for k, v in cloud.as_dict().items()})
    got = OnlineStream(det, scorer, ds, meshes={1: mesh}).process(bare)
    want = OnlineStream(det, scorer, ds, meshes={1: mesh}).process(full)
    assert np.isfinite(got["pred_score"]) and got["pred_score"] == want["pred_score"] and got["pred_err"] == want["pred_err"]
    assert np.array_equal(got["pred_pose"], want["pred_pose"]) and torch.equal(got["pred_mask_visib"], want["pred_mask_visib"])
    assert "model_points" not in bare                                          # the caller's frame is left as it came
