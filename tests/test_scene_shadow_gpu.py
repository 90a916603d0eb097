"""csrc/scene_shadow.hip and ossid_scene_light_shadowed against the restatement tests/ref_scene_shadow.py (SPEC.md
13.13-13.15), bit for bit: two scenes of a table and three objects under a directional and a point light at two map sizes
that are no multiple of the 8 x 8 walk, byte-identical repeats, lights that cast nothing, an occluder whose shadow
darkens the table and nothing else, work lists and face rows that lead outside the arrays, a triangle across the light's
near plane, outputs between guard words, the refusals, and the unshadowed path untouched. Every frame is 48 x 64. No
tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import ref_raster as rr
import ref_scene as rs
import ref_scene_light as rl
import ref_scene_shadow as rsh
from ossid_code_amd import _lib, render, scenes

pytestmark = pytest.mark.gpu

HW = (48, 64)
CAM_K = rs.rc.cam_matrix(60.0, 60.0, 31.5, 23.5)
F32 = np.float32
BETA = (1.5, 1.5)


def _same(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, name
    g, w = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)
    print("%-12s %s differing bytes %d" % (name, got.shape, int((g != w).sum())))
    assert np.array_equal(g, w), name


def _atlas():
    sv, sf = rr.icosphere(1)                               # 80 small triangles: the one-lane path, two rows of the work list
    cv, cf = rs.cube(0.05)
    rng = np.random.default_rng(3)
    col = lambda V: rng.integers(60, 256, (len(V), 3)).astype(np.uint8)
    return scenes.MeshAtlas({1: render.Mesh(0.06 * sv, sf, colors=col(sv)), 2: render.Mesh(cv, cf, colors=col(cv))})


def _ref_meshes(atlas):
    return [tuple(atlas.mesh_arrays(o)) for o in atlas.obj_ids]


def _two_lights(S):
    rows = np.zeros((S, 4, 8), F32)
    rows[:, 0] = (-0.3, -0.5, -1.0, 0, 0.45, 0.40, 0.35, 0)                  # directional, from above left of the camera
    rows[:, 1] = (0.25, -0.5, -0.3, 1, 0.30, 0.32, 0.36, 0)                  # a point light beside the camera
    return scenes.Lights(rows, np.full(S, 2, np.int32), np.full((S, 3), 0.3, F32))


@pytest.fixture(scope="module")
def setup(hiplib):
    atlas = _atlas()
    rng = np.random.default_rng(7)
    layout = scenes.sample_layouts(atlas, 2, 3, CAM_K, HW, rng, z_range=(0.4, 0.6))
    material = np.stack([rng.uniform(0.0, 0.3, layout.n_instances), rng.integers(3, 8, layout.n_instances)], 1).astype(F32)
    L = _two_lights(2)
    unlit = scenes.render_scenes(atlas, layout, HW)
    lit = scenes.render_scenes(atlas, layout, HW, lights=L, material=material)
    torch.cuda.synchronize()
    return atlas, layout, L, material, unlit, lit


def _restate(atlas, layout, L, material, batch, size, views, enable, items, meshes=None, z_near_l=rsh.Z_NEAR_L, boxes=None):
    """The restatement of the maps and of the shadowed pass over a device render's albedo, instance and face."""
    meshes = _ref_meshes(atlas) if meshes is None else meshes
    smap = rsh.shadow_maps(meshes, layout.instance_mesh, layout.transforms, layout.scene_first, L.lights, views, items, size, z_near_l,
                           boxes=boxes)
    albedo = (batch.color if batch.albedo is None else batch.albedo).cpu().numpy()
    out = rsh.light(meshes, rl.mesh_normals(_ref_meshes(atlas)), layout.instance_mesh, layout.transforms, layout.scene_first,
                    layout.cams, HW, albedo, batch.instance.cpu().numpy(), batch.face.cpu().numpy(), L.lights, L.n_lights,
                    L.ambient, material, smap, views, enable, size, np.tile(np.asarray(BETA, F32), (layout.n_scenes, 1)),
                    z_near_l=z_near_l)
    return smap, out


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).cuda()


def _raw_maps(desc, S, lights, views, items, size, fill=0xA5, n=None, z_near_l=rsh.Z_NEAR_L, null=()):
    """ossid_scene_shadow_maps itself, the map between guard words -> (status, map uint32 [S,4,Hs,Ws] as left there)."""
    guarded.ready()
    Hs, Ws = size
    d_l, d_v, d_i = _dev(lights, F32), _dev(views, F32), _dev(np.asarray(items).reshape(-1, 3), np.int32)
    g = guarded.Guarded(S * 4 * max(Hs, 1) * max(Ws, 1) * 4, fill)
    ptr = lambda name, p: None if name in null else p
    rc = _lib.fn("ossid_scene_shadow_maps")(ptr("desc", ctypes.byref(desc)), ptr("lights", d_l.data_ptr()),
                                            ptr("views", d_v.data_ptr()), ptr("items", d_i.data_ptr() if d_i.numel() else None),
                                            len(d_i) if n is None else n, Hs, Ws, z_near_l, ptr("map", g.ptr), _lib.stream())
    guarded.sync()
    assert g.intact(), "the guard words around shadow_map were overwritten"
    return rc, g.view(torch.int32).cpu().numpy().view(np.uint32).reshape(S, 4, max(Hs, 1), max(Ws, 1))


def _raw_pass(desc, atlas, layout, L, material, batch, smap, views, enable, size, fill=0xA5, z_near_l=rsh.Z_NEAR_L, null=()):
    """ossid_scene_light_shadowed itself, blocked between guard words -> (status, lit, normal, blocked)."""
    guarded.ready()
    S, (H, W), (Hs, Ws) = layout.n_scenes, HW, size
    albedo = batch.color if batch.albedo is None else batch.albedo
    d_l, d_n, d_a, d_m = _dev(L.lights, F32), _dev(L.n_lights, np.int32), _dev(L.ambient, F32), _dev(material, F32)
    d_map, d_v, d_e = _dev(np.asarray(smap).view(np.int32), np.int32), _dev(views, F32), _dev(enable, np.int32)
    d_b = _dev(np.tile(np.asarray(BETA, F32), (S, 1)), F32)
    lit = torch.full((S, H, W, 3), fill, dtype=torch.uint8, device="cuda")
    nrm = torch.full((S, H, W, 3), -7.5, dtype=torch.float32, device="cuda")
    g = guarded.Guarded(S * H * W, fill)
    ptr = lambda name, p: None if name in null else p
    rc = _lib.fn("ossid_scene_light_shadowed")(
        ptr("desc", ctypes.byref(desc)), atlas.normals.data_ptr(), albedo.data_ptr(), batch.instance.data_ptr(), batch.face.data_ptr(),
        d_l.data_ptr(), d_n.data_ptr(), d_a.data_ptr(), d_m.data_ptr(), ptr("map", d_map.data_ptr()), ptr("views", d_v.data_ptr()),
        ptr("enable", d_e.data_ptr()), Hs, Ws, z_near_l, ptr("params", d_b.data_ptr()), lit.data_ptr(), nrm.data_ptr(), g.ptr,
        _lib.stream())
    guarded.sync()
    assert g.intact(), "the guard words around blocked were overwritten"
    return rc, lit.cpu().numpy(), nrm.cpu().numpy(), g.payload.cpu().numpy().reshape(S, H, W)


# ---- the maps and the pass, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(32, 32), (33, 47)], ids=["32x32", "33x47"])
def test_maps_and_shadowed_pass_bit_equal_to_the_restatement(setup, size):
    atlas, layout, L, material, unlit, lit = setup
    sh = scenes.Shadows(size=size, beta=BETA)
    views, enable, items, z_near_l = scenes.shadow_views(atlas, layout, L, sh)
    assert enable[:, :2].all() and not enable[:, 2:].any() and z_near_l == rsh.Z_NEAR_L
    batch = scenes.render_scenes(atlas, layout, HW, lights=L, material=material, shadows=sh)
    again = scenes.render_scenes(atlas, layout, HW, lights=L, material=material, shadows=sh)
    torch.cuda.synchronize()
    boxes = []
    smap, want = _restate(atlas, layout, L, material, batch, size, views, enable, items, boxes=boxes)
    got_map = batch.shadow_map.map.cpu().numpy().view(np.uint32)
    _same(got_map, smap, "shadow_map")
    _same(batch.color.cpu().numpy(), want["lit"], "lit")
    _same(batch.normal.cpu().numpy(), want["normal"], "normal")
    _same(batch.blocked.cpu().numpy(), want["blocked"], "blocked")
    # both paths of the triangle stage are on the maps, counted from the restatement's clipped boxes: the table's triangles
    # have more than 64 samples in theirs and go to the whole wave, every covering triangle of the icosphere has at most 64
    # and is walked by its lane; and the shadows are there
    table, sphere = atlas.index_of[scenes.TABLE_OBJ_ID], atlas.index_of[1]
    wave = [n for m, n in boxes if n > 64]
    print("covering triangles: %d walked by the wave (largest box %d), %d by one lane" % (len(wave), max(wave), len(boxes) - len(wave)))
    assert sum(m == table and n > 64 for m, n in boxes) >= 8                  # two triangles under each of four lights
    assert sum(m == sphere for m, n in boxes) >= 50 and all(n <= 64 for m, n in boxes if m == sphere)
    drawn = (smap[:, :2] != rsh.ZFAR).mean()
    print("map samples drawn %.2f, blocked pixels %d, largest k %d" % (drawn, (want["blocked"] > 0).sum(), want["blocked"].max()))
    assert drawn > 0.5 and (want["blocked"] > 0).sum() >= 20 and (smap[:, 2:] == rsh.ZFAR).all()
    assert np.array_equal(want["shaded"], batch.instance.cpu().numpy() >= 0)
    # a second run gives the same bits
    for name in ("color", "normal", "blocked"):
        assert torch.equal(getattr(again, name).view(torch.uint8), getattr(batch, name).view(torch.uint8)), name
    assert torch.equal(again.shadow_map.map, batch.shadow_map.map)
    # nothing else depends on the shadows
    assert torch.equal(batch.albedo, unlit.color)
    for name in ("depth_clean", "depth", "depth_u16", "instance", "amodal", "gt_info", "face", "facing", "keep"):
        assert torch.equal(getattr(batch, name), getattr(unlit, name)), name
    # the entries themselves with shadow_map and blocked between guard words, prefilled with 0xFF and with 0x7F: the
    # guards stay intact and the results are those of the generous buffers above
    desc, _keep = scenes._lit_desc(atlas, layout, HW, 0.0, 0.05)
    for fill in (0xFF, 0x7F):
        rc, raw_map = _raw_maps(desc, 2, L.lights, views, items, size, fill=fill)
        assert rc == 0
        _same(raw_map, got_map, "guarded map %#x" % fill)
        rc, raw_lit, raw_nrm, raw_blocked = _raw_pass(desc, atlas, layout, L, material, unlit, raw_map, views, enable, size, fill=fill)
        assert rc == 0
        _same(raw_lit, want["lit"], "guarded lit")
        _same(raw_nrm, want["normal"], "guarded normal")
        _same(raw_blocked, want["blocked"], "guarded blocked")
    # light_scenes over maps drawn beforehand is the same pass
    maps = scenes.shadow_maps(atlas, layout, HW, L, sh)
    lit3, nrm3, blocked3 = scenes.light_scenes(atlas, layout, HW, unlit.color, unlit.instance, unlit.face, L, material, shadows=maps)
    assert torch.equal(maps.map, batch.shadow_map.map) and torch.equal(lit3, batch.color) and torch.equal(blocked3, batch.blocked)
    assert torch.equal(nrm3.view(torch.int32), batch.normal.view(torch.int32))


def test_lights_that_cast_nothing_leave_the_unshadowed_pass(setup):
    """Scene 0's only light is a point light at the centre of the objects' sphere, scene 1 has no light at all: enable is
    all 0 and lit and normal are ossid_scene_light's, byte for byte."""
    atlas, layout, _L, material, _unlit, _lit = setup
    objs = [i for i in range(layout.scene_first[0], layout.scene_first[1]) if layout.instance_mesh[i] != layout.table_mesh]
    rows = np.zeros((2, 4, 8), F32)
    rows[0, 0] = tuple(layout.transforms[objs, :3, 3].mean(0)) + (1, 0.5, 0.5, 0.5, 0)
    rows[1, 0] = (0, 0, -1, 0, 9, 9, 9, 0)                                   # beyond n_lights = 0: not read
    L = scenes.Lights(rows, np.array([1, 0], np.int32), np.full((2, 3), 0.4, F32))
    sh = scenes.Shadows(size=(32, 32))
    assert not scenes.shadow_views(atlas, layout, L, sh)[1].any()
    plain = scenes.render_scenes(atlas, layout, HW, lights=L, material=material)
    batch = scenes.render_scenes(atlas, layout, HW, lights=L, material=material, shadows=sh)
    torch.cuda.synchronize()
    assert torch.equal(batch.color, plain.color) and torch.equal(batch.normal.view(torch.int32), plain.normal.view(torch.int32))
    assert not bool(batch.blocked.any()) and bool((batch.shadow_map.map == int(rsh.ZFAR)).all())
    assert bool((plain.color != plain.albedo).any())
    # and so does a pass whose lights would cast, with enable zeroed by hand
    L2 = _two_lights(2)
    views, enable, items, _z = scenes.shadow_views(atlas, layout, L2, sh)
    desc, _keep = scenes._lit_desc(atlas, layout, HW, 0.0, 0.05)
    rc, smap = _raw_maps(desc, 2, L2.lights, views, items, (32, 32))
    plain2 = scenes.render_scenes(atlas, layout, HW, lights=L2, material=material)
    rc2, lit, nrm, blocked = _raw_pass(desc, atlas, layout, L2, material, plain2, smap, views, np.zeros_like(enable), (32, 32))
    assert rc == 0 and rc2 == 0 and not blocked.any()
    _same(lit, plain2.color.cpu().numpy(), "lit, enable 0")
    _same(nrm, plain2.normal.cpu().numpy(), "normal, enable 0")


# ---- an occluder ----------------------------------------------------------------------------------------------------------------------
def _occluder_scene(atlas):
    """The table tilted by 55 degrees, a cube 0.2 m above its centre, one directional light along the table's normal."""
    T0 = rr.pose_at((0.0, 0.1, 1.0), (1.0, 0.0, 0.0), 55.0)
    n = T0[:3, :3] @ np.array([0.0, 0.0, -1.0])
    T1 = rr.pose_at(T0[:3, 3] + 0.2 * n, (1.0, 0.0, 0.0), 55.0)
    T0[:3, :3] *= 0.5
    table = atlas.index_of[scenes.TABLE_OBJ_ID]
    layout = scenes.Layout([table, atlas.index_of[2]], np.stack([T0, T1]), [0, 2], [(150.0, 150.0, 31.5, 23.5)], table_mesh=table)
    rows = np.zeros((1, 4, 8), F32)
    rows[0, 0] = tuple(n) + (0, 0.6, 0.6, 0.6, 0)
    return layout, scenes.Lights(rows, np.array([1], np.int32), np.full((1, 3), 0.3, F32))


def test_an_occluder_darkens_the_table_under_it_and_nothing_else(hiplib):
    atlas = _atlas()
    layout, L = _occluder_scene(atlas)
    material = np.zeros((2, 2), F32)
    size = (64, 64)
    sh = scenes.Shadows(size=size, beta=BETA)
    plain = scenes.render_scenes(atlas, layout, HW, lights=L, material=material)
    batch = scenes.render_scenes(atlas, layout, HW, lights=L, material=material, shadows=sh)
    torch.cuda.synchronize()
    views, enable, items, _z = scenes.shadow_views(atlas, layout, L, sh)
    _smap, want = _restate(atlas, layout, L, material, batch, size, views, enable, items)
    on_table = batch.instance.cpu().numpy() == 0
    count = int(((want["blocked"] > 0) & on_table).sum())
    print("table pixels the restatement blocks: %d (all nine taps: %d)" % (count, ((want["blocked"] == 9) & on_table).sum()))
    assert count >= 50                                       # the test cannot pass on an empty shadow
    blocked = batch.blocked.cpu().numpy()
    _same(blocked, want["blocked"], "blocked")
    _same(batch.color.cpu().numpy(), want["lit"], "lit")
    dark, base = batch.color.cpu().numpy().astype(np.int32), plain.color.cpu().numpy().astype(np.int32)
    hit = blocked > 0
    assert (dark[hit] <= base[hit]).all() and (dark[hit & on_table].sum(-1) < base[hit & on_table].sum(-1)).all()
    assert np.array_equal(dark[~hit], base[~hit])
    assert torch.equal(batch.normal.view(torch.int32), plain.normal.view(torch.int32))


# ---- device data that leads outside the arrays --------------------------------------------------------------------------------------
def test_rows_and_faces_that_lead_outside_are_skipped(setup):
    atlas, layout, L, _material, _unlit, _lit = setup
    size = (33, 47)
    views, enable, items, _z = scenes.shadow_views(atlas, layout, L, scenes.Shadows(size=size))
    desc, _keep = scenes._lit_desc(atlas, layout, HW, 0.0, 0.05)
    rc, clean = _raw_maps(desc, 2, L.lights, views, items, size)
    assert rc == 0
    meshes = _ref_meshes(atlas)
    _same(clean, rsh.shadow_maps(meshes, layout.instance_mesh, layout.transforms, layout.scene_first, L.lights, views, items, size), "clean")
    i0, i1 = int(layout.scene_first[1]) - 1, int(layout.scene_first[1])       # the last instance of scene 0, the first of scene 1
    nf = lambda i: int(atlas.table_host[layout.instance_mesh[i], 3])
    I = layout.n_instances
    bad = [(4, i0, 0), (0, i1, 0),                                           # an instance of the other scene (slot 4 of scene 0 is slot 0 of scene 1)
           (8, i1, 0), (9, i0, 0), (2 ** 31 - 1, i1, 0), (-1, i0, 0), (-2 ** 31, i0, 0),      # a slot >= 4 of the last scene, and past every scene
           (0, I, 0), (0, -1, 0), (5, 2 ** 31 - 1, 0), (5, -2 ** 31, 0),     # an instance outside the draw list
           (0, i0, nf(i0)), (0, i0, 64 * ((nf(i0) + 63) // 64)), (5, i1, 2 ** 31 - 64), (5, i1, -64), (5, i1, -2 ** 31)]   # a first face past the mesh
    mixed = np.concatenate([np.asarray(bad[:5], np.int32), items, np.asarray(bad[5:], np.int32)])
    rc, got = _raw_maps(desc, 2, L.lights, views, mixed, size)
    assert rc == 0
    _same(got, clean, "bad rows")
    # a face row of the cube with an index == nv, one of the sphere with a negative one: those faces are skipped, the others drawn
    faces = atlas.faces_host.copy()
    f_cube, f_sphere = int(atlas.table_host[atlas.index_of[2], 2]), int(atlas.table_host[atlas.index_of[1], 2])
    faces[f_cube + 3, 1] = int(atlas.table_host[atlas.index_of[2], 1])
    faces[f_sphere + 70, 2] = -1
    d_faces = _dev(faces, np.int32)
    desc.faces = d_faces.data_ptr()
    rc, got = _raw_maps(desc, 2, L.lights, views, items, size)
    desc.faces = atlas.faces.data_ptr()
    assert rc == 0
    broken = [(V, faces[f0:f0 + n], C) for (V, _F, C), (_v0, _nv, f0, n) in zip(meshes, atlas.table_host)]
    _same(got, rsh.shadow_maps(broken, layout.instance_mesh, layout.transforms, layout.scene_first, L.lights, views, items, size),
          "bad face rows")
    assert (got != clean).any()                              # the skipped faces did draw before


def test_a_triangle_across_the_lights_near_plane_casts_nothing(hiplib):
    """One cube seen from a hand-made pinhole view whose eye sits inside it, 0.02 m in front of its centre: the four far
    vertices are usable, the four near ones are not. The map holds the far face's two triangles and nothing else."""
    atlas = _atlas()
    cube = atlas.index_of[2]
    layout = scenes.Layout([cube], [rr.pose_at((0.0, 0.0, 0.6), (0.0, 0.0, 1.0), 0.0)], [0, 1], [(60.0, 60.0, 31.5, 23.5)])
    rows = np.zeros((1, 4, 8), F32)
    rows[0, 0] = (0, 0, 0.58, 1, 1, 1, 1, 0)
    views = np.zeros((1, 4, 16), F32)
    views[0, 0] = (1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, -0.58, 10, 10, 16, 16)
    items = np.array([[0, 0, 0]], np.int32)
    desc, _keep = scenes._lit_desc(atlas, layout, HW, 0.0, 0.05)
    rc, got = _raw_maps(desc, 1, rows, views, items, (32, 32))
    assert rc == 0
    V, F, C = atlas.mesh_arrays(2)
    meshes = _ref_meshes(atlas)
    _same(got, rsh.shadow_maps(meshes, layout.instance_mesh, layout.transforms, layout.scene_first, rows, views, items, (32, 32)), "map")
    far = [f for f in F if (V[f, 2] > 0).all()]
    assert len(far) == 2 and sum(((V[f, 2] > 0).any() and not (V[f, 2] > 0).all()) for f in F) == 8
    only = list(meshes)
    only[cube] = (V, np.asarray(far), C)
    want = rsh.shadow_maps(only, layout.instance_mesh, layout.transforms, layout.scene_first, rows, views, items, (32, 32))
    _same(got, want, "the far face alone")
    hit = got[0, 0] != rsh.ZFAR
    assert 150 <= hit.sum() <= 230                           # (2 * 0.05 / 0.07 * 10)^2 = 204 samples
    assert (np.abs(got[0, 0][hit].view(F32).astype(np.float64) - 0.07) < 1e-6).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(setup):
    atlas, layout, L, material, unlit, _lit = setup
    size = (32, 32)
    views, enable, items, _z = scenes.shadow_views(atlas, layout, L, scenes.Shadows(size=size))
    desc, _keep = scenes._lit_desc(atlas, layout, HW, 0.0, 0.05)
    cases = [dict(null=("desc",)), dict(null=("lights",)), dict(null=("views",)), dict(null=("items",)), dict(null=("map",)),
             dict(size=(0, 32)), dict(size=(32, 4097)), dict(size=(4097, 32)), dict(size=(32, 0)), dict(n=-1),
             dict(z_near_l=0.0), dict(z_near_l=float("nan"))]
    for kw in cases:
        args = dict(size=size, fill=0x5B)
        args.update(kw)
        rc, left = _raw_maps(desc, 2, L.lights, views, items, **args)
        assert rc == _lib.EINVAL, kw
        assert (left.view(np.uint8) == 0x5B).all(), kw                       # nothing was launched: not even the clear
    bad = _lib.SceneDesc(S=2, H=HW[0], W=HW[1], K=1, Vt=1)                    # what ossid_scene_light refuses of a descriptor
    assert _raw_maps(bad, 2, L.lights, views, items, size)[0] == _lib.EINVAL
    rc, smap = _raw_maps(desc, 2, L.lights, views, items, size)
    assert rc == 0
    for kw in (dict(null=("desc",)), dict(null=("map",)), dict(null=("views",)), dict(null=("enable",)), dict(null=("params",)),
               dict(size=(0, 32)), dict(size=(32, 4097)), dict(z_near_l=-1.0)):
        args = dict(size=size, fill=0x5B)
        args.update(kw)
        rc, lit, _nrm, blocked = _raw_pass(desc, atlas, layout, L, material, unlit, smap, views, enable, **args)
        assert rc == _lib.EINVAL and (lit == 0x5B).all() and (blocked == 0x5B).all(), kw
    # n = 0 is legal and clears the map
    rc, empty = _raw_maps(desc, 2, L.lights, views, np.zeros((0, 3), np.int32), size)
    assert rc == 0 and (empty == rsh.ZFAR).all()


# ---- the unshadowed path ----------------------------------------------------------------------------------------------------------
def test_without_shadows_the_lit_path_is_the_one_it_was(setup, monkeypatch):
    """render_scenes(lights=L) makes the calls and the bytes it made before the shadows: the recorder sees the render, the
    sensor, gt-info and ossid_scene_light and no shadow entry; with shadows the last call alone gives way to two."""
    atlas, layout, L, material, unlit, lit = setup
    calls = []
    real = _lib.fn

    def recording(name):
        f = real(name)

        def call(*args):
            calls.append(name)
            return f(*args)
        return call
    monkeypatch.setattr(_lib, "fn", recording)
    plain = scenes.render_scenes(atlas, layout, HW, lights=L, material=material)
    seq_plain, calls[:] = [c for c in calls if not c.endswith("_workspace_bytes") and c != "ossid_scene_work_items"], []
    scenes.render_scenes(atlas, layout, HW)
    seq_unlit, calls[:] = [c for c in calls if not c.endswith("_workspace_bytes") and c != "ossid_scene_work_items"], []
    shadowed = scenes.render_scenes(atlas, layout, HW, lights=L, material=material, shadows=scenes.Shadows(size=(32, 32)))
    seq_shadowed = [c for c in calls if not c.endswith("_workspace_bytes") and c != "ossid_scene_work_items"]
    monkeypatch.undo()
    torch.cuda.synchronize()
    print(seq_plain, seq_shadowed)
    assert seq_plain == seq_unlit + ["ossid_scene_light"] and not [c for c in seq_plain if "shadow" in c]
    assert seq_shadowed == seq_unlit + ["ossid_scene_shadow_maps", "ossid_scene_light_shadowed"]
    assert plain.blocked is None and plain.shadow_map is None and shadowed.blocked is not None
    # the bytes: those of the fixture's lit render and of ref_scene_light's restatement, which knows no shadows
    assert torch.equal(plain.color, lit.color) and torch.equal(plain.normal.view(torch.int32), lit.normal.view(torch.int32))
    want = rl.light(_ref_meshes(atlas), rl.mesh_normals(_ref_meshes(atlas)), layout.instance_mesh, layout.transforms,
                    layout.scene_first, layout.cams, HW, unlit.color.cpu().numpy(), unlit.instance.cpu().numpy(),
                    unlit.face.cpu().numpy(), L.lights, L.n_lights, L.ambient, material, 0.0, 0.05)
    _same(plain.color.cpu().numpy(), want["lit"], "unshadowed lit")
    _same(plain.normal.cpu().numpy(), want["normal"], "unshadowed normal")
