"""SPEC.md 13.13-13.15 without a device: the restatement tests/ref_scene_shadow.py against geometry it cannot get wrong
-- a small square over a large one, lit along their common normal --, scenes.shadow_views' rule and work list, the
refusals that come before the device is touched, the pre-training set's draw order under shadows=True, and the
entries' place in the header and the build. No GPU.

test_a_square_over_a_floor_casts_its_outline checks the YARDSTICK, not the product: it runs tests/ref_scene_shadow.py
alone, so that the restatement the GPU tests hold the kernels to is itself held to something. It does not depend on the
package's shadow code; every other test here does."""
import numpy as np
import pytest

import ref_raster as rr
import ref_scene as rs
import ref_scene_light as rl
import ref_scene_shadow as rsh
from ossid_code_amd import _build, render, scenes

F32 = np.float32


# ---- the restatement against two squares ------------------------------------------------------------------------------------------
HW = (96, 128)
CAM = (120.0, 120.0, 63.5, 47.5)
SIZE = (256, 256)
HEIGHT, LIGHT_HEIGHT = 0.2, 2.0


def _two_squares(point):
    """A 0.1 m square 0.2 m above a 1 m square, both tilted by 55 degrees so that the camera sees the floor under the small
    one; one light on the squares' common normal through their centres: directional, or a point light 2 m above the floor
    -> (blocked u8 [H,W], floor mask, the floor pixels' coordinates in the floor's own frame, texel size on the floor,
    the shadow's half side)."""
    floor, small = rs.quad(0.5), rs.quad(0.05)
    meshes = [(V, F, np.full((len(V), 3), 180, np.uint8)) for V, F in (floor, small)]
    T0 = rr.pose_at((0.0, 0.1, 1.3), (1.0, 0.0, 0.0), 55.0)
    R, t = T0[:3, :3], T0[:3, 3]
    n = R @ np.array([0.0, 0.0, -1.0])                       # the squares' normal, towards the camera's side
    assert n[2] < 0
    T1 = T0.copy()
    T1[:3, 3] = t + HEIGHT * n
    transforms, imesh, first, cams = np.stack([T0, T1]), np.array([0, 1], np.int32), np.array([0, 2], np.int32), np.array([CAM], F32)
    lights = np.zeros((1, 4, 8), F32)
    lights[0, 0] = tuple(t + LIGHT_HEIGHT * n) + (1, 0.6, 0.6, 0.6, 0) if point else tuple(n) + (0, 0.6, 0.6, 0.6, 0)
    n_lights, ambient, material = np.array([1], np.int32), np.full((1, 3), 0.3, F32), np.zeros((2, 2), F32)
    radius = [float(np.sqrt((V * V).sum(1).max())) for V, _F in (floor, small)]
    views, enable, items = rsh.views(radius, [2, 2], imesh, transforms, first, -1, lights, n_lights, SIZE)
    assert enable.tolist() == [[1, 0, 0, 0]] and items.tolist() == [[0, 0, 0], [0, 1, 0]]
    img = rs.render_scenes(meshes, imesh, transforms, first, cams, HW, 0.0, 0.05)
    smap = rsh.shadow_maps(meshes, imesh, transforms, first, lights, views, items, SIZE)
    out = rsh.light(meshes, rl.mesh_normals(meshes), imesh, transforms, first, cams, HW, img["color"], img["instance"], img["face"],
                    lights, n_lights, ambient, material, smap, views, enable, SIZE, np.array([[1.5, 1.5]], F32))
    # the floor point under each pixel centre, by intersecting the pixel's ray with the floor's plane, in the floor's frame
    ys, xs = np.mgrid[0:HW[0], 0:HW[1]].astype(np.float64)
    d = np.stack([(xs - CAM[2]) / CAM[0], (ys - CAM[3]) / CAM[1], np.ones_like(xs)], -1)
    P = d * ((n @ t) / (d @ n))[..., None]
    local = (P - t) @ R                                       # R^T (P - t)
    a = float(views[0, 0, 12])
    texel = (LIGHT_HEIGHT / a) if point else 1.0 / a
    half = 0.05 * (LIGHT_HEIGHT / (LIGHT_HEIGHT - HEIGHT) if point else 1.0)
    return out["blocked"][0], img["instance"][0] == 0, local, texel, half, smap


@pytest.mark.parametrize("point", [False, True], ids=["directional", "point"])
def test_a_square_over_a_floor_casts_its_outline(point):
    blocked, floor, local, texel, half, smap = _two_squares(point)
    cheb = np.maximum(np.abs(local[..., 0]), np.abs(local[..., 1]))
    inside, outside = floor & (cheb < half - 2.0 * texel), floor & (cheb > half + 2.0 * texel)
    print("floor pixels %d, inside %d, outside %d, texel %.4f m, map samples drawn %d"
          % (floor.sum(), inside.sum(), outside.sum(), texel, (smap != rsh.ZFAR).sum()))
    assert inside.sum() >= 6 and outside.sum() > 2000 and 2.0 * texel < half
    assert (blocked[inside] == 9).all()
    assert (blocked[outside] == 0).all()
    assert blocked.max() <= 9                                # one light: nine taps
    assert (smap[0, 1:] == rsh.ZFAR).all() and (smap[0, 0] != rsh.ZFAR).any()


# ---- shadow_views ---------------------------------------------------------------------------------------------------------------
def _atlas():
    sv, sf = rr.icosphere(2)
    cv, cf = rs.cube(0.05)
    rng = np.random.default_rng(3)
    col = lambda V: rng.integers(0, 256, (len(V), 3)).astype(np.uint8)
    return scenes.MeshAtlas({1: render.Mesh(0.06 * sv, sf, device="cpu", colors=col(sv)),
                             2: render.Mesh(cv, cf, device="cpu", colors=col(cv))})


def _scene(atlas, S=3, n=3, seed=5):
    rng = np.random.default_rng(seed)
    K = rs.rc.cam_matrix(60.0, 60.0, 31.5, 23.5)
    layout = scenes.sample_layouts(atlas, S, n, K, (48, 64), rng, z_range=(0.4, 0.7))
    lights, material = scenes.sample_lights(layout, rng)
    return layout, lights, material


def test_shadow_views_are_determined_by_their_inputs_and_match_the_restatement():
    atlas = _atlas()
    layout, lights, _m = _scene(atlas)
    sh = scenes.Shadows(size=(33, 47))
    a, b = scenes.shadow_views(atlas, layout, lights, sh), scenes.shadow_views(atlas, layout, lights, sh)
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    views, enable, items, z_near_l = a
    assert views.dtype == F32 and views.shape == (3, 4, 16) and enable.dtype == np.int32 and enable.shape == (3, 4)
    assert items.dtype == np.int32 and items.shape[1] == 3 and z_near_l == 1e-3
    assert (enable[np.arange(4)[None, :] >= lights.n_lights[:, None]] == 0).all() and enable.sum() >= 3
    radius = [atlas.radius(o) for o in atlas.obj_ids]
    rv, re, ri = rsh.views(radius, atlas.table_host[:, 3], layout.instance_mesh, layout.transforms, layout.scene_first,
                           atlas.index_of[scenes.TABLE_OBJ_ID], lights.lights, lights.n_lights, (33, 47))
    assert np.array_equal(re, enable) and np.array_equal(ri, items)
    assert np.allclose(rv, views, rtol=1e-5, atol=1e-6)
    # a rotation, the eye behind the scene's centre, the principal point in the middle of the map
    for s, l in zip(*np.nonzero(enable)):
        R = views[s, l, :9].reshape(3, 3).astype(np.float64)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-5) and np.linalg.det(R) > 0.99
        assert views[s, l, 12] == views[s, l, 13] > 0 and tuple(views[s, l, 14:]) == (23.5, 16.5)


def test_a_point_light_inside_the_scenes_sphere_is_not_enabled():
    atlas = _atlas()
    layout, _l, _m = _scene(atlas, S=2)
    objs = [i for i in range(layout.scene_first[0], layout.scene_first[1]) if layout.instance_mesh[i] != layout.table_mesh]
    centres = layout.transforms[objs, :3, 3]
    c = centres.mean(0)
    r = max(np.linalg.norm(layout.transforms[i, :3, 3] - c) + atlas.radius(atlas.obj_ids[layout.instance_mesh[i]]) for i in objs)
    rows = np.zeros((2, 4, 8), F32)
    rows[0, 0] = tuple(c + np.array([0.0, 0.0, -1.05 * r])) + (1, 1, 1, 1, 0)          # inside 1.1 r
    rows[0, 1] = tuple(c + np.array([0.0, 0.0, -1.2 * r])) + (1, 1, 1, 1, 0)           # outside
    rows[0, 2] = (0, 0, 0, 0, 1, 1, 1, 0)                                              # a directional light without a direction
    rows[0, 3] = (0, -1, 0, 0, 1, 1, 1, 0)
    rows[1, 0] = (0, 0, -1, 0, 1, 1, 1, 0)                                             # beyond n_lights = 0
    L = scenes.Lights(rows, np.array([4, 0], np.int32), np.ones((2, 3), F32))
    views, enable, items, _z = scenes.shadow_views(atlas, layout, L, scenes.Shadows(size=(32, 32)))
    assert enable.tolist() == [[0, 1, 0, 1], [0, 0, 0, 0]]
    assert not views[0, 0].any() and not views[0, 2].any() and not views[1].any()
    assert set(items[:, 0].tolist()) == {1, 3}
    # a scene of a table alone enables nothing
    alone = scenes.Layout([layout.table_mesh], layout.transforms[:1], [0, 1], layout.cams[:1], table_mesh=layout.table_mesh)
    L1 = scenes.Lights(rows[:1], np.array([4], np.int32), np.ones((1, 3), F32))
    _v, e1, i1, _z = scenes.shadow_views(atlas, alone, L1, scenes.Shadows())
    assert not e1.any() and i1.shape == (0, 3)


def test_every_object_vertex_projects_inside_the_map():
    atlas = _atlas()
    layout, lights, _m = _scene(atlas, S=4, n=4, seed=11)
    for size in ((32, 32), (33, 47), (512, 512)):
        views, enable, _items, z_near_l = scenes.shadow_views(atlas, layout, lights, scenes.Shadows(size=size))
        seen = 0
        for s, l in zip(*np.nonzero(enable)):
            for i in range(layout.scene_first[s], layout.scene_first[s + 1]):
                if layout.instance_mesh[i] == layout.table_mesh:
                    continue
                V = atlas.mesh_arrays(atlas.obj_ids[layout.instance_mesh[i]])[0]
                C = rs.camera_points(V, layout.transforms[i]).astype(np.float64)
                qz, u, v, ok = rsh.project(views[s, l], bool(lights.lights[s, l, 3] != 0), [C[:, 0], C[:, 1], C[:, 2]], z_near_l)
                assert ok.all() and (u > 0).all() and (u < size[1]).all() and (v > 0).all() and (v < size[0]).all()
                seen += len(V)
        assert seen > 1000


def test_the_work_list_covers_each_enabled_light_instance_and_face_once():
    atlas = _atlas()                                         # 320, 12 and 2 faces: 5 rows, 1 and 1
    layout, lights, _m = _scene(atlas, S=3, n=3, seed=2)
    _views, enable, items, _z = scenes.shadow_views(atlas, layout, lights, scenes.Shadows(size=(32, 32)))
    nf = atlas.table_host[layout.instance_mesh, 3]
    got = sorted((int(ls), int(i), int(first) + k) for ls, i, first in items for k in range(min(64, int(nf[i]) - int(first))))
    want = sorted((4 * s + l, i, f) for s, l in zip(*np.nonzero(enable))
                  for i in range(layout.scene_first[s], layout.scene_first[s + 1]) for f in range(int(nf[i])))
    assert got == want and len(set(got)) == len(got) and len(got) > 0
    assert (items[:, 2] % 64 == 0).all() and (items[:, 2] < nf[items[:, 1]]).all()
    assert any(layout.instance_mesh[i] == layout.table_mesh for i in items[:, 1])           # the table casts too


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device(hiplib):
    atlas = _atlas()
    layout, lights, material = _scene(atlas)
    hw = (48, 64)
    good = scenes.Shadows()
    assert good.size == (512, 512) and good.beta == (1.5, 1.5)
    for kw in ({"size": (0, 32)}, {"size": (32, 4097)}, {"size": (32,)}, {"size": (32.0, 32)}, {"size": 32},
               {"beta": (np.nan, 1.0)}, {"beta": (1.0, np.inf)}, {"beta": (1.0,)}, {"beta": (1e300, 0.0)}):
        with pytest.raises(ValueError, match="Shadows"):
            scenes.Shadows(**kw)
    with pytest.raises(ValueError, match="without lights"):
        scenes.render_scenes(atlas, layout, hw, shadows=good)
    with pytest.raises(ValueError, match="scenes.Shadows"):
        scenes.render_scenes(atlas, layout, hw, lights=lights, material=material, shadows=True)
    bad = scenes.Shadows()
    bad.size = (512, 5000)                                   # changed after its own check: render_scenes checks again
    with pytest.raises(ValueError, match="size"):
        scenes.render_scenes(atlas, layout, hw, lights=lights, material=material, shadows=bad)
    bad = scenes.Shadows()
    bad.beta = (1.5, float("nan"))
    with pytest.raises(ValueError, match="beta"):
        scenes.render_scenes(atlas, layout, hw, lights=lights, material=material, shadows=bad)
    with pytest.raises(ValueError, match="beta"):
        scenes.light_scenes(atlas, layout, hw, None, None, None, lights, material, shadows=bad)
    with pytest.raises(ValueError, match="Lights"):
        scenes.shadow_views(atlas, layout, scenes.Lights.neutral(2), good)
    with pytest.raises(RuntimeError, match="GPU only"):      # everything was in order: no fall-back on the host
        scenes.render_scenes(atlas, layout, hw, lights=lights, material=material, shadows=good)
    # the C side refuses bad scalars and NULL buffers before anything is launched (no device is present here)
    assert hiplib.fn("ossid_scene_shadow_maps")(None, None, None, None, 0, 32, 32, 1e-3, None, None) == hiplib.EINVAL
    assert hiplib.fn("ossid_scene_light_shadowed")(None, *([None] * 11), 32, 32, 1e-3, None, None, None, None, None) == hiplib.EINVAL


def test_the_pretrain_sets_draws_do_not_move_under_shadows():
    import test_pretrain as tp
    from ossid_code_amd.dtoid import pretrain
    targets = np.array([[s, 4 * s + k] for s in range(4) for k in (1, 2, 3)], np.int32)
    plans = []
    for kw in ({}, {"lights": True}, {"lights": True, "shadows": True}, {"lights": True, "shadows": scenes.Shadows(size=(64, 64))}):
        st = tp._set(3, **kw)
        layout, sensor = st.draw_targets()
        plans.append((layout.transforms, layout.instance_mesh, sensor.thresholds, sensor.rects) + st.plan(layout, targets)
                     + (st.rng.integers(1 << 30),))
    for other in plans[1:]:
        for x, y in zip(plans[0], other):
            assert np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x,
                                  np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
    assert tp._set(0, lights=True, shadows=True).shadows.size == (512, 512) and tp._set(0).shadows is None
    with pytest.raises(ValueError, match="lights"):
        tp._set(0, shadows=True)
    assert pretrain.ScenePretrainSet.__init__.__defaults__[-1] is False


def test_the_header_and_the_build_hold_the_shadow_entries(hiplib):
    names = hiplib.exported_symbols()
    for must in ("ossid_scene_shadow_maps", "ossid_scene_light_shadowed"):
        assert must in names and hasattr(hiplib.lib(), must)
        assert must not in hiplib.RECORDABLE                 # ossid_scene_light is not recordable either
    assert "scene_shadow.hip" in _build.SOURCES and "ossid_scene_light" not in hiplib.RECORDABLE
    assert (scenes.SHADOW_MAX_SIDE, scenes.SHADOW_FACES, scenes.SHADOW_Z_NEAR) == (4096, 64, 1e-3)
    assert not [n for n in names if "shadow" in n and n.endswith(("_workspace_bytes", "_workspace_floats", "_partials",
                                                                   "_grid_bytes", "_pyramid_bytes"))]
