"""SPEC.md section 13 without a device: the restatement tests/ref_scene.py holds the properties the section states on the
issue's fixture, the layout and sensor sampling are deterministic and inside their ranges, a SceneBatch written as a BOP
folder reads back bit for bit (bop_eval.BopFolder and scenes.read_bop_frames), bad arguments are refused before any
device work, and the header declares the entries."""
import json
import os

import numpy as np
import pytest

import ref_scene as rs
from ossid_code_amd import bop_eval, render, scenes

H, W = rs.HW


def _atlas(device="cpu"):
    fx = rs.fixture()
    return scenes.MeshAtlas({o: render.Mesh(V, F, device=device, colors=C) for o, (V, F, C) in fx["meshes"].items()})


def _layout(atlas):
    fx = rs.fixture()
    return scenes.Layout([atlas.index_of[int(o)] for o in fx["instance_obj"]], fx["transforms"], fx["scene_first"], fx["cams"])


def _host_batch(atlas, depth_scale=1.0):
    """A SceneBatch of the restatement's arrays."""
    ref = rs.reference()
    fine = depth_scale != 1.0
    return scenes.SceneBatch(atlas, _layout(atlas), rs.HW, ref["color"], ref["depth"], ref["sensor_fine" if fine else "sensor"],
                             ref["u16_fine" if fine else "u16"], ref["instance"], rs.pack_amodal(ref["amodal"]),
                             ref["gt_info_fine" if fine else "gt_info"], depth_scale=depth_scale)


# ---- the restatement on the fixture --------------------------------------------------------------------------------------
def test_fixture_exercises_every_case():
    """The rehearsed figures of the issue's table: a fixture that stops exercising a case fails here."""
    ref = rs.reference()
    g = ref["gt_info"]
    assert g[0, :2].tolist() == [H * W, 1961] and g[0, 3:7].tolist() == [0, 0, W, H]          # the table covers the frame
    assert g[1, :2].tolist() == [150, 107]
    assert g[2, :2].tolist() == [150, 0] and g[2, 7:11].tolist() == [-1] * 4                   # the exact tie: the lower wins
    assert np.array_equal(ref["alone"][1][1], ref["alone"][2][1]) and np.array_equal(ref["amodal"][1], ref["amodal"][2])
    assert g[3, :2].tolist() == [113, 72] and 0 < g[1, 1] < g[1, 0]                            # both partly visible
    assert g[4, 3] + g[4, 5] - 1 == W - 1                                                      # cut by the right edge
    assert g[5, :2].tolist() == [16, 0] and g[5, 7:11].tolist() == [-1] * 4                    # hidden behind the table
    assert g[6].tolist() == [0, 0, 0] + [-1] * 8 + [0]                                         # behind the camera
    assert (ref["instance"][1] == -1).all() and not ref["depth"][1].any()                      # the empty scene
    assert g[7, 1] > 0 and g[8, 1] > 0
    assert not (rs.pack_amodal(ref["amodal"])[:, :, 1] >> np.uint32(W - 32)).any()             # tail bits past W stay 0


def test_a_scene_pixel_is_the_winner_among_the_instances_alone():
    ref, fx = rs.reference(), rs.fixture()
    first = fx["scene_first"]
    for s in range(3):
        best = np.zeros((H, W), np.float32)
        who = np.full((H, W), -1)
        for i in range(first[s], first[s + 1]):
            d = ref["alone"][i][1]
            better = (d > 0) & ((who < 0) | (d < best))
            best[better], who[better] = d[better], i
        assert np.array_equal(who, ref["instance"][s]) and np.array_equal(best, ref["depth"][s])
        for i in range(first[s], first[s + 1]):
            m = who == i
            assert np.array_equal(ref["color"][s][m], ref["alone"][i][0][m])
            assert np.array_equal(ref["face"][s][m], ref["alone"][i][2][m])
            assert not (m & ~ref["amodal"][i]).any()               # visible is a subset of amodal
    f = ref["facing"]
    assert f.dtype == np.float32 and (f[ref["instance"] < 0] == 0).all() and f.max() <= 1.0 and f[ref["instance"] >= 0].min() > 0


def test_sensor_rule_on_the_fixture():
    ref, fx = rs.reference(), rs.fixture()
    keep, u16, dep = ref["keep"], ref["u16"], ref["sensor"]
    low = ref["facing"][0] < np.float32(0.2)
    assert low.any() and not keep[0][low].any()
    assert not keep[0, 5:12, 3:20].any() and not keep[0, 30:, 40:].any() and not keep[0, 39].any()      # clipped at the border
    assert keep[0, 10, 25:40].all()                                                                      # the zero-area one
    assert keep[1].all() and not u16[1].any()                                                            # threshold 0, no depth
    assert np.array_equal(keep[2], ref["facing"][2] >= np.float32(0.5)) and 0 < keep[2].sum() < H * W
    assert (u16[~keep] == 0).all() and np.array_equal(dep, (u16.astype(np.float64) * 0.001).astype(np.float32))
    assert np.array_equal(u16[keep], np.rint(ref["depth"][keep].astype(np.float64) * 1000.0).astype(np.uint16))
    # the clean sensor at 0.01 mm per count: everything is kept, and what lies beyond 0.65535 m does not fit 16 bits
    far = ref["depth"] * np.float64(1e5) > 65535.5
    assert ref["keep_fine"].all() and far.any() and not ref["u16_fine"][far].any() and ref["u16_fine"].max() > 40000
    assert ref["gt_info_fine"][0, 2] < ref["gt_info_fine"][0, 0] and ref["gt_info_fine"][7, 2] == ref["gt_info_fine"][7, 0]


# ---- sampling ---------------------------------------------------------------------------------------------------------------
def test_layouts_are_deterministic_and_inside_their_ranges():
    atlas = _atlas()
    K = rs.rc.cam_matrix(572.4, 573.6, 325.3, 242.0)
    a = scenes.sample_layouts(atlas, 5, 3, K, (480, 640), np.random.default_rng(7))
    b = scenes.sample_layouts(atlas, 5, 3, K, (480, 640), np.random.default_rng(7))
    c = scenes.sample_layouts(atlas, 5, 3, K, (480, 640), np.random.default_rng(8))
    for name in ("instance_mesh", "transforms", "scene_first", "cams"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert not np.array_equal(a.transforms, c.transforms)
    assert a.scene_first.tolist() == [0, 4, 8, 12, 16, 20] and a.cams.dtype == np.float32
    table = atlas.index_of[scenes.TABLE_OBJ_ID]
    for s in range(5):
        mine = slice(a.scene_first[s], a.scene_first[s + 1])
        assert a.instance_mesh[mine][0] == table and sorted(a.instance_mesh[mine][1:]) == [0, 1, 2]     # distinct objects
        corners = (a.transforms[mine][0] @ np.array([[-1, -1, 0, 1], [1, -1, 0, 1], [1, 1, 0, 1], [-1, 1, 0, 1.0]]).T).T
        assert corners[:, 2].min() >= 1.2 + max(atlas.radius(o) for o in (1, 2, 3)) - 1e-9            # behind every object
        for T in a.transforms[mine][1:]:
            R, t = T[:3, :3], T[:3, 3]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0
            u, v = 572.4 * t[0] / t[2] + 325.3, 573.6 * t[1] / t[2] + 242.0
            assert 0.5 <= t[2] <= 1.2 and -1e-3 <= u <= 640 + 1e-3 and -1e-3 <= v <= 480 + 1e-3
    bare = scenes.sample_layouts(atlas, 2, 5, K, (480, 640), np.random.default_rng(7), table=False)     # more than the atlas has
    assert bare.scene_first.tolist() == [0, 5, 10] and table not in bare.instance_mesh
    assert scenes.sample_layouts(atlas, 2, 0, K, (480, 640), np.random.default_rng(7), table=False).n_instances == 0


def test_sensor_samples_follow_the_reference_distributions():
    a = scenes.sample_sensor(64, (480, 640), np.random.default_rng(3))
    b = scenes.sample_sensor(64, (480, 640), np.random.default_rng(3))
    assert np.array_equal(a.thresholds, b.thresholds) and np.array_equal(a.n_rects, b.n_rects) and np.array_equal(a.rects, b.rects)
    assert a.thresholds.dtype == np.float32 and a.thresholds.min() >= 0.2 and a.thresholds.max() <= 0.5
    assert set(a.n_rects.tolist()) == set(range(7))
    for s in range(64):
        for k in range(6):
            r0, r1, c0, c1 = a.rects[s, k]
            if k >= a.n_rects[s]:
                assert (a.rects[s, k] == 0).all()
                continue
            assert 0 <= r0 < 480 and 0 <= c0 < 640 and r1 <= 479 and c1 <= 639
            assert r1 - r0 < 120 and c1 - c0 < 160 and (r1 == 479 or r1 - r0 >= 30) and (c1 == 639 or c1 - c0 >= 40)


# ---- the BOP folder ----------------------------------------------------------------------------------------------------------
def _diameters(atlas):
    out = {}
    for o in (1, 2, 3):
        V = atlas.mesh_arrays(o)[0].astype(np.float64)
        out[o] = float(np.sqrt(((V[:, None] - V[None]) ** 2).sum(-1).max()))
    return out


@pytest.mark.parametrize("depth_scale", [1.0, 0.01])
def test_bop_folder_round_trip(hiplib, tmp_path, depth_scale):
    atlas = _atlas()
    batch = _host_batch(atlas, depth_scale)
    with pytest.raises(ValueError, match="depth_scale"):
        batch.write_bop(str(tmp_path), "synth", depth_scale=depth_scale * 2)
    batch.write_bop(str(tmp_path), "synth", depth_scale=depth_scale, diameters=_diameters(atlas))
    mine, back = list(batch.frames()), list(scenes.read_bop_frames(str(tmp_path), "synth"))
    assert len(mine) == len(back) == 9 and [f["scene_id"] for f in mine] == [0] * 7 + [2] * 2
    for a, b in zip(mine, back):
        assert sorted(a) == sorted(b)
        for k in ("img", "depth", "mask_gt", "mask_gt_visib", "cam_K"):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        for k in ("obj_id", "bbox_visib", "visib_fract", "scene_id", "im_id"):
            assert a[k] == b[k], k
        assert np.array_equal(a["pose_gt"][:3, :3], b["pose_gt"][:3, :3]) and np.abs(a["pose_gt"] - b["pose_gt"]).max() < 1e-15
    ref = rs.reference()
    assert np.array_equal(mine[3]["mask_gt"], ref["amodal"][3]) and mine[3]["visib_fract"] == 72 / 113
    assert mine[2]["bbox_visib"] == (-1, -1, -1, -1) and mine[6]["visib_fract"] == 0.0
    # ... and what the evaluator reads: millimetres
    folder = bop_eval.BopFolder(str(tmp_path), "synth")
    depth_mm, K = folder.frame(0, 0)
    want = ref["u16_fine" if depth_scale != 1.0 else "u16"][0].astype(np.float64) * depth_scale
    assert np.array_equal(depth_mm, want.astype(np.float32)) and np.array_equal(K, batch.layout.cam_K(0))
    assert folder.targets == [{"scene_id": 0, "im_id": 0, "obj_id": 1, "inst_count": 4},
                              {"scene_id": 0, "im_id": 0, "obj_id": 2, "inst_count": 2},
                              {"scene_id": 0, "im_id": 0, "obj_id": 3, "inst_count": 1},
                              {"scene_id": 2, "im_id": 0, "obj_id": 1, "inst_count": 1},
                              {"scene_id": 2, "im_id": 0, "obj_id": 2, "inst_count": 1}]
    T = folder.gt_pose(2, 0, 2)
    assert np.allclose(T[:3, 3], rs.fixture()["transforms"][8][:3, 3] * 1000.0, rtol=0, atol=1e-9)
    V, F = folder.mesh(1)
    assert np.array_equal(V, atlas.mesh_arrays(1)[0].astype(np.float64) * 1000.0) and np.array_equal(F, atlas.mesh_arrays(1)[1])
    info = folder.model_info(2)
    assert abs(info["diameter"] - 120.0) < 1e-3 and abs(info["size_x"] - 120.0) < 2.0 and info["min_z"] < 0
    with open(os.path.join(str(tmp_path), "synth", "test", "000000", "scene_gt_info.json")) as f:
        gi = json.load(f)["0"]
    assert gi[0] == {"bbox_obj": [0, 0, W, H], "bbox_visib": [0, 0, W, H], "px_count_all": H * W,
                     "px_count_valid": int(batch.gt_info[0, 2]), "px_count_visib": 1961, "visib_fract": 1961 / (H * W)}
    assert os.path.isdir(os.path.join(str(tmp_path), "synth", "test", "000001", "rgb")) and not \
        os.listdir(os.path.join(str(tmp_path), "synth", "test", "000001", "mask"))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_device_work(hiplib):
    atlas = _atlas()
    lay = _layout(atlas)
    fx = rs.fixture()
    with pytest.raises(ValueError, match="object ids"):
        scenes.MeshAtlas({0: render.Mesh(*fx["meshes"][1][:2], device="cpu", colors=fx["meshes"][1][2])})
    with pytest.raises(ValueError, match="vertex colours"):
        scenes.MeshAtlas({1: render.Mesh(*fx["meshes"][1][:2], device="cpu")})
    with pytest.raises(ValueError, match="scene_first"):
        scenes.Layout(lay.instance_mesh, lay.transforms, [0, 7, 6, 9], lay.cams)
    with pytest.raises(ValueError, match="at most 1024 instances"):
        scenes.Layout(np.zeros(1025, np.int32), np.tile(np.eye(4), (1025, 1, 1)), [0, 1025], lay.cams[:1])
    with pytest.raises(ValueError, match="1 to 256 scenes"):
        scenes.Layout([], np.zeros((0, 4, 4)), np.zeros(258, np.int32), np.ones((257, 4)))
    with pytest.raises(ValueError, match="n_rects"):
        scenes.Sensor(np.zeros(3), [0, 7, 0], np.zeros((3, 6, 4)))
    for kwargs, match in (({"hw": (0, 56)}, "frame"), ({"pixel_offset": 1.5}, "pixel_offset"), ({"z_near": -1.0}, "z_near"),
                          ({"depth_scale": 0.0}, "depth_scale"), ({"sensor": scenes.Sensor.clean(2)}, "sensor"),
                          ({"background": np.zeros((H, W, 3), np.float32)}, "background"),
                          ({"background": np.zeros((2, H, W, 3), np.uint8)}, "background")):
        args = {"hw": rs.HW, **kwargs}
        with pytest.raises(ValueError, match=match):
            scenes.render_scenes(atlas, lay, args.pop("hw"), **args)
    bad = scenes.Layout(lay.instance_mesh + 3, lay.transforms, lay.scene_first, lay.cams)
    with pytest.raises(ValueError, match="instance_mesh"):
        scenes.render_scenes(atlas, bad, rs.HW)
    with pytest.raises(RuntimeError, match="GPU only"):          # no fall-back: a host atlas is not rendered on the host
        scenes.render_scenes(atlas, lay, rs.HW)
    with pytest.raises(ValueError):
        scenes.sample_layouts(atlas, 0, 3, np.eye(3), rs.HW, np.random.default_rng(0))
    with pytest.raises(ValueError, match="Generator"):
        scenes.sample_sensor(2, rs.HW, 5)
    # the C side: bad scalars come back as OSSID_EINVAL before anything is launched (no device is present here)
    assert hiplib.fn("ossid_scene_workspace_bytes")(10, 0, H, W) == 0
    assert hiplib.fn("ossid_scene_workspace_bytes")(10, 3, H, W) == 16 * 10 + 8 * 3 * H * W
    assert hiplib.fn("ossid_scene_work_items")(12) == 12 * 8 and hiplib.fn("ossid_scene_work_items")(320) == 64
    assert hiplib.fn("ossid_scene_work_items")(0) == 0 and hiplib.fn("ossid_scene_work_items")(1 << 22) == 1 << 16
    assert hiplib.fn("ossid_scene_work_items")((1 << 22) + 1) == -1
    assert hiplib.fn("ossid_scene_render")(None, None, 0, None) == -22
    assert hiplib.fn("ossid_scene_gt_info")(None, None, None, None, 1, 1, H, W, None, None) == -22
    assert hiplib.fn("ossid_scene_sensor")(None, None, 1, H, W, None, None, None, 1000.0, 0.001, None, None, None, None) == -22


def test_work_offsets_are_the_prefix_sums_of_the_draw_list(hiplib):
    atlas = _atlas()
    off = scenes.work_offsets(atlas, _layout(atlas))
    items = {1: 96, 2: 64, 3: 16}
    nv = {1: 8, 2: 162, 3: 4}
    want = np.cumsum([[0, 0]] + [[items[int(o)], nv[int(o)]] for o in rs.fixture()["instance_obj"]], axis=0)
    assert off.dtype == np.int32 and np.array_equal(off, want)


def test_header_declares_the_scene_entries(hiplib):
    names = hiplib.exported_symbols()
    for must in ("ossid_scene_render", "ossid_scene_workspace_bytes", "ossid_scene_work_items", "ossid_scene_gt_info",
                 "ossid_scene_sensor"):
        assert must in names and hasattr(hiplib.lib(), must)
    assert (hiplib.SCENE_MAX_SCENES, hiplib.SCENE_MAX_INSTANCES, hiplib.SCENE_MAX_RECTS) == (256, 1024, 6)
    assert hiplib.RASTER_MAX_FACES == 1 << 22
    assert [f for f, _ in hiplib.SceneDesc._fields_][-12:] == ["Vt", "Ft", "K", "I", "S", "H", "W", "Sb", "work_items", "records",
                                                               "pixel_offset", "z_near"]
