"""csrc/scene.hip through scenes.render_scenes against the restatement tests/ref_scene.py (SPEC.md section 13) on the
issue's fixture: bit equality of every output -- colour, depth, instance, face, facing, the amodal bits, gt-info, the
16-bit and f32 sensor depth and `keep` --, the defining property against this build's own render_color per instance,
and byte-identical repeats. No tolerance and no pixel left out."""
import numpy as np
import pytest
import torch

import ref_scene as rs
from ossid_code_amd import render, scenes

pytestmark = pytest.mark.gpu

H, W = rs.HW


@pytest.fixture(scope="module")
def setup(hiplib):
    fx = rs.fixture()
    meshes = {o: render.Mesh(V, F, colors=C) for o, (V, F, C) in fx["meshes"].items()}
    atlas = scenes.MeshAtlas(meshes)
    layout = scenes.Layout([atlas.index_of[int(o)] for o in fx["instance_obj"]], fx["transforms"], fx["scene_first"], fx["cams"])
    sensor = scenes.Sensor(fx["thresholds"], fx["n_rects"], fx["rects"])
    return meshes, atlas, layout, sensor


def _outputs(batch):
    torch.cuda.synchronize()
    names = ("color", "depth_clean", "depth", "depth_u16", "instance", "amodal", "gt_info", "face", "facing", "keep")
    return {n: getattr(batch, n).cpu().numpy() for n in names}


def _same(got, ref, fine=False):
    tag = "_fine" if fine else ""
    pairs = (("depth_clean", ref["depth"]), ("instance", ref["instance"]), ("face", ref["face"]), ("color", ref["color"]),
             ("facing", ref["facing"]), ("keep", ref["keep" + tag].astype(np.uint8)), ("depth_u16", ref["u16" + tag]),
             ("depth", ref["sensor" + tag]), ("gt_info", ref["gt_info" + tag]))
    for name, want in pairs:
        g = got[name]
        print("%-12s %s %s differing %d" % (name, g.dtype, g.shape, int((g != want).sum())))
        assert g.dtype == want.dtype and g.shape == want.shape, name
        assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g,
                              want.view(np.uint32) if want.dtype == np.float32 else want), name
    words = got["amodal"].view(np.uint32)
    assert np.array_equal(words, rs.pack_amodal(ref["amodal"]))                    # the tail word's spare bits included
    assert np.array_equal(scenes.unpack_amodal(got["amodal"], W), ref["amodal"])


def test_bit_equal_to_the_restatement(setup):
    _meshes, atlas, layout, sensor = setup
    ref = rs.reference()
    g = ref["gt_info"]                     # the fixture still exercises the cases (test_scene.py holds the full list)
    assert g[0, 0] == H * W and g[2, :2].tolist() == [150, 0] and g[5, :2].tolist() == [16, 0] and not g[6, :3].any()
    _same(_outputs(scenes.render_scenes(atlas, layout, rs.HW, sensor=sensor)), ref)


def test_clean_sensor_and_a_depth_past_16_bits(setup):
    _meshes, atlas, layout, _sensor = setup
    got = _outputs(scenes.render_scenes(atlas, layout, rs.HW, depth_scale=0.01))
    _same(got, rs.reference(), fine=True)
    assert got["keep"].all() and ((got["depth_clean"] > 0.7) & (got["depth_u16"] == 0)).any()


def test_background_shows_where_nothing_is_drawn(setup):
    _meshes, atlas, layout, sensor = setup
    ref = rs.reference()
    bg = np.random.default_rng(5).integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    for b in (bg, bg[1]):                                                          # one per scene, one for all
        got = scenes.render_scenes(atlas, layout, rs.HW, background=b, sensor=sensor).color.cpu().numpy()
        want = np.where((ref["instance"] < 0)[..., None], b.reshape(-1, H, W, 3), ref["color"])
        assert np.array_equal(got, want) and (ref["instance"] < 0).any()


def _composite(meshes, atlas, layout, hw):
    """The defining property's right-hand side on the device's own renders: per pixel the winner by (bits(z), instance)
    among what render_color makes of each instance alone under the scene's camera -> (color, depth, instance, face,
    covered bool [I,H,W])."""
    S, (H, W) = layout.n_scenes, hw
    color = torch.zeros(S, H, W, 3, dtype=torch.uint8, device="cuda")
    depth = torch.zeros(S, H, W, dtype=torch.float32, device="cuda")
    inst = torch.full((S, H, W), -1, dtype=torch.int32, device="cuda")
    face = torch.full((S, H, W), -1, dtype=torch.int32, device="cuda")
    covered = torch.zeros(layout.n_instances, H, W, dtype=torch.bool, device="cuda")
    for s in range(S):
        for i in range(int(layout.scene_first[s]), int(layout.scene_first[s + 1])):
            mesh = meshes[atlas.obj_ids[layout.instance_mesh[i]]]
            c, d, f = render.render_color(mesh, layout.transforms[i], layout.cam_K(s), hw, pixel_offset=0.0, z_near=0.05,
                                          return_face_id=True)
            covered[i] = d > 0
            take = covered[i] & ((inst[s] < 0) | (d < depth[s]))
            color[s][take], depth[s][take], face[s][take] = c[take], d[take], f[take]
            inst[s][take] = i
    return color, depth, inst, face, covered


def _same_as_composite(batch, meshes, atlas, layout, hw):
    color, depth, inst, face, covered = _composite(meshes, atlas, layout, hw)
    assert torch.equal(batch.depth_clean.view(torch.int32), depth.view(torch.int32))
    assert torch.equal(batch.instance, inst) and torch.equal(batch.face, face) and torch.equal(batch.color, color)
    # an instance's amodal mask is what it covers alone
    assert np.array_equal(scenes.unpack_amodal(batch.amodal, hw[1]), covered.cpu().numpy())
    return inst, covered


def test_equals_the_composite_of_render_color_per_instance(setup):
    meshes, atlas, layout, _sensor = setup
    _same_as_composite(scenes.render_scenes(atlas, layout, rs.HW), meshes, atlas, layout, rs.HW)


def test_larger_frame_many_workgroups_and_every_group_size(hiplib):
    """120 x 300 (the mask rows end in a 12-bit tail word, the gt-info of an instance spans five workgroups) with a mesh of
    5120 faces (64 triangles per group), one of 320 (5 per group), a cube and the atlas's table (one triangle per group,
    split over eight waves; large boxes whose tile rows straddle mask words): the scene equals the composite of render_color
    per instance, and gt-info equals plain numpy counts over the outputs."""
    hw = (120, 300)
    fx = rs.fixture()
    rng = np.random.default_rng(4)
    V4, F4 = rs.rr.icosphere(4)
    meshes = {1: render.Mesh(*fx["meshes"][1][:2], colors=fx["meshes"][1][2]),
              2: render.Mesh(*fx["meshes"][2][:2], colors=fx["meshes"][2][2]),
              3: render.Mesh(0.08 * V4, F4, colors=rng.integers(0, 256, (len(V4), 3)).astype(np.uint8))}
    atlas = scenes.MeshAtlas(meshes)
    tv, tf, tc = atlas.mesh_arrays(scenes.TABLE_OBJ_ID)
    meshes[scenes.TABLE_OBJ_ID] = render.Mesh(tv, tf, colors=tc)
    K = rs.rc.cam_matrix(280.0, 275.0, 151.0, 58.5)
    layout = scenes.sample_layouts(atlas, 3, 3, K, hw, rng, z_range=(0.3, 0.6))
    sensor = scenes.sample_sensor(3, hw, rng)
    batch = scenes.render_scenes(atlas, layout, hw, sensor=sensor)
    inst, covered = _same_as_composite(batch, meshes, atlas, layout, hw)
    g = batch.gt_info.cpu().numpy()
    valid = (batch.depth > 0).cpu().numpy()
    inst, covered = inst.cpu().numpy(), covered.cpu().numpy()
    want = rs.gt_info(covered, inst, np.where(valid, 1.0, 0.0), layout.scene_first)
    assert np.array_equal(g, want)
    assert (g[:, 0] > 2000).sum() >= 3 and (g[:, 1] < g[:, 0]).any()          # large masks, and some occlusion


def test_two_runs_give_identical_bytes(setup):
    _meshes, atlas, layout, sensor = setup
    a = _outputs(scenes.render_scenes(atlas, layout, rs.HW, sensor=sensor))
    b = _outputs(scenes.render_scenes(atlas, layout, rs.HW, sensor=sensor))
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name


def test_frames_carry_what_the_stream_takes(setup):
    _meshes, atlas, layout, sensor = setup
    ref = rs.reference()
    frames = list(scenes.render_scenes(atlas, layout, rs.HW, sensor=sensor).frames())
    assert len(frames) == 9 and [f["obj_id"] for f in frames] == [3, 1, 1, 2, 1, 2, 1, 1, 2]
    f = frames[3]
    assert f["img"].shape == (H, W, 3) and f["img"].dtype == np.uint8 and f["depth"].dtype == np.float32
    assert np.array_equal(f["depth"], ref["sensor"][0]) and np.array_equal(f["mask_gt"], ref["amodal"][3])
    assert np.array_equal(f["mask_gt_visib"], ref["instance"][0] == 3) and f["bbox_visib"] == tuple(ref["gt_info"][3, 7:11])
    assert f["visib_fract"] == 72 / 113 and np.array_equal(f["pose_gt"], rs.fixture()["transforms"][3])
    assert frames[8]["scene_id"] == 2 and np.array_equal(frames[8]["cam_K"], rs.rc.cam_matrix(*rs.CAM3))
