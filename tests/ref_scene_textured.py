"""Independent numpy restatement of SPEC.md section 13 for an atlas that mixes texture-mapped and vertex-coloured meshes,
the yardstick of ossid_scene_render_textured: ref_scene.render_scenes' composite by comparisons -- the smaller f32 depth
wins and, at equal depth, the lower instance -- with each instance rendered alone by ref_raster_textured.render (colour
and level) when the atlas draws its mesh from the texture and by ref_raster_color.render otherwise. Coverage, facing,
gt-info, the sensor and the packed masks are ref_scene's own.

The fixture is ref_scene.fixture()'s geometry, draw list, cameras and sensor with other surfaces: the cube (1) has a
texture only, 37 x 50, with per-vertex UVs partly outside [0, 1]; the sphere (2) has its vertex colours and an 8 x 8
texture; the quad (3) keeps its vertex colours. The two chains differ in size, so the second starts at a texel offset
that is neither zero nor a power of two.
"""
import functools

import numpy as np

import ref_raster as rr
import ref_raster_color as rc
import ref_raster_textured as rt
import ref_scene as rs

F32 = np.float32
HW, NEAR = rs.HW, rs.NEAR


def chain_texels(Ht, Wt):
    n = Ht * Wt
    while Ht > 1 or Wt > 1:
        Ht, Wt = (Ht + 1) >> 1, (Wt + 1) >> 1
        n += Ht * Wt
    return n


def is_textured(mesh, use_texture):
    """render_color's rule: the vertex colours when the mesh has them, unless use_texture; the texture when that is all."""
    _V, _F, C, U, _I = mesh
    return U is not None and (use_texture or C is None)


@functools.lru_cache(maxsize=None)
def fixture():
    """ref_scene.fixture() with "meshes" {obj_id: (V, F, C u8 [V,3] or None, uvs f32 [V,2] or None, texture u8 [Ht,Wt,3] or
    None)}. Computed once; callers must not write into it."""
    fx = dict(rs.fixture())
    rng = np.random.default_rng(1313)
    (V1, F1, _C1), (V2, F2, C2), (V3, F3, C3) = (fx["meshes"][o] for o in (1, 2, 3))
    uv1 = rng.uniform(-0.5, 1.5, (len(V1), 2)).astype(F32)
    n = V2 / np.sqrt((V2 * V2).sum(1, keepdims=True))
    uv2 = np.stack([np.arctan2(n[:, 1], n[:, 0]) / (2.0 * np.pi) + 0.5, np.arccos(np.clip(n[:, 2], -1.0, 1.0)) / np.pi], 1)
    uv2 = uv2.astype(F32)
    tex1 = rng.integers(0, 256, (37, 50, 3)).astype(np.uint8)
    tex2 = rng.integers(0, 256, (8, 8, 3)).astype(np.uint8)
    fx["meshes"] = {1: (V1, F1, None, uv1, tex1), 2: (V2, F2, C2, uv2, tex2), 3: (V3, F3, C3, None, None)}
    return fx


@functools.lru_cache(maxsize=None)
def _levels(obj_id):
    return rt.mip_chain(fixture()["meshes"][obj_id][4])


def render_instance(mesh, levels, textured, pose, cam, hw, pixel_offset, z_near):
    """One instance alone -> (color, depth, face, lod (-1 everywhere for a vertex-coloured render), covered bool [H,W])."""
    V, F, C, U, _I = mesh
    K = rc.cam_matrix(*[float(F32(v)) for v in cam])
    if textured:
        color, depth, face, lod, _s = rt.render(V, F, U, levels, pose, K, hw, pixel_offset, z_near)
    else:
        color, depth, face, _s = rc.render(V, F, C, pose, K, hw, pixel_offset, z_near)
        lod = np.full(depth.shape, -1, np.int32)
    _d, count, _s = rr.render(V, F, pose, K, hw, pixel_offset, z_near)
    return color, depth, face, lod, count > 0


def render_scenes(meshes, levels, textured, instance_mesh, transforms, scene_first, cams, hw, pixel_offset=0.0, z_near=0.05,
                  background=None, alone=None):
    """meshes: list of (V, F, C, uvs, texture); levels: their mip chains (None without a texture); textured: bool per mesh
    -> dict as ref_scene.render_scenes returns, with lod int32 [S,H,W] (-1 = nothing drawn or a vertex-coloured winner) and
    alone = the per-instance (color, depth, face, lod). alone(i, mesh index) may supply the per-instance renders."""
    H, W = hw
    S, I = len(cams), len(instance_mesh)
    color = np.zeros((S, H, W, 3), np.uint8)
    if background is not None:
        color[:] = np.asarray(background, np.uint8).reshape(-1, H, W, 3)
    depth = np.zeros((S, H, W), F32)
    instance = np.full((S, H, W), -1, np.int32)
    face = np.full((S, H, W), -1, np.int32)
    lod = np.full((S, H, W), -1, np.int32)
    facing = np.zeros((S, H, W), F32)
    amodal = np.zeros((I, H, W), bool)
    out_alone = []
    for s in range(S):
        for i in range(int(scene_first[s]), int(scene_first[s + 1])):       # ascending: a tie stays with the lower instance
            k = int(instance_mesh[i])
            c, d, f, l, cov = alone(i, k) if alone is not None else \
                render_instance(meshes[k], levels[k], textured[k], transforms[i], cams[s], hw, pixel_offset, z_near)
            out_alone.append((c, d, f, l))
            amodal[i] = cov
            take = (d > 0) & ((instance[s] < 0) | (d < depth[s]))
            per_face = rs.face_facing(meshes[k][0], meshes[k][1], transforms[i])
            color[s][take], depth[s][take], face[s][take], lod[s][take], instance[s][take] = c[take], d[take], f[take], l[take], i
            facing[s][take] = per_face[f[take]]
    return {"color": color, "depth": depth, "instance": instance, "face": face, "lod": lod, "facing": facing, "amodal": amodal,
            "alone": out_alone}


@functools.lru_cache(maxsize=None)
def _alone(i, textured):
    """Instance i of the fixture alone, from its texture or from its colours: shared by the two atlas modes."""
    fx = fixture()
    o = int(fx["instance_obj"][i])
    s = int(np.searchsorted(fx["scene_first"], i, side="right")) - 1
    return render_instance(fx["meshes"][o], _levels(o) if textured else None, textured, fx["transforms"][i], fx["cams"][s], HW,
                           0.0, NEAR)


@functools.lru_cache(maxsize=None)
def reference(use_texture=False):
    """The restatement's outputs on the fixture (meshes in obj_id order 1, 2, 3 = atlas indices 0, 1, 2) for
    MeshAtlas(..., use_texture=use_texture), computed once per mode: the scene render with lod, and the corrupted sensor at
    depth_scale 1 with its gt-info. textured = which meshes the atlas draws from their texture; tex_table = the rows
    (first texel, Ht, Wt) the atlas must hold for them."""
    fx = fixture()
    order = sorted(fx["meshes"])
    meshes = [fx["meshes"][o] for o in order]
    textured = [is_textured(m, use_texture) for m in meshes]
    imesh = np.array([order.index(o) for o in fx["instance_obj"]], np.int32)
    out = render_scenes(meshes, None, textured, imesh, fx["transforms"], fx["scene_first"], fx["cams"], HW, 0.0, NEAR,
                        alone=lambda i, k: _alone(i, textured[k]))
    out["instance_mesh"], out["textured"] = imesh, textured
    table, t0 = np.zeros((len(meshes), 3), np.int64), 0
    for k, m in enumerate(meshes):
        if textured[k]:
            table[k] = (t0, m[4].shape[0], m[4].shape[1])
            t0 += chain_texels(m[4].shape[0], m[4].shape[1])
    out["tex_table"], out["mip_texels"] = table, t0
    out["u16"], out["sensor"], out["keep"] = rs.sensor(out["depth"], out["facing"], fx["thresholds"], fx["n_rects"], fx["rects"],
                                                       1000.0 / 1.0, 1.0 / 1000.0)
    out["gt_info"] = rs.gt_info(out["amodal"], out["instance"], out["sensor"], fx["scene_first"])
    return out
