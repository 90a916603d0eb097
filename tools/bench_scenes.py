"""Times the scene renderer (csrc/scene.hip, SPEC.md section 13) against the route that exists without it, in one call and
alternating, on the same seeded layout -> profiles/scenes.json:

  scene      scenes.render_scenes: every instance of every scene in one draw list (7 launches);
  composite  one render.render_color per instance, then a torch composite by (depth, instance) into the scene's frame, the
             instance's coverage as its amodal mask and the pixel counts -- entry points that predate scene.hip only.

The workload is 32 scenes of 480 x 640 with 12 instances each: a table and 11 objects drawn from four ellipsoids of a
level-6 icosphere (81 920 faces each; no BOP model ships with the repository). Outputs are checked equal first: colour,
depth, instance, face, the amodal masks and the amodal / visible pixel counts. Times are HIP events around one call of
each route, median of `--rounds` alternating rounds after `--warmup`. Launches: the C ABI's own are counted from the
calls made; torch's are counted as dispatched device operations (each is at least one kernel).

--textured draws the same four ellipsoids from a texture each instead (spherical UVs, a seeded 1024 x 1024 image, no
vertex colours; the table stays vertex-coloured): `scene` is then ossid_scene_render_textured and `composite` renders
every object by ossid_raster_textured; the mip level is compared as well -> profiles/scenes_textured.json.

--lights times the light instead (csrc/scene_light.hip, SPEC 13.10-13.11) on the same workload, the same way -- HIP events,
alternating rounds in one call -> profiles/scenes_lit.json: `render` is the unlit scenes.render_scenes, `pass` the
shading pass alone over the images a render left (scenes.light_scenes, one launch), `lit` render_scenes(lights=...),
the two together; and the one-off build of the atlas's vertex normals (three launches per mesh), cold and warm. The lit
image is checked against the pass over the unlit render, and neutral lights against the albedo, first.

--lights --shadows times the cast shadows (csrc/scene_shadow.hip, SPEC 13.13-13.15) beside the lit legs, in alternation
-> profiles/scenes_shadow.json: `lit` and `pass` as above, `maps` the shadow-map pass (scenes.shadow_maps: the host's
views and work list, two launches), `shadowed_pass` the shadowed pass over maps drawn beforehand (one launch), `shadowed`
render_scenes(lights=..., shadows=...). First the shadowed image is checked: the two routes agree, enable = 0 gives
the unshadowed pass, and so does every pixel no tap blocks.

--rest times the placement (csrc/scene_rest.hip, SPEC 13.16-13.18) beside the render of the same run -> profiles/
scenes_rest.json: `support` the one-off support pass of one mesh (scenes.mesh_support at the 2562 directions of level 4:
upload, one launch, read-back) and `resting_table` the host's descent on its heights, per mesh; `drop`
scenes.scene_drop over every scene of a rest layout (upload, one launch, read-back), per refresh; `render` and
`render_free` scenes.render_scenes of the rest layout (z_range --rest_z, 0.8 to 1.6 m: nearer, a table in view has no room
for 11 such objects and sample_layouts says so) and of the free layout of the same seed. The drop is first checked
against the layout's own.

    python3 tools/bench_scenes.py [--textured | --lights [--shadows] | --rest] [--out profiles/scenes.json] [--scenes 32] [--objects 11] [--level 6]
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/bench_scenes.py --trace       (three untimed calls of `scene`;
                                                                          with --lights: of the lit render, normals first)
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_raster as rr   # noqa: E402
import ref_raster_color as rc   # noqa: E402
from ossid_code_amd import render, scenes, synth  # noqa: E402

HW = (480, 640)
AXES = ((0.06, 0.06, 0.06), (0.09, 0.05, 0.04), (0.04, 0.08, 0.06), (0.05, 0.05, 0.10))
TEXTURE_SIDE = 1024


class CountOps(TorchDispatchMode):
    """Counts the dispatched operations that touch a device tensor (views and metadata-only ops excluded)."""
    SKIP = ("view", "reshape", "select", "slice", "expand", "unsqueeze", "squeeze", "alias", "detach", "empty", "as_strided", "_unsafe_view", "permute", "t.")

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.__name__
        if not any(name.startswith(s) for s in self.SKIP):
            self.n += 1
        return func(*args, **(kwargs or {}))


def composite_route(meshes, atlas, layout, T_dev, cams_dev, counter=None):
    """-> dict of device tensors; counter["c_abi"] gets the number of kernel launches the C ABI made."""
    H, W = HW
    S, I = layout.n_scenes, layout.n_instances
    color = torch.zeros(S, H, W, 3, dtype=torch.uint8, device="cuda")
    depth = torch.zeros(S, H, W, dtype=torch.float32, device="cuda")
    inst = torch.full((S, H, W), -1, dtype=torch.int32, device="cuda")
    face = torch.full((S, H, W), -1, dtype=torch.int32, device="cuda")
    amodal = torch.empty(I, H, W, dtype=torch.bool, device="cuda")
    lod = torch.full((S, H, W), -1, dtype=torch.int32, device="cuda") if atlas.mips is not None else None
    for s in range(S):
        for i in range(int(layout.scene_first[s]), int(layout.scene_first[s + 1])):
            mesh = meshes[atlas.obj_ids[layout.instance_mesh[i]]]
            textured = bool(atlas.textured[layout.instance_mesh[i]])
            c, d, f, *l = render.render_color(mesh, T_dev[i], None, HW, pixel_offset=0.0, z_near=0.05,
                                              intrinsics=cams_dev[s:s + 1], return_face_id=True, return_lod=textured)
            if counter is not None:
                counter["c_abi"] += 3
            torch.gt(d, 0, out=amodal[i])
            take = amodal[i] & ((inst[s] < 0) | (d < depth[s]))
            color[s] = torch.where(take[..., None], c, color[s])
            depth[s] = torch.where(take, d, depth[s])
            face[s] = torch.where(take, f, face[s])
            inst[s].masked_fill_(take, i)
            if lod is not None:
                lod[s] = torch.where(take, l[0] if textured else -1, lod[s])
    px_all = amodal.sum((1, 2), dtype=torch.int32)
    px_visib = torch.bincount((inst.reshape(-1) + 1).long(), minlength=I + 1)[1:].to(torch.int32)
    return {"color": color, "depth": depth, "instance": inst, "face": face, "amodal": amodal, "px_all": px_all,
            "px_visib": px_visib, "lod": lod}


def unpack_device(words, W):
    bits = (words[..., None] >> torch.arange(32, device=words.device, dtype=torch.int32)) & 1
    return bits.reshape(words.shape[0], words.shape[1], -1)[..., :W].bool()


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return {"ms": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def bench_lit(a, atlas, layout, sensor, n_faces):
    """The legs of --lights -> the result dict."""
    H, W = HW
    lights, material = scenes.sample_lights(layout, np.random.default_rng(np.random.SeedSequence(a.seed, spawn_key=(0,))))

    def build_normals():
        atlas._normals = None
        return atlas.normals
    cold_ms, normals = once_ms(build_normals)
    warm = [once_ms(build_normals)[0] for _ in range(max(a.rounds, 3))]
    render_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor)  # noqa: E731
    lit_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor, lights=lights, material=material)  # noqa: E731
    unlit = render_fn()
    pass_fn = lambda: scenes.light_scenes(atlas, layout, HW, unlit.color, unlit.instance, unlit.face, lights, material)  # noqa: E731
    batch, (lit, normal) = lit_fn(), pass_fn()
    neutral = scenes.light_scenes(atlas, layout, HW, unlit.color, unlit.instance, unlit.face, scenes.Lights.neutral(a.scenes), material)[0]
    same = {"albedo": torch.equal(batch.albedo, unlit.color), "lit": torch.equal(batch.color, lit),
            "normal": torch.equal(batch.normal.view(torch.int32), normal.view(torch.int32)),
            "neutral_is_albedo": torch.equal(neutral, unlit.color),
            "geometry": all(torch.equal(getattr(batch, n), getattr(unlit, n)) for n in ("depth_clean", "depth_u16", "instance", "face", "gt_info"))}
    print("outputs equal:", same, flush=True)
    if not all(same.values()):
        raise SystemExit("the lit and the unlit route disagree: %s" % same)
    drawn = float((unlit.instance >= 0).float().mean())
    changed = float((batch.color != batch.albedo).any(-1).float().mean())
    del batch, lit, normal, neutral
    for _ in range(a.warmup):
        render_fn(), pass_fn(), lit_fn()
    torch.cuda.synchronize()
    t = {"render": [], "pass": [], "lit": []}
    for _ in range(a.rounds):
        for name, fn in (("render", render_fn), ("pass", pass_fn), ("lit", lit_fn)):
            t[name].append(once_ms(fn)[0])
    npix = a.scenes * H * W
    res = {"workload": {"scenes": a.scenes, "instances": layout.n_instances, "instances_per_scene": a.objects + 1, "frame": list(HW),
                        "faces_per_object": n_faces, "seed": a.seed, "drawn_pixel_fraction": drawn, "changed_pixel_fraction": changed,
                        "lights_per_scene": [int(v) for v in lights.n_lights]},
           "outputs_equal": same,
           "render": dict(stats(t["render"]), c_abi_launches=7),
           "pass": dict(stats(t["pass"]), c_abi_launches=1,
                        # albedo, instance, face in; lit and the normal image out
                        bytes_moved=int(npix * (3 + 4 + 4 + 3 + 12))),
           "lit": dict(stats(t["lit"]), c_abi_launches=8),
           "vertex_normals": {"cold_ms": float(cold_ms), "warm": stats(warm), "meshes": atlas.n_meshes,
                              "vertices": int(len(atlas.vertices_host)), "faces": int(len(atlas.faces_host)),
                              "c_abi_launches": 3 * atlas.n_meshes},
           "rounds": a.rounds, "warmup": a.warmup}
    res["ratio_pass_over_render"] = res["pass"]["ms"] / res["render"]["ms"]
    res["ratio_lit_over_render"] = res["lit"]["ms"] / res["render"]["ms"]
    return res


def bench_shadowed(a, atlas, layout, sensor, n_faces):
    """The legs of --lights --shadows -> the result dict: the lit render, the shading pass, the shadow-map pass
    (scenes.shadow_maps: the host's views and work list, their uploads, two launches), the shadowed pass over maps drawn
    beforehand (one launch) and the lit, shadowed render, timed in alternation."""
    H, W = HW
    lights, material = scenes.sample_lights(layout, np.random.default_rng(np.random.SeedSequence(a.seed, spawn_key=(0,))))
    sh = scenes.Shadows() if a.shadow_size is None else scenes.Shadows(size=tuple(a.shadow_size))
    atlas.normals
    unlit = scenes.render_scenes(atlas, layout, HW, sensor=sensor)
    maps = scenes.shadow_maps(atlas, layout, HW, lights, sh)
    lit_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor, lights=lights, material=material)  # noqa: E731
    shadowed_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor, lights=lights, material=material, shadows=sh)  # noqa: E731
    pass_fn = lambda: scenes.light_scenes(atlas, layout, HW, unlit.color, unlit.instance, unlit.face, lights, material)  # noqa: E731
    maps_fn = lambda: scenes.shadow_maps(atlas, layout, HW, lights, sh)  # noqa: E731
    spass_fn = lambda: scenes.light_scenes(atlas, layout, HW, unlit.color, unlit.instance, unlit.face, lights, material, shadows=maps)  # noqa: E731
    lit, batch = lit_fn(), shadowed_fn()
    s_lit, s_normal, s_blocked = spass_fn()
    off = scenes.ShadowMaps(maps.map, maps.views, torch.zeros_like(maps.enable), maps.params, maps.size, maps.z_near_l, maps.n_items)
    o_lit, o_normal, o_blocked = scenes.light_scenes(atlas, layout, HW, unlit.color, unlit.instance, unlit.face, lights, material, shadows=off)
    free = batch.blocked == 0
    same = {"maps": torch.equal(batch.shadow_map.map, maps.map), "lit": torch.equal(batch.color, s_lit),
            "blocked": torch.equal(batch.blocked, s_blocked),
            "normal": torch.equal(batch.normal.view(torch.int32), lit.normal.view(torch.int32)),
            "enable_0_is_the_unshadowed_pass": torch.equal(o_lit, lit.color) and not bool(o_blocked.any()),
            "unblocked_pixels_are_the_unshadowed_pass": torch.equal(batch.color[free], lit.color[free]),
            "geometry": all(torch.equal(getattr(batch, n), getattr(unlit, n)) for n in ("depth_clean", "depth_u16", "instance", "face", "gt_info"))}
    print("outputs equal:", same, flush=True)
    if not all(same.values()):
        raise SystemExit("the shadowed and the unshadowed route disagree: %s" % same)
    drawn = unlit.instance >= 0
    # what acne would look like: pixels with a blocked tap and no pixel a light blocks whole (nine taps) within four pixels
    # of them -- stray taps away from any shadow --, on the table and on the objects
    whole = torch.nn.functional.max_pool2d((batch.blocked >= 9).float()[:, None], 9, 1, 4)[:, 0] > 0
    stray = (batch.blocked > 0) & ~whole
    is_table = torch.from_numpy(layout.instance_mesh == layout.table_mesh).to(drawn.device)[unlit.instance.clamp(min=0).long()] & drawn
    frac = lambda m: float((stray & m).sum()) / max(1, int(m.sum()))  # noqa: E731
    workload = {"stray_blocked_fraction_of_table_pixels": frac(is_table), "stray_blocked_fraction_of_object_pixels": frac(drawn & ~is_table),
                "blocked_fraction_of_table_pixels": float(((batch.blocked > 0) & is_table).sum()) / max(1, int(is_table.sum())),
                "blocked_fraction_of_object_pixels": float(((batch.blocked > 0) & drawn & ~is_table).sum()) / max(1, int((drawn & ~is_table).sum())),
                "table_pixel_fraction": float(is_table.float().mean())}
    workload.update({"scenes": a.scenes, "instances": layout.n_instances, "instances_per_scene": a.objects + 1, "frame": list(HW),
                "faces_per_object": n_faces, "seed": a.seed, "lights_per_scene": [int(v) for v in lights.n_lights],
                "shadow_map": list(maps.size), "beta": list(sh.beta), "lights_enabled": int(maps.enable.sum()),
                "work_list_rows": int(maps.n_items), "drawn_pixel_fraction": float(drawn.float().mean()),
                "blocked_pixel_fraction": float((batch.blocked > 0).float().mean()),
                "fully_blocked_by_a_light_fraction": float((batch.blocked >= 9).float().mean()),
                "map_samples_drawn_fraction_of_enabled": float((maps.map != 0x7F800000).float().sum() / max(1, int(maps.enable.sum()) * maps.size[0] * maps.size[1]))})
    del lit, batch, s_lit, s_normal, s_blocked, o_lit, o_normal, o_blocked
    legs = (("lit", lit_fn), ("shadowed", shadowed_fn), ("pass", pass_fn), ("maps", maps_fn), ("shadowed_pass", spass_fn))
    for _ in range(a.warmup):
        for _name, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _fn in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(once_ms(fn)[0])
    res = {"workload": workload, "outputs_equal": same,
           "lit": dict(stats(t["lit"]), c_abi_launches=8), "shadowed": dict(stats(t["shadowed"]), c_abi_launches=10),
           "pass": dict(stats(t["pass"]), c_abi_launches=1), "maps": dict(stats(t["maps"]), c_abi_launches=2),
           "shadowed_pass": dict(stats(t["shadowed_pass"]), c_abi_launches=1), "rounds": a.rounds, "warmup": a.warmup}
    res["added_ms_shadowed_pass_over_pass"] = res["shadowed_pass"]["ms"] - res["pass"]["ms"]
    res["added_ms_shadowed_over_lit"] = res["shadowed"]["ms"] - res["lit"]["ms"]
    # the yardstick of the issue: one more scene render per enabled light, scaled by the map's share of the frame's pixels
    per_light = res["lit"]["ms"] / a.scenes * (maps.size[0] * maps.size[1]) / float(H * W)
    res["one_render_per_light_scaled_ms"] = per_light * workload["lights_enabled"]
    return res


def bench_rest(a, atlas, free_layout, sensor, n_faces):
    """The legs of --rest -> the result dict."""
    import time
    objects = [o for o in atlas.obj_ids if o != scenes.TABLE_OBJ_ID]
    dirs = render._icosphere_vertices(a.rest_level)
    rows = {o: atlas.table_host[atlas.index_of[o]] for o in objects}
    support_fn = lambda o: scenes.mesh_support(atlas.vertices[rows[o][0]:rows[o][0] + rows[o][1]], dirs)  # noqa: E731
    cold_ms, h0 = once_ms(lambda: support_fn(objects[0]))
    t_sup = [once_ms(lambda: support_fn(o))[0] for _ in range(max(a.rounds, 3)) for o in objects]
    t0 = time.perf_counter()
    table = scenes.resting_table(dirs, h0, scenes.surface_centroid(*atlas.mesh_arrays(objects[0])[:2]))
    table_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    layout = scenes.sample_layouts(atlas, a.scenes, a.objects, synth.CAM_K, HW, np.random.default_rng(a.seed), placement="rest",
                                   rest_level=a.rest_level, z_range=tuple(a.rest_z))
    first_layout_ms = (time.perf_counter() - t0) * 1e3     # with the support pass and the table of every object
    t_host = []
    for k in range(3):
        t0 = time.perf_counter()
        scenes.sample_layouts(atlas, a.scenes, a.objects, synth.CAM_K, HW, np.random.default_rng(a.seed + 1 + k), placement="rest",
                              rest_level=a.rest_level, z_range=tuple(a.rest_z))
        t_host.append((time.perf_counter() - t0) * 1e3)
    obj = layout.instance_mesh != layout.table_mesh
    counts = [int(obj[layout.scene_first[s]:layout.scene_first[s + 1]].sum()) for s in range(a.scenes)]
    first = np.concatenate([[0], np.cumsum(counts)])
    G, cell = layout.grid
    drop_fn = lambda: scenes.scene_drop(atlas, layout.instance_mesh[obj], first, layout.local[obj], G, cell)  # noqa: E731
    d, s = drop_fn()
    same = {"drop": bool(np.array_equal(d, layout.drop[obj])), "status": bool(np.array_equal(s, layout.status[obj])),
            "status_all_0": bool((layout.status == 0).all())}
    print("outputs equal:", same, flush=True)
    if not all(same.values()):
        raise SystemExit("the drop does not repeat the layout's own: %s" % same)
    render_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor)  # noqa: E731
    free_fn = lambda: scenes.render_scenes(atlas, free_layout, HW, sensor=sensor)  # noqa: E731
    g = render_fn().gt_info.cpu().numpy()
    legs = (("drop", drop_fn), ("render", render_fn), ("render_free", free_fn))
    for _ in range(a.warmup):
        for _name, fn in legs:
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _fn in legs}
    for _ in range(a.rounds):
        for name, fn in legs:
            t[name].append(once_ms(fn)[0])
    res = {"workload": {"scenes": a.scenes, "instances": layout.n_instances, "instances_per_scene": a.objects + 1, "frame": list(HW),
                        "faces_per_object": n_faces, "faces_dropped": int(atlas.table_host[layout.instance_mesh[obj], 3].sum()),
                        "seed": a.seed, "z_range": list(a.rest_z), "rest_level": a.rest_level, "directions": int(len(dirs)), "grid": int(G), "cell_m": float(cell),
                        "stacked_objects": int((layout.drop[obj] > 1e-9 + np.array(
                            [-(layout.local[i][2, :3] @ atlas.mesh_arrays(atlas.obj_ids[layout.instance_mesh[i]])[0].astype(np.float64).T).min()
                             for i in np.nonzero(obj)[0]])).sum()),
                        "resting_orientations_of_first_object": int(len(table.fixed)),
                        "visible_instances": int((g[:, 1] > 0).sum()), "objects_in_frame": int((g[obj, 0] > 0).sum())},
           "outputs_equal": same,
           "support": dict(stats(t_sup), cold_ms=float(cold_ms), c_abi_launches=1, per="mesh, once"),
           "resting_table": {"host_ms": float(table_ms), "per": "mesh, once"},
           "drop": dict(stats(t["drop"]), c_abi_launches=1, per="refresh"),
           "render": dict(stats(t["render"]), c_abi_launches=7), "render_free": dict(stats(t["render_free"]), c_abi_launches=7),
           "sample_layouts_rest_host_ms": {"first": float(first_layout_ms), "later": stats(t_host)},
           "rounds": a.rounds, "warmup": a.warmup}
    res["ratio_drop_over_render"] = res["drop"]["ms"] / res["render"]["ms"]
    return res


def finish(a, res):
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    res.update(commit=commit, box={"gpu": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip})
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/scenes.json, or profiles/scenes_textured.json with --textured")
    ap.add_argument("--textured", action="store_true", help="draw the objects from a 1024 x 1024 texture each")
    ap.add_argument("--lights", action="store_true", help="time the shading pass and the vertex normals -> profiles/scenes_lit.json")
    ap.add_argument("--shadows", action="store_true", help="with --lights: time the shadow maps and the shadowed pass -> profiles/scenes_shadow.json")
    ap.add_argument("--rest", action="store_true", help="time the support pass and the drop beside the render -> profiles/scenes_rest.json")
    ap.add_argument("--rest_level", type=int, default=4, help="icosphere level of the resting directions (4: 2562)")
    ap.add_argument("--rest_z", type=float, nargs=2, default=(0.8, 1.6),
                    help="z_range of the rest layout: a table holds 11 objects of 8 to 20 cm inside the frame from about 0.7 m on")
    ap.add_argument("--shadow_size", type=int, nargs=2, default=None, help="Hs Ws of the shadow maps (default: scenes.Shadows' own)")
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--objects", type=int, default=11, help="objects per scene; the table is one more instance")
    ap.add_argument("--level", type=int, default=6, help="icosphere level of the objects (6: 81 920 faces)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--trace", action="store_true", help="three untimed calls of the scene route, for a kernel trace")
    a = ap.parse_args()
    if a.lights and a.textured:
        raise SystemExit("--lights times the pass over the vertex-coloured workload; it does not combine with --textured")
    if a.shadows and not a.lights:
        raise SystemExit("--shadows needs --lights: shadows are cast by lights")
    if a.rest and (a.lights or a.textured or a.trace):
        raise SystemExit("--rest times the placement on the vertex-coloured workload; it does not combine with other modes")
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "scenes_rest.json" if a.rest else "scenes_shadow.json" if a.shadows else "scenes_lit.json" if a.lights else ("scenes_textured.json" if a.textured else "scenes.json"))
    if not torch.cuda.is_available():
        raise SystemExit("bench_scenes.py needs the GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    V, F = rr.icosphere(a.level)
    if a.textured:
        trng = np.random.default_rng(a.seed + 1)
        n = V / np.sqrt((V * V).sum(1, keepdims=True))
        uvs = np.stack([np.arctan2(n[:, 1], n[:, 0]) / (2.0 * np.pi) + 0.5, np.arccos(np.clip(n[:, 2], -1.0, 1.0)) / np.pi], 1)
        meshes = {k + 1: render.Mesh(V * np.asarray(ax), F, uvs=uvs,
                                     texture=trng.integers(0, 256, (TEXTURE_SIDE, TEXTURE_SIDE, 3)).astype(np.uint8))
                  for k, ax in enumerate(AXES)}
    else:
        meshes = {k + 1: render.Mesh(V * np.asarray(ax), F, colors=rc.axis_colors(V * np.asarray(ax))[0])
                  for k, ax in enumerate(AXES)}
    atlas = scenes.MeshAtlas(meshes)
    tv, tf, tc = atlas.mesh_arrays(scenes.TABLE_OBJ_ID)
    meshes[scenes.TABLE_OBJ_ID] = render.Mesh(tv, tf, colors=tc)           # the composite route draws the table too
    rng = np.random.default_rng(a.seed)
    layout = scenes.sample_layouts(atlas, a.scenes, a.objects, synth.CAM_K, HW, rng)
    sensor = scenes.sample_sensor(a.scenes, HW, rng)
    scene_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor)  # noqa: E731
    if a.trace:
        if a.lights:                                       # the normals' three launches per mesh, then the eight of a lit render
            lights, material = scenes.sample_lights(layout, np.random.default_rng(np.random.SeedSequence(a.seed, spawn_key=(0,))))
            sh = scenes.Shadows() if a.shadows else None
            scene_fn = lambda: scenes.render_scenes(atlas, layout, HW, sensor=sensor, lights=lights, material=material, shadows=sh)  # noqa: E731
        for _ in range(3):
            scene_fn()
        torch.cuda.synchronize()
        return
    if a.rest:
        return finish(a, bench_rest(a, atlas, layout, sensor, int(len(F))))
    if a.shadows:
        return finish(a, bench_shadowed(a, atlas, layout, sensor, int(len(F))))
    if a.lights:
        return finish(a, bench_lit(a, atlas, layout, sensor, int(len(F))))
    T_dev = torch.from_numpy(layout.transforms.astype(np.float32)).cuda()
    cams_dev = torch.from_numpy(layout.cams).cuda()
    comp_fn = lambda: composite_route(meshes, atlas, layout, T_dev, cams_dev)  # noqa: E731

    # the two routes agree, bit for bit
    batch, comp = scene_fn(), comp_fn()
    same = {"color": torch.equal(batch.color, comp["color"]),
            "depth": torch.equal(batch.depth_clean.view(torch.int32), comp["depth"].view(torch.int32)),
            "instance": torch.equal(batch.instance, comp["instance"]), "face": torch.equal(batch.face, comp["face"]),
            "amodal": torch.equal(unpack_device(batch.amodal, HW[1]), comp["amodal"]),
            "px_count_all": torch.equal(batch.gt_info[:, 0], comp["px_all"]),
            "px_count_visib": torch.equal(batch.gt_info[:, 1], comp["px_visib"])}
    if a.textured:
        same["lod"] = torch.equal(batch.lod, comp["lod"])
    print("outputs equal:", same, flush=True)
    if not all(same.values()):
        raise SystemExit("the routes disagree: %s" % same)
    g = batch.gt_info.cpu().numpy()
    counter = {"c_abi": 0}
    with CountOps() as ops:
        composite_route(meshes, atlas, layout, T_dev, cams_dev, counter)
    comp_ops = ops.n
    with CountOps() as ops:
        scene_fn()
    scene_ops = ops.n
    ws_comp = max(m._ws_color.numel() for m in meshes.values() if m._ws_color is not None)
    del batch, comp
    for _ in range(a.warmup):
        scene_fn(), comp_fn()
    torch.cuda.synchronize()
    t_scene, t_comp = [], []
    for _ in range(a.rounds):
        t_scene.append(once_ms(scene_fn)[0])
        t_comp.append(once_ms(comp_fn)[0])
    batch = scene_fn()
    H, W = HW
    I = layout.n_instances
    res = {
        "workload": {"textured": a.textured, "texture": [TEXTURE_SIDE, TEXTURE_SIDE] if a.textured else None,
                     "scenes": a.scenes, "instances": I, "instances_per_scene": a.objects + 1, "frame": list(HW),
                     "faces_per_object": int(len(F)), "faces_drawn": int(atlas.table_host[layout.instance_mesh, 3].sum()),
                     "seed": a.seed, "visible_instances": int((g[:, 1] > 0).sum()),
                     "mean_visib_fract": float(np.mean(g[:, 1][g[:, 0] > 0] / g[:, 0][g[:, 0] > 0]))},
        "outputs_equal": same,
        "scene": {"ms": float(np.median(t_scene)), "ms_min": float(min(t_scene)), "ms_max": float(max(t_scene)),
                  "c_abi_launches": 7, "torch_device_ops": scene_ops, "workspace_bytes": int(batch.workspace_bytes),
                  "amodal_bytes": int(batch.amodal.numel() * 4), "frames_touched": a.scenes},
        "composite": {"ms": float(np.median(t_comp)), "ms_min": float(min(t_comp)), "ms_max": float(max(t_comp)),
                      "c_abi_launches": counter["c_abi"], "torch_device_ops": comp_ops, "workspace_bytes": int(ws_comp),
                      "amodal_bytes": int(I * H * W), "frames_touched": I},
        "rounds": a.rounds, "warmup": a.warmup}
    res["ratio_composite_over_scene"] = res["composite"]["ms"] / res["scene"]["ms"]
    finish(a, res)


if __name__ == "__main__":
    main()
