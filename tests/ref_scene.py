"""Independent numpy restatement of SPEC.md section 13 (multi-object scenes with ground truth), the yardstick of
csrc/scene.hip, built on ref_raster_color.render: every instance is rendered alone and the images are composited by
comparisons -- the smaller f32 depth wins and, at equal depth, the lower instance; no packed key is written anywhere.
Amodal coverage is ref_raster.render's sample count, facing comes from camera points computed as ref_raster.vertex_stage
computes them, gt-info is plain numpy and the sensor rule is written with slices.

Also the fixture of the issue (fixture()): the smallest scenes at which each mechanism can go wrong.
"""
import functools

import numpy as np

import ref_raster as rr
import ref_raster_color as rc

F32 = np.float32


# ---- SPEC 13.2-13.4 ---------------------------------------------------------------------------------------------------------
def camera_points(vertices, pose):
    """f32 [V,3]: X, Y, Z of SPEC 7.2 in the written order."""
    P = np.asarray(vertices, dtype=np.float64).astype(F32)
    T = np.asarray(pose, dtype=np.float64).astype(F32)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def face_facing(vertices, faces, pose):
    """f32 [F]: |n_z| / |n| of n = (P1 - P0) x (P2 - P0) in float64 from the f32 camera points, 0 where n = 0."""
    P = camera_points(vertices, pose).astype(np.float64)
    F = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = P[F[:, 1]] - P[F[:, 0]], P[F[:, 2]] - P[F[:, 0]]
    nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    nn = (nx * nx + ny * ny) + nz * nz
    with np.errstate(all="ignore"):
        return np.where(nn == 0.0, 0.0, np.abs(nz) / np.sqrt(nn)).astype(F32)


def render_instance(mesh, pose, cam, hw, pixel_offset, z_near):
    """One instance alone -> (color, depth, face, covered bool [H,W])."""
    V, F, C = mesh
    K = rc.cam_matrix(*[float(F32(v)) for v in cam])
    color, depth, face, _s = rc.render(V, F, C, pose, K, hw, pixel_offset, z_near)
    _d, count, _s = rr.render(V, F, pose, K, hw, pixel_offset, z_near)
    return color, depth, face, count > 0


def render_scenes(meshes, instance_mesh, transforms, scene_first, cams, hw, pixel_offset=0.0, z_near=0.05, background=None):
    """meshes: list of (V f64 [V,3], F int [F,3], C u8 [V,3]) -> dict of color u8 [S,H,W,3], depth f32 [S,H,W], instance
    int32 (-1 = nothing drawn), face int32 (-1), facing f32 (0), amodal bool [I,H,W], alone = the per-instance renders."""
    H, W = hw
    S, I = len(cams), len(instance_mesh)
    color = np.zeros((S, H, W, 3), np.uint8)
    if background is not None:
        color[:] = np.asarray(background, np.uint8).reshape(-1, H, W, 3)
    depth = np.zeros((S, H, W), F32)
    instance = np.full((S, H, W), -1, np.int32)
    face = np.full((S, H, W), -1, np.int32)
    facing = np.zeros((S, H, W), F32)
    amodal = np.zeros((I, H, W), bool)
    alone = []
    for s in range(S):
        for i in range(int(scene_first[s]), int(scene_first[s + 1])):       # ascending: a tie stays with the lower instance
            mesh = meshes[int(instance_mesh[i])]
            c, d, f, cov = render_instance(mesh, transforms[i], cams[s], hw, pixel_offset, z_near)
            alone.append((c, d, f))
            amodal[i] = cov
            take = (d > 0) & ((instance[s] < 0) | (d < depth[s]))
            per_face = face_facing(mesh[0], mesh[1], transforms[i])
            color[s][take], depth[s][take], face[s][take], instance[s][take] = c[take], d[take], f[take], i
            facing[s][take] = per_face[f[take]]
    return {"color": color, "depth": depth, "instance": instance, "face": face, "facing": facing, "amodal": amodal,
            "alone": alone}


# ---- SPEC 13.5 ----------------------------------------------------------------------------------------------------------------
def _box(mask):
    ys, xs = np.nonzero(mask)
    if len(ys) == 0:
        return [-1, -1, -1, -1]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def gt_info(amodal, instance, sensor_depth, scene_first):
    """int32 [I,12]: px_count_all, px_count_visib, px_count_valid, bbox_obj (x, y, w, h), bbox_visib, 0."""
    out = np.zeros((len(amodal), 12), np.int32)
    for s in range(len(scene_first) - 1):
        for i in range(int(scene_first[s]), int(scene_first[s + 1])):
            visib = instance[s] == i
            out[i, 0], out[i, 1] = amodal[i].sum(), visib.sum()
            out[i, 2] = (amodal[i] & (sensor_depth[s] > 0)).sum()
            out[i, 3:7], out[i, 7:11] = _box(amodal[i]), _box(visib)
    return out


# ---- SPEC 13.6 ----------------------------------------------------------------------------------------------------------------
def sensor(depth, facing, thresholds, n_rects, rects, units, unit_inv):
    """-> (depth_u16 uint16 [S,H,W], depth f32, keep bool). rects (r0, r1, c0, c1) are non-negative."""
    keep = facing >= np.asarray(thresholds, F32)[:, None, None]
    for s in range(len(depth)):
        for k in range(int(n_rects[s])):
            r0, r1, c0, c1 = (int(v) for v in rects[s][k])
            assert min(r0, r1, c0, c1) >= 0
            keep[s, r0:r1, c0:c1] = False
    q = np.rint(depth.astype(np.float64) * float(units))
    q[~keep] = 0.0
    q[q > 65535.0] = 0.0
    return q.astype(np.uint16), (q * float(unit_inv)).astype(F32), keep


def pack_amodal(amodal):
    """bool [I,H,W] -> uint32 [I,H,ceil(W/32)]: bit x & 31 of word x >> 5."""
    I, H, W = amodal.shape
    padded = np.zeros((I, H, 32 * ((W + 31) // 32)), np.uint8)
    padded[..., :W] = amodal
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u4").astype(np.uint32)


# ---- the fixture -------------------------------------------------------------------------------------------------------------
HW = (40, 56)                      # W is not a multiple of 32: the amodal rows have a tail word
CAM = (60.0, 60.0, 27.5, 19.5)
CAM3 = (70.0, 65.0, 30.0, 18.0)    # the third scene's own camera
NEAR = 0.05


def cube(h):
    V = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=np.float64)
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return V, F


def quad(h):
    return np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]], dtype=np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


@functools.lru_cache(maxsize=None)
def fixture():
    """-> dict: meshes {obj_id: (V, F, C)} (1 cube, 2 sphere, 3 quad), instance_obj [I], transforms [I,4,4], scene_first,
    cams [S,4], sensor inputs. Computed once; callers must not write into it."""
    rng = np.random.default_rng(13)
    sv, sf = rr.icosphere(2)
    geo = {1: cube(0.05), 2: (0.06 * sv, sf), 3: quad(0.6)}
    meshes = {o: (V, F, rng.integers(0, 256, (len(V), 3)).astype(np.uint8)) for o, (V, F) in geo.items()}
    inst = [(3, rr.pose_at((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), 20.0)),      # 0 the table: the whole-wave path
            (1, rr.pose_at((-0.10, 0.0, 0.60))),                          # 1 a cube
            (1, rr.pose_at((-0.10, 0.0, 0.60))),                          # 2 the same cube again: an exact tie everywhere
            (2, rr.pose_at((-0.06, 0.01, 0.60))),                         # 3 a sphere through the cube
            (1, rr.pose_at((0.25, 0.0, 0.62))),                           # 4 a cube cut by the right edge
            (2, rr.pose_at((0.0, 0.0, 1.6))),                             # 5 a sphere behind the table
            (1, rr.pose_at((0.0, 0.0, -0.2))),                            # 6 a cube behind the camera
            (1, rr.pose_at((0.02, 0.0, 0.50))),                           # scene 2, under its own camera
            (2, rr.pose_at((0.0, 0.02, 0.45)))]
    H, W = HW
    rects = np.zeros((3, 6, 4), np.int32)
    rects[0] = [(5, 12, 3, 20), (10, 10, 0, 56), (30, 47, 40, 70), (0, 3, 50, 56), (18, 25, 24, 25), (39, 40, 0, 56)]
    return {"meshes": meshes, "instance_obj": np.array([o for o, _ in inst]), "transforms": np.stack([T for _, T in inst]),
            "scene_first": np.array([0, 7, 7, 9], np.int32), "cams": np.array([CAM, CAM, CAM3], np.float32),
            # scene 0: six rectangles (one of zero area, one past the border, one over the whole last row); scene 2: none
            "thresholds": np.array([0.2, 0.0, 0.5], np.float32), "n_rects": np.array([6, 0, 0], np.int32), "rects": rects}


@functools.lru_cache(maxsize=None)
def reference():
    """The restatement's outputs on the fixture (meshes in obj_id order 1, 2, 3 = atlas indices 0, 1, 2), computed once:
    the scene render, the corrupted sensor at depth_scale 1 with its gt-info, and the clean sensor at depth_scale 0.01,
    under which every depth beyond 0.65535 m quantises past 16 bits."""
    fx = fixture()
    order = sorted(fx["meshes"])
    meshes = [fx["meshes"][o] for o in order]
    imesh = np.array([order.index(o) for o in fx["instance_obj"]], np.int32)
    out = render_scenes(meshes, imesh, fx["transforms"], fx["scene_first"], fx["cams"], HW, 0.0, NEAR)
    out["instance_mesh"] = imesh
    out["u16"], out["sensor"], out["keep"] = sensor(out["depth"], out["facing"], fx["thresholds"], fx["n_rects"], fx["rects"],
                                                    1000.0 / 1.0, 1.0 / 1000.0)
    out["gt_info"] = gt_info(out["amodal"], out["instance"], out["sensor"], fx["scene_first"])
    zeros = np.zeros(3, np.float32)
    out["u16_fine"], out["sensor_fine"], out["keep_fine"] = sensor(out["depth"], out["facing"], zeros, np.zeros(3, np.int32),
                                                                   fx["rects"], 1000.0 / 0.01, 0.01 / 1000.0)
    out["gt_info_fine"] = gt_info(out["amodal"], out["instance"], out["sensor_fine"], fx["scene_first"])
    return out
