"""Cluttered multi-object RGB-D scenes with BOP ground truth, rendered on the device (csrc/scene.hip, SPEC.md section 13):
the data the reference gets from offline BlenderProc renders (datasets/render_dataset.py:81-189,
datasets/dtoid_dataset.py:97-235) and corrupts with utils/augmentation.py:5-26. A directory of BOP .ply models, vertex-
coloured (LM-O) or texture-mapped (YCB-V: `comment TextureFile`, UVs and a PNG beside the model), is enough to train the
scorer, run the stream and evaluate it:

    atlas = MeshAtlas({obj_id: render.Mesh(V, F, colors=C), ...})          # metres; or read_models_dir(folder)
    layout = sample_layouts(atlas, 32, 12, cam_K, (480, 640), rng)
    batch = render_scenes(atlas, layout, (480, 640), sensor=sample_sensor(32, (480, 640), rng))
    batch.write_bop(root, "synth")        # bop_eval.BopFolder, tools/eval_bop19.py and read_bop_frames read it back
    for frame in batch.frames(): ...      # the dicts OnlineStream.process / networkInference / make_dtoid_sample take

MeshAtlas, Layout, Sensor and the folder reader and writer are host code and need no device; render_scenes needs one.
The layout and sensor sampling are build-defined (SPEC 13.7-13.8): host numpy from the caller's Generator.

The scenes are unlit unless asked otherwise (csrc/scene_light.hip, SPEC 13.10-13.12):

    lights, material = sample_lights(layout, rng)                            # or a Lights of your own
    batch = render_scenes(atlas, layout, (480, 640), lights=lights, material=material)     # .color lit, .albedo, .normal

and the lights cast no shadows unless asked (csrc/scene_shadow.hip, SPEC 13.13-13.15):

    batch = render_scenes(atlas, layout, (480, 640), lights=lights, material=material, shadows=Shadows())    # .blocked

and the objects float at free poses unless asked to rest on the table (csrc/scene_rest.hip, SPEC 13.16-13.18):

    layout = sample_layouts(atlas, 32, 12, cam_K, (480, 640), rng, placement="rest")    # .table_pose, .local, .drop, .status
"""
import ctypes
import json
import os

import numpy as np
import torch

from . import _lib
from . import render as _render

TABLE_OBJ_ID = 0            # the atlas's own mesh behind the objects; real objects have ids >= 1, as in BOP


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


class MeshAtlas:
    """Meshes packed back to back (SPEC 13.1): vertices f32 [Vt,3], colors u8 [Vt,3], faces int32 [Ft,3] with indices
    local to their mesh, table int32 [K,4] = (v0, nv, f0, nf), on the host (`*_host`) and on the device of the meshes.
    meshes: dict obj_id (>= 1) -> render.Mesh with vertex colours, a texture or both, all on one device and in one unit
    (metres). The last mesh, obj_id TABLE_OBJ_ID, is the unit square [-1, 1]^2 in z = 0 that sample_layouts scales into a
    table; it is vertex-coloured.

    Each mesh is drawn from the surface render_color would take (render._textured): its vertex colours when it has them,
    unless use_texture asks for its texture; its texture when that is all it has. use_texture=True asks for every
    object's texture, a collection of object ids for theirs (an atlas of textured and vertex-coloured models); an object
    it asks for that has no texture is refused. `textured` is the choice made, a bool per mesh. With a
    textured mesh the atlas also keeps uvs f32 [Vt,2] (zero rows where unused), mips -- the chosen meshes' Mesh.mips
    concatenated on the device -- and tex_table int64 [K,3] = (first texel of the mesh's chain, Ht, Wt), zeros for a
    vertex-coloured mesh; all three are None when no mesh is textured. The colour rows of a texture-only mesh are zeros."""

    uvs = uvs_host = mips = tex_table = tex_table_host = _normals = _radii = None

    @property
    def normals(self):
        """f32 [Vt,3] on the atlas's device, row for row beside `vertices`: each mesh's smooth vertex normals (SPEC 13.10,
        mesh_vertex_normals), built on first use -- an atlas that is never lit never pays for them. Hard edges are not
        detected; the table's two triangles get their flat normal."""
        if self._normals is None:
            out = torch.empty(len(self.vertices_host), 3, dtype=torch.float32, device=self.device)
            for v0, nv, f0, nf in self.table_host:
                mesh_vertex_normals(self.vertices[v0:v0 + nv], self.faces[f0:f0 + nf],
                                    normals_shift(self.vertices_host[v0:v0 + nv]), out=out[v0:v0 + nv])
            self._normals = out
        return self._normals

    def __init__(self, meshes, table_color=(128, 120, 110), use_texture=False):
        if not isinstance(meshes, dict) or len(meshes) < 1:
            raise ValueError("MeshAtlas: meshes must be a non-empty dict obj_id -> render.Mesh")
        ids = sorted(int(k) for k in meshes)
        if ids[0] < 1 or len(set(ids)) != len(ids):
            raise ValueError("MeshAtlas: object ids must be distinct integers >= 1, got %s" % (ids,))
        by_id = {int(k): m for k, m in meshes.items()}
        devices = {str(by_id[i].device) for i in ids if isinstance(by_id[i], _render.Mesh)}
        if isinstance(use_texture, (bool, np.bool_)):
            wanted = set(ids) if use_texture else set()
        else:
            wanted = {int(o) for o in use_texture}
        if not wanted <= set(ids):
            raise ValueError("MeshAtlas: use_texture names objects %s, which the atlas does not hold" % sorted(wanted - set(ids)))
        for i in ids:
            m = by_id[i]
            if not isinstance(m, _render.Mesh) or (m.colors is None and not _render._has_texture(m)):
                raise ValueError("MeshAtlas: object %d is not a render.Mesh with vertex colours (Mesh(..., colors=...)) or a "
                                 "texture (Mesh(..., uvs=..., texture=...), render.load_mesh(path))" % i)
            if i in wanted and not _render._has_texture(m):
                raise ValueError("MeshAtlas: use_texture asks for the texture of object %d, which has none" % i)
            if _render._textured(m, i in wanted) and m.device.type != "cuda":
                # Mesh builds mip chains on the GPU only, so a host mesh's texture is of no use to an atlas
                raise ValueError("MeshAtlas: object %d is not a render.Mesh with vertex colours, and a texture is drawn from "
                                 "on the GPU only (its device is %s)" % (i, m.device))
            if m.n_faces > _lib.RASTER_MAX_FACES:
                raise ValueError("MeshAtlas: object %d has %d faces, at most %d" % (i, m.n_faces, _lib.RASTER_MAX_FACES))
        if len(devices) != 1:
            raise ValueError("MeshAtlas: the meshes live on different devices: %s" % sorted(devices))
        self.device = by_id[ids[0]].device
        V = [by_id[i].vertices.cpu().numpy() for i in ids] + [np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32)]
        C = [np.zeros((by_id[i].n_vertices, 3), np.uint8) if by_id[i].colors is None else by_id[i].colors.cpu().numpy()
             for i in ids] + [np.tile(np.asarray(table_color, np.uint8), (4, 1))]
        F = [by_id[i].faces.cpu().numpy().reshape(-1, 3) for i in ids] + [np.array([[0, 1, 2], [0, 2, 3]], np.int32)]
        self.obj_ids = ids + [TABLE_OBJ_ID]
        self.index_of = {o: k for k, o in enumerate(self.obj_ids)}
        nv, nf = np.array([len(v) for v in V]), np.array([len(f) for f in F])
        v0, f0 = np.concatenate([[0], np.cumsum(nv)[:-1]]), np.concatenate([[0], np.cumsum(nf)[:-1]])
        if nv.sum() > 1 << 29 or nf.sum() > 1 << 29:
            raise ValueError("MeshAtlas: %d vertices and %d faces in all, at most 2^29 each" % (nv.sum(), nf.sum()))
        self.table_host = np.ascontiguousarray(np.stack([v0, nv, f0, nf], 1).astype(np.int32))
        self.vertices_host = np.ascontiguousarray(np.concatenate(V).astype(np.float32))
        self.colors_host = np.ascontiguousarray(np.concatenate(C).astype(np.uint8))
        self.faces_host = np.ascontiguousarray(np.concatenate(F).astype(np.int32))
        self.vertices, self.colors, self.faces, self.table = (
            torch.from_numpy(a).to(self.device) for a in (self.vertices_host, self.colors_host, self.faces_host, self.table_host))
        self.n_meshes = len(self.obj_ids)
        self.textured = np.array([_render._textured(by_id[i], i in wanted) for i in ids] + [False])
        if self.textured.any():
            chosen = [by_id[i] for i, t in zip(ids, self.textured) if t]
            U = np.zeros((len(self.vertices_host), 2), np.float32)
            tex = np.zeros((self.n_meshes, 3), np.int64)
            t0 = 0
            for k in np.nonzero(self.textured)[0]:
                m = by_id[ids[k]]
                U[v0[k]:v0[k] + nv[k]] = m.uvs.cpu().numpy()
                tex[k] = (t0, m.texture_hw[0], m.texture_hw[1])
                t0 += m.mips.numel() // 4
            self.uvs_host, self.tex_table_host = U, tex
            self.uvs, self.tex_table = torch.from_numpy(U).to(self.device), torch.from_numpy(tex).to(self.device)
            self.mips = torch.cat([m.mips.reshape(-1) for m in chosen])         # device to device: nothing is rebuilt

    def mesh_arrays(self, obj_id):
        """(vertices f32 [V,3], faces int32 [F,3], colors u8 [V,3]) of one object, host arrays; the colours of a mesh that
        has only a texture are zeros."""
        v0, nv, f0, nf = self.table_host[self.index_of[int(obj_id)]]
        return self.vertices_host[v0:v0 + nv], self.faces_host[f0:f0 + nf], self.colors_host[v0:v0 + nv]

    def texture_arrays(self, obj_id):
        """(uvs f32 [V,2], image u8 [Ht,Wt,3]) of an object the atlas draws from its texture, host arrays, or None for a
        vertex-coloured one. The image is level 0 of the object's chain, read back: for the folder writer, not for a loop."""
        k = self.index_of[int(obj_id)]
        if not self.textured[k]:
            return None
        v0, nv = self.table_host[k, :2]
        t0, Ht, Wt = (int(v) for v in self.tex_table_host[k])
        image = self.mips[4 * t0:4 * (t0 + Ht * Wt)].reshape(Ht, Wt, 4)[..., :3].cpu().numpy()
        return self.uvs_host[v0:v0 + nv], np.ascontiguousarray(image)

    def radius(self, obj_id):
        """The largest distance of a vertex from the mesh's origin. Computed once per object and kept: the atlas's
        vertices are fixed at construction (vertices_host is not to be written into)."""
        if self._radii is None:
            self._radii = {}
        if int(obj_id) not in self._radii:
            V = self.mesh_arrays(obj_id)[0].astype(np.float64)
            self._radii[int(obj_id)] = float(np.sqrt((V * V).sum(1).max()))
        return self._radii[int(obj_id)]

    _resting = None

    def resting(self, obj_id, level=4):
        """The resting orientations of one object (SPEC 13.16-13.17) -> Resting, computed once per (object, level) and
        kept like `radius`: the support heights of the object's vertices along the icosphere directions of `level`
        (render._icosphere_vertices: 2562 at level 4, about 2 degrees apart), one launch of ossid_mesh_support and one
        read-back, then resting_table on the host about the surface centroid. Needs the atlas on a GPU."""
        if self._resting is None:
            self._resting = {}
        key = (int(obj_id), int(level))
        if key not in self._resting:
            if not 0 <= key[1] <= 5:
                raise ValueError("resting: the icosphere level must lie in [0, 5], got %r" % (level,))
            v0, nv, _f0, _nf = self.table_host[self.index_of[key[0]]]
            V, F, _C = self.mesh_arrays(key[0])
            dirs = _render._icosphere_vertices(key[1])
            h = mesh_support(self.vertices[v0:v0 + nv], dirs)
            t = resting_table(dirs, h, surface_centroid(V, F))
            # per resting orientation the object's extent in the table frame, the same under any yaw: how high its origin
            # lies when it stands on the table, how far it reaches above the origin, and its horizontal radius
            P = [V[np.isfinite(V).all(1)].astype(np.float64) @ R.T for R in t.rotations]
            t.extent = np.array([[-p[:, 2].min(), p[:, 2].max(), np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]).max())]
                                 if len(p) else [0.0, 0.0, 0.0] for p in P])
            self._resting[key] = t
        return self._resting[key]


class Layout:
    """A draw list (SPEC 13.1): instance_mesh int32 [I] (index into the atlas's table), transforms f64 [I,4,4]
    (model -> camera; rows 0-2 are used, so a scale is allowed), scene_first int32 [S+1] (the instances of a scene are
    contiguous; an empty scene is legal), cams f32 [S,4] = fx, fy, cx, cy. table_mesh: the atlas index of the mesh that
    is a table, not an object (sample_layouts sets it; sample_lights gives its instances no highlight), or None.

    A layout of sample_layouts(placement="rest") (SPEC 13.18) also holds table_pose f64 [S,4,4] (table frame -> camera),
    local f64 [I,3,4] (model -> table frame before the drop), drop f64 [I] and status int32 [I] (ossid_scene_drop's; 0
    for the table's own instance): transforms[i] = table_pose[s] . translate(0, 0, drop[i]) . local[i], and grid = (G,
    cell), the field the objects were dropped on. All five are None for any other layout."""

    table_pose = local = drop = status = grid = None

    def __init__(self, instance_mesh, transforms, scene_first, cams, table_mesh=None):
        self.table_mesh = None if table_mesh is None else int(table_mesh)
        self.instance_mesh = np.ascontiguousarray(np.asarray(instance_mesh).reshape(-1), dtype=np.int32)
        self.transforms = np.ascontiguousarray(np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4))
        self.scene_first = np.ascontiguousarray(np.asarray(scene_first).reshape(-1), dtype=np.int32)
        self.cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float64).reshape(-1, 4).astype(np.float32))
        S, I = len(self.cams), len(self.instance_mesh)
        if not 1 <= S <= _lib.SCENE_MAX_SCENES:
            raise ValueError("a layout has 1 to %d scenes, got %d" % (_lib.SCENE_MAX_SCENES, S))
        if len(self.scene_first) != S + 1 or self.scene_first[0] != 0 or self.scene_first[-1] != I or \
                np.any(np.diff(self.scene_first) < 0):
            raise ValueError("scene_first must be non-decreasing [S+1] = [%d] from 0 to I = %d, got %s"
                             % (S + 1, I, self.scene_first.tolist()))
        if np.diff(self.scene_first).max(initial=0) > _lib.SCENE_MAX_INSTANCES:
            raise ValueError("a scene has at most %d instances, got %d"
                             % (_lib.SCENE_MAX_INSTANCES, np.diff(self.scene_first).max()))
        if len(self.transforms) != I:
            raise ValueError("transforms must be [I,4,4] = [%d,4,4], got %s" % (I, self.transforms.shape))
        if not (np.isfinite(self.transforms).all() and np.isfinite(self.cams).all()):
            raise ValueError("transforms and cams must be finite")

    @property
    def n_scenes(self):
        return len(self.cams)

    @property
    def n_instances(self):
        return len(self.instance_mesh)

    def cam_K(self, s):
        fx, fy, cx, cy = (float(v) for v in self.cams[s])
        return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


class Sensor:
    """The inputs of SPEC 13.6 per scene: thresholds f32 [S], n_rects int32 [S] in [0, 6], rects int32 [S,6,4] =
    (r0, r1, c0, c1), rows [r0, r1) and columns [c0, c1)."""

    def __init__(self, thresholds, n_rects, rects):
        self.thresholds = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64).reshape(-1).astype(np.float32))
        self.n_rects = np.ascontiguousarray(np.asarray(n_rects).reshape(-1), dtype=np.int32)
        S = len(self.thresholds)
        self.rects = np.ascontiguousarray(np.asarray(rects).reshape(S, _lib.SCENE_MAX_RECTS, 4), dtype=np.int32)
        if len(self.n_rects) != S or (S and (self.n_rects.min() < 0 or self.n_rects.max() > _lib.SCENE_MAX_RECTS)):
            raise ValueError("n_rects must be [S] = [%d] with values in [0, %d]" % (S, _lib.SCENE_MAX_RECTS))
        if not np.isfinite(self.thresholds).all():
            raise ValueError("thresholds must be finite")

    @staticmethod
    def clean(n_scenes):
        """Quantisation only: every pixel keeps its depth."""
        return Sensor(np.zeros(n_scenes), np.zeros(n_scenes, np.int32), np.zeros((n_scenes, _lib.SCENE_MAX_RECTS, 4), np.int32))


def _uniform_rotation(rng):
    """Uniform over SO(3): a normalised 4-vector of normals as a quaternion (w, x, y, z)."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.sqrt(q @ q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def surface_centroid(vertices, faces):
    """SPEC 13.17 -> f64 [3]: the area-weighted centroid of a mesh's surface, sum(A_f m_f) / sum(A_f) with A_f the area and
    m_f the mean corner of face f, over the faces whose indices are valid and whose area is finite and not zero; the mean
    of the finite vertices when no face counts ((0, 0, 0) without one). It stands in for the centre of mass -- that of a
    thin shell of even thickness, not of a solid -- and, unlike the solid's, is defined for an open mesh."""
    V = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    F = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    F = F[((F >= 0) & (F < len(V))).all(1)]
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
        n = np.cross(b - a, c - a)
        area = 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        mid = ((a + b) + c) / 3.0
        ok = np.isfinite(area) & (area > 0.0) & np.isfinite(mid).all(1)
        total = float(area[ok].sum())
        if ok.any() and np.isfinite(total) and total > 0.0:
            return (area[ok, None] * mid[ok]).sum(0) / total
    fin = V[np.isfinite(V).all(1)]
    return fin.sum(0) / float(len(fin)) if len(fin) else np.zeros(3)


def mesh_support(vertices, dirs):
    """SPEC 13.16 -> f64 [D], host: h[d] = the largest ((dx x + dy y) + dz z) over the finite vertices of a device tensor
    f32 [V,3], in f64; -inf when none is finite. One launch of ossid_mesh_support on the current stream and one read-back."""
    from .model_cloud import _refuse_cpu
    dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 3))
    if not (torch.is_tensor(vertices) and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3
            and 1 <= vertices.shape[0] <= _lib.RASTER_MAX_VERTICES):
        raise ValueError("mesh_support: vertices must be a float32 tensor [V,3], 1 <= V <= %d" % _lib.RASTER_MAX_VERTICES)
    if not 1 <= len(dirs) <= _lib.REST_MAX_DIRS:
        raise ValueError("mesh_support: dirs must be [D,3] with 1 <= D <= %d, got %d rows" % (_lib.REST_MAX_DIRS, len(dirs)))
    _refuse_cpu(vertices.device)
    vertices = vertices.contiguous()
    d_dirs = torch.from_numpy(dirs).to(vertices.device)
    h = torch.empty(len(dirs), dtype=torch.float64, device=vertices.device)
    with _lib.on_device(vertices.device):
        _lib.check(_lib.fn("ossid_mesh_support")(vertices.data_ptr(), int(vertices.shape[0]), d_dirs.data_ptr(), len(dirs),
                                                 h.data_ptr(), _lib.stream()), "ossid_mesh_support")
    return h.cpu().numpy()


REST_NEIGHBOURS = 6         # a direction's neighbours on the grid of directions (an icosphere vertex has 5 or 6)
REST_WIDER = 18             # ... and the two rings around it, looked at where a walk over the neighbours stalls


class Resting:
    """What resting_table returns, host arrays: dirs f64 [D,3], h and potential f64 [D], centroid f64 [3], neighbours
    int [D,k], rest_of int [D] (the fixed point each direction descends to), fixed int [n] (the fixed points, ascending:
    the resting directions), basin int [n] (how many directions descend to each) and rotations f64 [n,3,3] (rotations[j]
    takes dirs[fixed[j]] to the table's down, (0, 0, -1)). slot_of(d) is the j of rest_of[d], rotation_of(d) its rotation.
    MeshAtlas.resting adds extent f64 [n,3] = (origin above the table, top above the origin, horizontal radius)."""

    extent = None

    def __init__(self, dirs, h, centroid, potential, neighbours, rest_of, fixed, basin, rotations):
        self.dirs, self.h, self.centroid, self.potential, self.neighbours = dirs, h, centroid, potential, neighbours
        self.rest_of, self.fixed, self.basin, self.rotations = rest_of, fixed, basin, rotations
        self._slot = {int(d): j for j, d in enumerate(fixed)}

    def slot_of(self, d):
        return self._slot[int(self.rest_of[int(d)])]

    def rotation_of(self, d):
        return self.rotations[self.slot_of(d)]


def descend(potential, neighbours, wider=None):
    """SPEC 13.17's descent -> rest_of int [D]: from d, step to the neighbour with the lowest potential that is strictly
    below the current one (the lowest index among equals) until there is none. Every step lowers the potential, so the
    walk ends; a direction whose potential is NaN stays where it is. wider int [D,k2], when given, is looked at where the
    neighbours hold nothing lower, by the same rule: the walk stops only where neither holds a lower direction."""
    U = np.asarray(potential, dtype=np.float64).reshape(-1)
    rings = [np.asarray(n, dtype=np.int64).reshape(len(U), -1) for n in (neighbours, wider) if n is not None]
    step = np.arange(len(U))
    for d in range(len(U)):
        for N in rings:
            best, at = U[d], d
            for j in N[d]:
                if U[j] < best or (U[j] == best and at != d and j < at):
                    best, at = U[j], int(j)
            if at != d:
                break
        step[d] = at
    rest_of = step.copy()
    for d in range(len(U)):
        k = d
        while step[k] != k:
            k = step[k]
        rest_of[d] = k
    return rest_of


def rotation_to_down(d):
    """-> f64 [3,3], the rotation that takes the direction d to (0, 0, -1) by the shortest way: about the axis d x
    (0, 0, -1) by the angle between them (Rodrigues: I + K + K K / (1 + c) with K the cross-product matrix of the axis and
    c = -d_z, d normalised first). d = (0, 0, 1), the antipode, has no such axis: within 1e-12 of it (1 + c < 1e-12) the
    half turn about the x axis, diag(1, -1, -1)."""
    d = np.asarray(d, dtype=np.float64).reshape(3)
    d = d / np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    c = -d[2]
    if 1.0 + c < 1e-12:
        return np.diag([1.0, -1.0, -1.0])
    v = np.array([-d[1], d[0], 0.0])                       # d x (0, 0, -1)
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + (K @ K) / (1.0 + c)


def resting_table(dirs, h, centroid):
    """SPEC 13.17, a pure host function of (dirs f64 [D,3], h f64 [D], centroid [3]) -> Resting. A direction d means "this
    side of the object faces down"; U[d] = h[d] - ((dx cx + dy cy) + dz cz) is the centroid's height above the support
    plane then. A direction's neighbours are its REST_NEIGHBOURS nearest others by dot product (all the others when there
    are fewer), ties to the lower index; `descend` follows them downhill, and its fixed points are the resting
    orientations. Drawing d uniformly and taking rest_of[d] lands in each in proportion to its basin.

    U has creases -- for a box the three great circles of the directions that balance it on an edge, valleys that lead
    down to the faces -- and the six neighbours of a grid direction in such a valley can all lie up its walls: on them
    alone a 1 x 2 x 3 box keeps 14 "resting" directions at level 2 and 57 at level 4, most of them on an edge. So where
    the neighbours hold nothing lower, the walk looks once at the REST_WIDER nearest directions (two rings of the grid,
    about 4 degrees at level 4) before it stops; with that the box rests on its six faces at levels 2 to 4."""
    dirs = np.ascontiguousarray(np.asarray(dirs, dtype=np.float64).reshape(-1, 3))
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    c = np.asarray(centroid, dtype=np.float64).reshape(3)
    D = len(dirs)
    if D < 1 or len(h) != D:
        raise ValueError("resting_table: dirs [D,3] and h [D] must agree and D >= 1, got %d and %d" % (D, len(h)))
    if not (np.isfinite(dirs).all() and np.isfinite(c).all()):
        raise ValueError("resting_table: dirs and centroid must be finite")
    U = h - ((dirs[:, 0] * c[0] + dirs[:, 1] * c[1]) + dirs[:, 2] * c[2])
    k = min(REST_NEIGHBOURS, D - 1)
    k2 = min(REST_WIDER, D - 1)
    wider = np.zeros((D, k2), np.int64)
    for d in range(D if k else 0):
        dot = (dirs[:, 0] * dirs[d, 0] + dirs[:, 1] * dirs[d, 1]) + dirs[:, 2] * dirs[d, 2]
        dot[d] = -np.inf
        wider[d] = np.argsort(-dot, kind="stable")[:k2]                       # stable: equal dots keep the lower index first
    neighbours = np.ascontiguousarray(wider[:, :k])
    rest_of = descend(U, neighbours, wider)
    fixed, basin = np.unique(rest_of, return_counts=True)
    rotations = np.stack([rotation_to_down(dirs[d]) for d in fixed])
    return Resting(dirs, h, c, U, neighbours, rest_of, fixed, basin, rotations)


def scene_drop(atlas, instance_mesh, scene_first, local, grid, cell, height=False):
    """SPEC 13.18 -> (drop f64 [I], status int32 [I]) and, with height=True, the final height fields f32 [S,G,G], host
    arrays: ossid_scene_drop over the draw list (instance_mesh int32 [I], scene_first int32 [S+1]) with local f64 [I,3,4],
    model -> table frame. One launch on the current stream, then the read-back of the results: the call's only
    synchronisation."""
    from .model_cloud import _refuse_cpu
    if not isinstance(atlas, MeshAtlas):
        raise ValueError("scene_drop takes a MeshAtlas")
    mesh = np.ascontiguousarray(np.asarray(instance_mesh).reshape(-1), dtype=np.int32)
    first = np.ascontiguousarray(np.asarray(scene_first).reshape(-1), dtype=np.int32)
    I, S, G = len(mesh), len(first) - 1, int(grid)
    local = np.ascontiguousarray(np.asarray(local, dtype=np.float64).reshape(-1, 3, 4))
    if not 1 <= S <= _lib.SCENE_MAX_SCENES or I > S * _lib.SCENE_MAX_INSTANCES:
        raise ValueError("scene_drop: 1 to %d scenes of at most %d instances each, got %d and %d instances"
                         % (_lib.SCENE_MAX_SCENES, _lib.SCENE_MAX_INSTANCES, S, I))
    if len(local) != I:
        raise ValueError("scene_drop: local must be [I,3,4] = [%d,3,4], got %s" % (I, local.shape))
    if not 1 <= G <= _lib.REST_MAX_GRID:
        raise ValueError("scene_drop: grid must lie in [1, %d], got %r" % (_lib.REST_MAX_GRID, grid))
    if not (float(cell) > 0.0 and np.isfinite(float(cell))):
        raise ValueError("scene_drop: cell must be finite and > 0, got %r" % (cell,))
    _refuse_cpu(atlas.device)
    dev = atlas.device
    up = lambda a: torch.from_numpy(a).to(dev)
    d_mesh, d_first, d_local = up(mesh), up(first), up(local)
    drop = torch.empty(I, dtype=torch.float64, device=dev)
    status = torch.empty(I, dtype=torch.int32, device=dev)
    field = torch.empty(S, G, G, dtype=torch.float32, device=dev) if height else None
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_scene_drop")(
            atlas.vertices.data_ptr(), atlas.faces.data_ptr(), atlas.table.data_ptr(), len(atlas.vertices_host),
            len(atlas.faces_host), atlas.n_meshes, d_mesh.data_ptr() if I else None, d_first.data_ptr(),
            d_local.data_ptr() if I else None, I, S, G, float(cell), drop.data_ptr() if I else None,
            status.data_ptr() if I else None, None if field is None else field.data_ptr(), _lib.stream()), "ossid_scene_drop")
    out = (drop.cpu().numpy(), status.cpu().numpy())
    return out + (field.cpu().numpy(),) if height else out


REST_TRIES = 256            # positions tried per object of a rest layout before sample_layouts gives up


def _rest_layouts(atlas, S, n, intr, hw, rng, z_range, table, elevation, rest_level, grid):
    """sample_layouts(placement="rest"), SPEC 13.18, after the argument checks."""
    (H, W), (fx, fy, cx, cy), (z0, z1), (e0, e1) = hw, intr, z_range, elevation
    objects = [o for o in atlas.obj_ids if o != TABLE_OBJ_ID]
    rest = {o: atlas.resting(o, rest_level) for o in objects} if n else {}
    radius = {o: atlas.radius(o) for o in objects}
    r_max = max(radius.values())
    t_mesh = atlas.index_of[TABLE_OBJ_ID]
    mesh, local, first, poses, is_table = [], [], [0], [], []
    # the field is fixed before anything is drawn: no foot point lies farther from the table frame's origin than `reach`
    # (|x'| = |u - cx| / fx z; |y'| = |z - zt| / cos e, and = |v - cy| / fy z / sin e as the foot point lies in the frame)
    far = 1.5 * z1
    reach = max(max(cx, W - cx) / fx * far,
                min((far - z0) / np.cos(np.deg2rad(e1)), max(cy, H - cy) / fy * far / np.sin(np.deg2rad(e0)))) + r_max
    cell = 2.0 * reach * 1.001 / grid                      # the grid covers every object's sphere with a margin
    x0 = -(grid * 0.5) * cell
    for _ in range(S):
        e = np.deg2rad(rng.uniform(e0, e1))
        zt = rng.uniform(z0, z1)
        ce, se = np.cos(e), np.sin(e)
        P = np.eye(4)                                      # columns: x', y' (away from the camera), z' (the table's up), origin
        P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = (1.0, 0.0, 0.0), (0.0, -se, ce), (0.0, -ce, -se), (0.0, 0.0, zt)
        poses.append(P)
        picks = rng.permutation(len(objects))[:n] if n <= len(objects) else rng.integers(0, len(objects), n)
        chosen = [objects[int(k)] for k in picks]
        placed = []                                        # (its box of cells, a bound on the height of its top)
        if table:
            # the square reaches from the depth zn, where the plane leaves the frame's lower edge with a quarter to
            # spare, 2 `half` away from the camera and `half` to either side
            q = 1.25 * max(H - cy, 1.0) / fy
            zn = zt * (se / ce) / (se / ce + q)
            half = 2.0 * (z1 + r_max) * max(W / fx, H / fy, 1.0)
            L = np.zeros((3, 4))
            L[0, 0], L[1, 1], L[2, 2], L[1, 3] = half, half, 1.0, (zn - zt) / ce + half
            mesh.append(t_mesh), local.append(L), is_table.append(True)
        for o in chosen:
            slot = rest[o].slot_of(int(rng.integers(0, len(rest[o].dirs))))
            R, (lo, hi, rho) = rest[o].rotations[slot], rest[o].extent[slot]
            yaw = rng.uniform(0.0, 2.0 * np.pi)
            Rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
            for _try in range(REST_TRIES):
                u, v = rng.uniform(0.0, W), rng.uniform(0.0, H)
                den = ce * ((v - cy) / fy) + se            # the pixel's ray meets the plane at the depth z ...
                z = zt * se / den if den > 0.0 else np.inf
                if not 0.5 * z0 <= z <= 1.5 * z1:          # ... or above the horizon, or too near or far to be of use
                    continue
                xp, yp = (u - cx) / fx * z, (z - zt) / ce
                # the origin ends at the height `drop`: at most `lo` above the table or above the top of an earlier object
                # whose box of cells -- that of its horizontal circle, which holds every triangle's -- meets this one's
                box = [int(np.floor((c - x0) / cell)) for c in (xp - rho, xp + rho, yp - rho, yp + rho)]
                under = [tb for (a0, a1, b0, b1), tb in placed if a0 <= box[1] and box[0] <= a1 and b0 <= box[3] and box[2] <= b1]
                high = lo + max(under, default=0.0)
                foot = P[:3, :3] @ np.array([xp, yp, 0.0]) + P[:3, 3]
                head = foot + high * P[:3, 2]
                inside = True
                for p in (foot, head):                     # the centre lies between them, and the frame is convex
                    pu, pv = (fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy) if p[2] > 0.0 else (-1.0, -1.0)
                    inside = inside and 0.0 <= pu <= W and 0.0 <= pv <= H
                if inside:
                    break
            else:
                raise ValueError("sample_layouts: no position on the table within the frame for an object after %d tries "
                                 "(z_range %r, elevation %r)" % (REST_TRIES, (z0, z1), (e0, e1)))
            L = np.zeros((3, 4))
            L[:, :3], L[0, 3], L[1, 3] = Rz @ R, xp, yp
            placed.append((box, high + hi))
            mesh.append(atlas.index_of[o]), local.append(L), is_table.append(False)
        first.append(len(mesh))
    mesh = np.asarray(mesh, dtype=np.int32)
    local = np.stack(local) if local else np.zeros((0, 3, 4))
    is_table = np.asarray(is_table, dtype=bool)
    I = len(mesh)
    drop, status = np.zeros(I), np.zeros(I, np.int32)
    if (~is_table).any():
        # the objects alone are dropped: the table's own square is the plane z' = 0 the field starts from
        counts = [int((~is_table[first[s]:first[s + 1]]).sum()) for s in range(S)]
        drop[~is_table], status[~is_table] = scene_drop(atlas, mesh[~is_table], np.concatenate([[0], np.cumsum(counts)]),
                                                        local[~is_table], grid, cell)
    T = np.zeros((I, 4, 4))
    for s in range(S):
        for i in range(first[s], first[s + 1]):
            T[i] = rest_compose(poses[s], drop[i], local[i])
    out = Layout(mesh, T, first, np.tile([fx, fy, cx, cy], (S, 1)), table_mesh=t_mesh)
    out.table_pose, out.local, out.drop, out.status = np.stack(poses), local, drop, status
    out.grid = (grid, cell)
    return out


def rest_compose(table_pose, drop, local):
    """SPEC 13.18 -> f64 [4,4]: table_pose . translate(0, 0, drop) . local, local f64 [3,4] completed by the row 0 0 0 1."""
    M, D = np.eye(4), np.eye(4)
    M[:3] = np.asarray(local, dtype=np.float64).reshape(3, 4)
    D[2, 3] = float(drop)
    return np.asarray(table_pose, dtype=np.float64).reshape(4, 4) @ (D @ M)


def sample_layouts(atlas, n_scenes, objects_per_scene, cam_K, hw, rng, z_range=(0.5, 1.2), table=True, placement="free",
                   elevation=(25.0, 65.0), rest_level=4, grid=128):
    """SPEC 13.7 (build-defined) -> Layout of n_scenes scenes under the camera cam_K, each with objects_per_scene objects
    of the atlas: distinct ones while the atlas has enough, drawn with replacement otherwise. Rotations are uniform; a
    centre has its depth uniform in z_range and its projection uniform over the frame. table=True puts the atlas's
    square first in every scene, tilted by 15 to 40 degrees so that it recedes towards the top of the image, its nearest
    edge behind the farthest possible object. The same Generator state gives the same layout.

    placement="free" is the above, draw for draw; elevation, rest_level and grid are not read. placement="rest" (SPEC
    13.18, needs the atlas on a GPU) rests the objects on a table plane instead: per scene the camera's elevation above
    the plane is uniform in `elevation` (degrees, within (0, 90)) and the plane passes through the point of the optical axis at
    a depth uniform in z_range; table=True draws the atlas's square in it, first in the scene. Per object a uniform
    direction index goes through MeshAtlas.resting(obj, rest_level).rest_of to a resting orientation, the yaw about the
    table's normal is uniform, and the foot point is where the ray of a pixel uniform over the frame meets the plane,
    redrawn while that is above the horizon or at a depth outside [z_range[0] / 2, 1.5 z_range[1]], and
    redrawn (at most REST_TRIES times, then a ValueError) until it and the point above it at a bound on the centre's
    height -- the radius above the table or above the earlier objects it can land on -- project inside the frame, so
    every object centre does. One ossid_scene_drop call over all
    scenes on a grid x grid field then stacks the objects in draw order, and ONE read-back of its results -- the call's
    only synchronisation -- gives the transforms. The layout also carries table_pose, local, drop and status."""
    H, W = _render._check_frame(None, hw)
    S, n = int(n_scenes), int(objects_per_scene)
    if not isinstance(rng, np.random.Generator):
        raise ValueError("rng must be a numpy.random.Generator")
    if not 1 <= S <= _lib.SCENE_MAX_SCENES:
        raise ValueError("n_scenes must lie in [1, %d], got %r" % (_lib.SCENE_MAX_SCENES, n_scenes))
    if not 0 <= n <= _lib.SCENE_MAX_INSTANCES - 1:
        raise ValueError("objects_per_scene must lie in [0, %d], got %r" % (_lib.SCENE_MAX_INSTANCES - 1, objects_per_scene))
    z0, z1 = float(z_range[0]), float(z_range[1])
    if not 0.0 < z0 <= z1 < np.inf:
        raise ValueError("z_range must be 0 < near <= far, got %r" % (z_range,))
    fx, fy, cx, cy = _render._intrinsics(cam_K)
    if placement not in ("free", "rest"):
        raise ValueError("placement must be 'free' or 'rest', got %r" % (placement,))
    if placement == "rest":
        try:
            e0, e1 = (float(v) for v in elevation)
        except (TypeError, ValueError):
            e0 = e1 = np.nan
        if not 0.0 < e0 <= e1 < 90.0:
            raise ValueError("elevation must be two angles 0 < low <= high < 90 in degrees, got %r" % (elevation,))
        if isinstance(rest_level, (bool, np.bool_)) or not isinstance(rest_level, (int, np.integer)) or not 0 <= rest_level <= 5:
            raise ValueError("rest_level must be an integer in [0, 5], got %r" % (rest_level,))
        if isinstance(grid, (bool, np.bool_)) or not isinstance(grid, (int, np.integer)) or not 1 <= grid <= _lib.REST_MAX_GRID:
            raise ValueError("grid must be an integer in [1, %d], got %r" % (_lib.REST_MAX_GRID, grid))
        from .model_cloud import _refuse_cpu
        _refuse_cpu(atlas.device)
        return _rest_layouts(atlas, S, n, (fx, fy, cx, cy), (H, W), rng, (z0, z1), bool(table), (e0, e1), int(rest_level),
                             int(grid))
    objects = [o for o in atlas.obj_ids if o != TABLE_OBJ_ID]
    r_max = max(atlas.radius(o) for o in objects)
    mesh, T, first = [], [], [0]
    for _ in range(S):
        if table:
            a = np.deg2rad(rng.uniform(15.0, 40.0))
            half = 1.5 * (z1 + r_max) * max(W / fx, H / fy)
            M = np.eye(4)
            M[:3, :3] = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), np.sin(a)], [0.0, -np.sin(a), np.cos(a)]]) * half
            M[2, 3] = z1 + r_max + half * np.sin(a)
            mesh.append(atlas.index_of[TABLE_OBJ_ID])
            T.append(M)
        picks = rng.permutation(len(objects))[:n] if n <= len(objects) else rng.integers(0, len(objects), n)
        for k in picks:
            z = rng.uniform(z0, z1)
            u, v = rng.uniform(0.0, W), rng.uniform(0.0, H)
            M = np.eye(4)
            M[:3, :3] = _uniform_rotation(rng)
            M[:3, 3] = ((u - cx) / fx * z, (v - cy) / fy * z, z)
            mesh.append(atlas.index_of[objects[int(k)]])
            T.append(M)
        first.append(len(mesh))
    return Layout(mesh, np.zeros((0, 4, 4)) if not T else np.stack(T), first, np.tile([fx, fy, cx, cy], (S, 1)),
                  table_mesh=atlas.index_of[TABLE_OBJ_ID])


def sample_sensor(n_scenes, hw, rng):
    """SPEC 13.8, the distributions of utils/augmentation.py:5-26 -> Sensor: the threshold uniform in [0.2, 0.5]; 0 to 6
    rectangles, each starting at a row and column uniform over the frame with an extent uniform in [H//16, H//4) x
    [W//16, W//4), its end clipped at H-1 / W-1."""
    H, W = _render._check_frame(None, hw)
    S = int(n_scenes)
    if not isinstance(rng, np.random.Generator):
        raise ValueError("rng must be a numpy.random.Generator")
    if not 1 <= S <= _lib.SCENE_MAX_SCENES:
        raise ValueError("n_scenes must lie in [1, %d], got %r" % (_lib.SCENE_MAX_SCENES, n_scenes))
    if H < 8 or W < 8:
        raise ValueError("sample_sensor needs a frame of at least 8 x 8 (the extents are drawn from [side//16, side//4))")
    thresholds = rng.uniform(0.2, 0.5, S)
    n_rects = rng.integers(0, _lib.SCENE_MAX_RECTS + 1, S)
    rects = np.zeros((S, _lib.SCENE_MAX_RECTS, 4), dtype=np.int32)
    for s in range(S):
        for k in range(int(n_rects[s])):
            r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            r1 = min(H - 1, r0 + int(rng.integers(H // 16, H // 4)))
            c1 = min(W - 1, c0 + int(rng.integers(W // 16, W // 4)))
            rects[s, k] = (r0, r1, c0, c1)
    return Sensor(thresholds, n_rects, rects)


def normals_shift(vertices):
    """The fixed-point shift of SPEC 13.10 for one mesh's vertices [V,3], host arithmetic: with e the largest of the
    three f64 extents of the bounding box of the finite vertices, the largest integer with 2 e e 2^shift <= 2^40; 0 when
    e = 0 or no vertex is finite. Every term of a vertex's sum is then at most 2^40 in magnitude."""
    V = np.asarray(vertices, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    V = V[np.isfinite(V).all(1)]
    e = float((V.max(0) - V.min(0)).max()) if len(V) else 0.0
    if not e > 0.0:
        return 0
    m, x = np.frexp(2.0 * e * e)                 # 2 e e = m 2^x exactly, m in [0.5, 1): m 2^(x + shift) <= 2^40
    return int(40 - x + (1 if m == 0.5 else 0))


def mesh_vertex_normals(vertices, faces, shift=None, out=None):
    """SPEC 13.10 -> f32 [V,3] on the device of `vertices`: smooth area-weighted unit normals of one mesh (device tensors
    vertices f32 [V,3], faces int32 [F,3]), bit-reproducible; (0, 0, 0) for a vertex no face uses. shift=None computes
    normals_shift from a copy of the vertices on the host. Three launches on the current stream."""
    from .model_cloud import _refuse_cpu
    if not (torch.is_tensor(vertices) and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3
            and vertices.shape[0] >= 1):
        raise ValueError("mesh_vertex_normals: vertices must be a float32 tensor [V,3] with V >= 1")
    _refuse_cpu(vertices.device)
    if not (torch.is_tensor(faces) and faces.dtype == torch.int32 and faces.device == vertices.device
            and faces.numel() % 3 == 0):
        raise ValueError("mesh_vertex_normals: faces must be an int32 tensor [F,3] on the vertices' device")
    V, F = int(vertices.shape[0]), faces.numel() // 3
    if F > _lib.RASTER_MAX_FACES:
        raise ValueError("mesh_vertex_normals: %d faces, at most %d" % (F, _lib.RASTER_MAX_FACES))
    shift = normals_shift(vertices.cpu().numpy()) if shift is None else int(shift)
    vertices, faces = vertices.contiguous(), faces.contiguous()
    if out is None:
        out = torch.empty(V, 3, dtype=torch.float32, device=vertices.device)
    elif not (out.dtype == torch.float32 and tuple(out.shape) == (V, 3) and out.is_contiguous() and out.device == vertices.device):
        raise ValueError("mesh_vertex_normals: out must be a contiguous float32 [V,3] = [%d,3] on the vertices' device" % V)
    need = int(_lib.fn("ossid_mesh_vertex_normals_workspace_bytes")(V))
    ws = torch.empty(need // 8, dtype=torch.int64, device=vertices.device)
    with _lib.on_device(vertices.device):
        _lib.check(_lib.fn("ossid_mesh_vertex_normals")(vertices.data_ptr(), faces.data_ptr() if F else None, V, F, shift,
                                                        ws.data_ptr(), need, out.data_ptr(), _lib.stream()),
                   "ossid_mesh_vertex_normals")
    return out


class Lights:
    """The lights of SPEC 13.11 per scene, host arrays: lights f32 [S,4,8] = (x, y, z, w, r, g, b, unused) in camera
    space -- w == 0: (x, y, z) is the direction towards the light, otherwise the position of a point light --, n_lights
    int32 [S] in [0, 4], ambient f32 [S,3]."""

    def __init__(self, lights, n_lights, ambient):
        lights, n_lights, ambient = np.asarray(lights), np.asarray(n_lights), np.asarray(ambient)
        M = _lib.SCENE_MAX_LIGHTS
        if lights.ndim != 3 or lights.shape[1:] != (M, 8) or lights.dtype.kind != "f":
            raise ValueError("lights must be a float array [S,%d,8], got %s %s" % (M, lights.dtype, lights.shape))
        S = lights.shape[0]
        if n_lights.shape != (S,) or n_lights.dtype.kind not in "iu" or (S and (n_lights.min() < 0 or n_lights.max() > M)):
            raise ValueError("n_lights must be an integer array [S] = [%d] with values in [0, %d], got %s %s"
                             % (S, M, n_lights.dtype, n_lights.shape))
        if ambient.shape != (S, 3) or ambient.dtype.kind != "f":
            raise ValueError("ambient must be a float array [S,3] = [%d,3], got %s %s" % (S, ambient.dtype, ambient.shape))
        self.lights = np.ascontiguousarray(lights.astype(np.float32))
        self.n_lights = np.ascontiguousarray(n_lights.astype(np.int32))
        self.ambient = np.ascontiguousarray(ambient.astype(np.float32))
        if not (np.isfinite(self.lights).all() and np.isfinite(self.ambient).all()):
            raise ValueError("lights and ambient must be finite")

    @property
    def n_scenes(self):
        return len(self.n_lights)

    @staticmethod
    def neutral(n_scenes):
        """Ambient 1 and no light: the lit image is the albedo, bit for bit."""
        S = int(n_scenes)
        return Lights(np.zeros((S, _lib.SCENE_MAX_LIGHTS, 8), np.float32), np.zeros(S, np.int32), np.ones((S, 3), np.float32))


def sample_lights(layout, rng, strength=1.0):
    """SPEC 13.12 (build-defined, host numpy) -> (Lights, material f32 [I,2] = (k_s, e)) for the layout's scenes and
    instances, drawn from the caller's Generator. Per scene 1 to 3 lights, each directional or a point light with equal
    odds, on the camera's side of the scene, and a tinted ambient term; per instance a specular weight k_s in [0, 0.3] and
    an exponent 2^e, e in 3..7. Instances of layout.table_mesh get k_s = 0. strength in [0, 1]
    scales the departure from Lights.neutral; 0 returns it, with a zero material, and draws nothing. The same
    Generator state gives the same lights."""
    if not isinstance(layout, Layout):
        raise ValueError("sample_lights takes a Layout")
    if not isinstance(rng, np.random.Generator):
        raise ValueError("rng must be a numpy.random.Generator")
    s = float(strength)
    if not 0.0 <= s <= 1.0:
        raise ValueError("strength must lie in [0, 1], got %r" % (strength,))
    S, I = layout.n_scenes, layout.n_instances
    material = np.zeros((I, 2), np.float32)
    if s == 0.0:
        return Lights.neutral(S), material
    table = layout.table_mesh
    rows = np.zeros((S, _lib.SCENE_MAX_LIGHTS, 8), np.float64)
    count, ambient = np.zeros(S, np.int32), np.zeros((S, 3), np.float64)
    for k in range(S):
        n = int(rng.integers(1, 4))
        count[k] = n
        for l in range(n):
            point = int(rng.integers(0, 2))
            g = rng.normal(size=3)
            t = rng.uniform(0.5, 3.0)                      # drawn for a directional light too: the draw count is fixed
            base, tint = rng.uniform(0.3, 0.9), rng.uniform(-0.1, 0.1, 3)
            g[2] = -abs(g[2])                              # the camera's side: the camera looks along +z
            norm = np.sqrt(g @ g)
            d = g / norm if norm > 0.0 else np.array([0.0, 0.0, -1.0])
            rows[k, l, :3] = d * t if point else d
            rows[k, l, 3] = float(point)
            rows[k, l, 4:7] = s * (base / n) * (1.0 + tint)
        a, tint = rng.uniform(0.25, 0.6), rng.uniform(-0.1, 0.1, 3)
        ambient[k] = (1.0 - s) + s * a * (1.0 + tint)
    for i in range(I):
        ks, e = rng.uniform(0.0, 0.3), int(rng.integers(3, 8))
        material[i] = (0.0 if table is not None and layout.instance_mesh[i] == table else s * ks, e)
    return Lights(rows.astype(np.float32), count, ambient.astype(np.float32)), material


def _check_lights(layout, lights, material):
    """-> material f32 [I,2] (zeros for None) after the checks of a Lights and a material against a layout."""
    if not isinstance(lights, Lights) or lights.n_scenes != layout.n_scenes:
        raise ValueError("lights must be a Lights of the layout's %d scenes" % layout.n_scenes)
    I = layout.n_instances
    if material is None:
        return np.zeros((I, 2), np.float32)
    material = np.asarray(material)
    if material.shape != (I, 2) or material.dtype.kind != "f" or not np.isfinite(material).all():
        raise ValueError("material must be a finite float array [I,2] = [%d,2] of (k_s, e), got %s %s"
                         % (I, material.dtype, material.shape))
    return np.ascontiguousarray(material.astype(np.float32))


SHADOW_MAX_SIDE = 4096      # Hs, Ws of a shadow map (csrc/scene_shadow.h)
SHADOW_FACES = 64           # faces per row of the shadow pass's work list: one per lane of a wave
SHADOW_Z_NEAR = 1e-3        # z_near_l: in front of it a vertex is usable from the light


class Shadows:
    """Cast shadows for a lit render (SPEC 13.13-13.15): size = (Hs, Ws) of the depth map each (scene, light) gets, each
    side in [1, 4096], and beta = (beta0, beta1), the constant and the slope-scaled depth bias in texels."""

    def __init__(self, size=(512, 512), beta=(1.5, 1.5)):
        self.size, self.beta = size, beta
        _check_shadows(self)


def _check_shadows(shadows, lights=True):
    """-> ((Hs, Ws), (beta0, beta1)) of a Shadows, after the checks render_scenes makes before it touches the device."""
    if not isinstance(shadows, Shadows):
        raise ValueError("shadows must be a scenes.Shadows or None, got %r" % (shadows,))
    if lights is None:
        raise ValueError("shadows are cast by lights: shadows is given without lights")
    try:
        size = tuple(shadows.size)
        ok = len(size) == 2 and all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in size)
    except TypeError:
        ok = False
    if not ok or not all(1 <= int(v) <= SHADOW_MAX_SIDE for v in size):
        raise ValueError("Shadows: size must be two integers (Hs, Ws) in [1, %d], got %r" % (SHADOW_MAX_SIDE, shadows.size))
    try:
        beta = tuple(float(v) for v in shadows.beta)
    except (TypeError, ValueError):
        beta = ()
    with np.errstate(over="ignore"):                       # a beta past f32's range is refused as not finite
        finite = len(beta) == 2 and bool(np.isfinite(np.asarray(beta, dtype=np.float64).astype(np.float32)).all())
    if not finite:
        raise ValueError("Shadows: beta must be two finite numbers (beta0, beta1), got %r" % (shadows.beta,))
    return (int(size[0]), int(size[1])), beta


def _unit(v):
    n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return v / n


def shadow_views(atlas, layout, lights, shadows):
    """SPEC 13.15 (build-defined, host numpy in f64, rounded to f32 at the end; nothing random) -> (light_views f32
    [S,4,16], enable int32 [S,4], items int32 [n,3], z_near_l): where each light of `lights` looks from, which lights cast
    shadows and the work list of ossid_scene_shadow_maps.

    Per scene the sphere (c, r) around its instances that are not the table (instance_mesh != the atlas's table): c the
    mean of their centres (the translations of their transforms, rigid ones), r the largest |centre - c| +
    atlas.radius(obj). A scene without such an instance, or with r not positive and finite, enables none of its lights;
    slots >= n_lights[s] are never enabled. With R0 = 1.05 r, Hs x Ws the map and m = min(Hs, Ws):
      directional light, d = (x, y, z) / |(x, y, z)| (|.| = 0: not enabled): eye e = c + R0 d, forward f = -d,
                         a = b = 0.5 m / R0;
      point light at p, D = |p - c| (D <= 1.1 r: not enabled -- the light sits among the objects): e = p,
                         f = (c - p) / D, a = b = 0.5 m sqrt(D D - R0 R0) / R0: the cone that touches the sphere R0.
    The up vector is the camera axis e_k with the smallest |e_k . f|, the lowest k on a tie; x = (up x f) / |up x f|,
    y = f x x; R's rows are x, y, f and t = -R e. cx = Ws / 2, cy = Hs / 2. A row is (R row-major, t, a, b, cx, cy).
    items lists, for every enabled (scene s, slot l) in ascending order, every instance i of the scene (the table
    included) in ascending order and every first face 0, 64, 128, ... below the nf of its mesh: (4 s + l, i, first)."""
    (Hs, Ws), _beta = _check_shadows(shadows)
    if not isinstance(atlas, MeshAtlas) or not isinstance(layout, Layout):
        raise ValueError("shadow_views takes a MeshAtlas and a Layout")
    if not isinstance(lights, Lights) or lights.n_scenes != layout.n_scenes:
        raise ValueError("lights must be a Lights of the layout's %d scenes" % layout.n_scenes)
    S, M = layout.n_scenes, _lib.SCENE_MAX_LIGHTS
    if layout.n_instances and (layout.instance_mesh.min() < 0 or layout.instance_mesh.max() >= atlas.n_meshes):
        raise ValueError("instance_mesh outside [0, %d)" % atlas.n_meshes)
    table = atlas.index_of[TABLE_OBJ_ID]
    radius = np.array([atlas.radius(o) for o in atlas.obj_ids], dtype=np.float64)
    views = np.zeros((S, M, 16), np.float64)
    enable = np.zeros((S, M), np.int32)
    m = float(min(Hs, Ws))
    axes = np.eye(3)
    for s in range(S):
        i0, i1 = int(layout.scene_first[s]), int(layout.scene_first[s + 1])
        objs = [i for i in range(i0, i1) if layout.instance_mesh[i] != table]
        if not objs:
            continue
        centres = layout.transforms[objs, :3, 3]
        c = centres.sum(0) / float(len(objs))
        off = centres - c
        r = float((np.sqrt((off[:, 0] * off[:, 0] + off[:, 1] * off[:, 1]) + off[:, 2] * off[:, 2])
                   + radius[layout.instance_mesh[objs]]).max())
        if not (r > 0.0 and np.isfinite(r)):
            continue
        R0 = 1.05 * r
        for l in range(int(lights.n_lights[s])):
            row = lights.lights[s, l].astype(np.float64)
            g = row[:3]
            if row[3] != 0.0:
                v = c - g
                D = float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
                if not D > 1.1 * r:
                    continue
                eye, f = g, v / D
                a = 0.5 * m * np.sqrt(D * D - R0 * R0) / R0
            else:
                if not (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2] > 0.0:
                    continue
                d = _unit(g)
                eye, f = c + R0 * d, -d
                a = 0.5 * m / R0
            up = axes[int(np.argmin(np.abs(f)))]            # argmin takes the first of equal values
            x = _unit(np.cross(up, f))
            y = np.cross(f, x)
            R = np.stack([x, y, f])
            t = -np.array([(R[k, 0] * eye[0] + R[k, 1] * eye[1]) + R[k, 2] * eye[2] for k in range(3)])
            views[s, l, :9], views[s, l, 9:12] = R.reshape(9), t
            views[s, l, 12:] = (a, a, Ws / 2.0, Hs / 2.0)
            enable[s, l] = 1
    views32 = np.ascontiguousarray(views.astype(np.float32))
    enable[~np.isfinite(views32).all(2)] = 0
    return views32, np.ascontiguousarray(enable), _shadow_items(atlas, layout, enable), SHADOW_Z_NEAR


def _shadow_items(atlas, layout, enable):
    """The work list of shadow_views for the enabled (scene, slot)s, int32 [n,3], built once per layout: the rows of a
    scene -- its instances times their groups of 64 faces, by repeats -- are the same under each of its lights, and the
    list of a layout under one `enable` is kept on the layout (callers must not write into it)."""
    nf = atlas.table_host[layout.instance_mesh, 3].astype(np.int64) if layout.n_instances else np.zeros(0, np.int64)
    key = (enable.tobytes(), layout.instance_mesh.tobytes(), layout.scene_first.tobytes(), nf.tobytes())
    kept = getattr(layout, "_shadow_items_kept", None)
    if kept is not None and kept[0] == key:
        return kept[1]
    M = _lib.SCENE_MAX_LIGHTS
    groups = (nf + SHADOW_FACES - 1) // SHADOW_FACES                          # per instance
    first_group = np.concatenate([[0], np.cumsum(groups)])
    inst = np.repeat(np.arange(layout.n_instances, dtype=np.int32), groups)    # per group of the draw list, in order
    first = ((np.arange(len(inst), dtype=np.int64) - first_group[inst]) * SHADOW_FACES).astype(np.int32)
    ls = np.nonzero(enable.reshape(-1))[0]
    lo, hi = first_group[layout.scene_first[ls // M]], first_group[layout.scene_first[ls // M + 1]]
    n = int((hi - lo).sum())
    if n > 1 << 30:
        raise ValueError("the shadow pass's work list has %d rows, at most 2^30" % n)
    items = np.empty((n, 3), np.int32)
    at = 0
    for k, a, b in zip(ls, lo, hi):                                           # at most 4 S blocks, each one slice copy
        items[at:at + b - a, 0], items[at:at + b - a, 1], items[at:at + b - a, 2] = k, inst[a:b], first[a:b]
        at += b - a
    layout._shadow_items_kept = (key, items)
    return items


class ShadowMaps:
    """The shadow maps of one (layout, lights, Shadows), device tensors, as the shadowed pass takes them: map int32
    [S,4,Hs,Ws] (the bits of the nearest f32 light-space depth, 0x7f800000 where nothing is drawn), views f32 [S,4,16],
    enable int32 [S,4], params f32 [S,2] = (beta0, beta1); size = (Hs, Ws), z_near_l and n_items, the work list's rows.
    light_scenes(shadows=...) takes one in place of a Shadows and then draws no maps of its own."""

    def __init__(self, map, views, enable, params, size, z_near_l, n_items):
        self.map, self.views, self.enable, self.params = map, views, enable, params
        self.size, self.z_near_l, self.n_items = size, z_near_l, n_items


def _shadow_maps(desc, atlas, layout, lights, d_lights, shadows):
    """shadow_views on the host, then ossid_scene_shadow_maps on the current stream -> ShadowMaps."""
    dev, S = atlas.device, layout.n_scenes
    up = lambda a: torch.from_numpy(a).to(dev)
    (Hs, Ws), beta = _check_shadows(shadows)
    views, enable, items, z_near_l = shadow_views(atlas, layout, lights, shadows)
    d_v, d_e, d_b = up(views), up(enable), up(np.tile(np.asarray(beta, np.float32), (S, 1)))
    d_items = None
    if len(items):                                         # the list is the layout's (_shadow_items): so is its upload
        kept = getattr(layout, "_shadow_items_dev", None)
        if kept is None or kept[0] is not items or kept[1].device != dev:
            kept = layout._shadow_items_dev = (items, up(items))
        d_items = kept[1]
    shadow_map = torch.empty(S, _lib.SCENE_MAX_LIGHTS, Hs, Ws, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_scene_shadow_maps")(ctypes.byref(desc), d_lights.data_ptr(), d_v.data_ptr(),
                                                      None if d_items is None else d_items.data_ptr(), len(items), Hs, Ws,
                                                      z_near_l, shadow_map.data_ptr(), _lib.stream()), "ossid_scene_shadow_maps")
    return ShadowMaps(shadow_map, d_v, d_e, d_b, (Hs, Ws), z_near_l, len(items))


def _light_pass(desc, atlas, layout, hw, albedo, instance, face, lights, material, normals, out, shadows=None):
    """ossid_scene_light on the current stream over the images of a render made with `desc` -> (lit, normal, None, None);
    with a Shadows, ossid_scene_shadow_maps and ossid_scene_light_shadowed -> (lit, normal, blocked, ShadowMaps); with a
    ShadowMaps the shadowed pass alone."""
    dev, S, (H, W) = atlas.device, layout.n_scenes, hw
    up = lambda a: torch.from_numpy(a).to(dev)
    d_l, d_n, d_a, d_m = up(lights.lights), up(lights.n_lights), up(lights.ambient), up(material)
    if d_m.numel() == 0:
        d_m = torch.zeros(1, 2, dtype=torch.float32, device=dev)             # the entry refuses NULL; no row is read
    lit = torch.empty(S, H, W, 3, dtype=torch.uint8, device=dev) if out is None else out
    normal = torch.empty(S, H, W, 3, dtype=torch.float32, device=dev)
    if shadows is None:
        with _lib.on_device(dev):
            _lib.check(_lib.fn("ossid_scene_light")(ctypes.byref(desc), normals.data_ptr(), albedo.data_ptr(),
                                                    instance.data_ptr(), face.data_ptr(), d_l.data_ptr(), d_n.data_ptr(),
                                                    d_a.data_ptr(), d_m.data_ptr(), lit.data_ptr(), normal.data_ptr(),
                                                    _lib.stream()), "ossid_scene_light")
        return lit, normal, None, None
    maps = shadows if isinstance(shadows, ShadowMaps) else _shadow_maps(desc, atlas, layout, lights, d_l, shadows)
    blocked = torch.empty(S, H, W, dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_scene_light_shadowed")(
            ctypes.byref(desc), normals.data_ptr(), albedo.data_ptr(), instance.data_ptr(), face.data_ptr(), d_l.data_ptr(),
            d_n.data_ptr(), d_a.data_ptr(), d_m.data_ptr(), maps.map.data_ptr(), maps.views.data_ptr(), maps.enable.data_ptr(),
            maps.size[0], maps.size[1], maps.z_near_l, maps.params.data_ptr(), lit.data_ptr(), normal.data_ptr(),
            blocked.data_ptr(), _lib.stream()), "ossid_scene_light_shadowed")
    return lit, normal, blocked, maps


def _lit_desc(atlas, layout, hw, pixel_offset, z_near):
    """-> (the SceneDesc the shading and shadow entries read, the tensors it points into)."""
    dev, S, I = atlas.device, layout.n_scenes, layout.n_instances
    up = lambda a: torch.from_numpy(a).to(dev)
    keep = (up(layout.instance_mesh), up(layout.transforms.astype(np.float32)), up(layout.scene_first), up(layout.cams))
    d_mesh, d_T, d_first, d_cams = keep
    desc = _lib.SceneDesc(
        vertices=atlas.vertices.data_ptr(), faces=atlas.faces.data_ptr(), meshes=atlas.table.data_ptr(),
        instance_mesh=d_mesh.data_ptr() if I else None, transforms=d_T.data_ptr() if I else None,
        scene_first=d_first.data_ptr(), cams=d_cams.data_ptr(), Vt=len(atlas.vertices_host), Ft=len(atlas.faces_host),
        K=atlas.n_meshes, I=I, S=S, H=hw[0], W=hw[1], pixel_offset=float(pixel_offset), z_near=float(z_near))
    return desc, keep


def shadow_maps(atlas, layout, hw, lights, shadows, pixel_offset=0.0, z_near=0.05):
    """SPEC 13.13 and 13.15 alone -> ShadowMaps: the maps render_scenes(lights=..., shadows=...) draws, for a caller that
    lights images of its own with light_scenes(shadows=the result), or wants the maps. Two launches."""
    H, W = _check_layout(atlas, layout, None, None, hw, pixel_offset, z_near, 1.0)
    _check_shadows(shadows, lights)
    _check_lights(layout, lights, None)
    from .model_cloud import _refuse_cpu
    _refuse_cpu(atlas.device)
    desc, _keep = _lit_desc(atlas, layout, (H, W), pixel_offset, z_near)
    return _shadow_maps(desc, atlas, layout, lights, torch.from_numpy(lights.lights).to(atlas.device), shadows)


def light_scenes(atlas, layout, hw, albedo, instance, face, lights, material=None, normals=None, out=None,
                 pixel_offset=0.0, z_near=0.05, shadows=None):
    """SPEC 13.11 on images a render of (atlas, layout, hw, pixel_offset, z_near) returned -> (lit u8 [S,H,W,3], normal
    f32 [S,H,W,3]): the deferred shading pass render_scenes(lights=...) runs, for a caller that holds the images. albedo
    u8 [S,H,W,3], instance and face int32 [S,H,W] are device tensors (SceneBatch.color, .instance, .face); material f32
    [I,2] = (k_s, e), None for no highlights; normals f32 [Vt,3] replaces atlas.normals; out may be albedo itself. The
    kernel checks instance and face: a pixel whose values lead outside an array is copied through. One launch.
    shadows: a Shadows casts shadows (SPEC 13.13-13.15: two launches for the maps, then the shadowed pass in place of
    the pass) and returns (lit, normal, blocked u8 [S,H,W]) instead; a ShadowMaps (shadow_maps) does so from maps
    already drawn, in one launch."""
    H, W = _check_layout(atlas, layout, None, None, hw, pixel_offset, z_near, 1.0)
    if isinstance(shadows, ShadowMaps):
        if tuple(shadows.map.shape[:2]) != (layout.n_scenes, _lib.SCENE_MAX_LIGHTS) or shadows.map.device != atlas.device:
            raise ValueError("light_scenes: the ShadowMaps are not of this layout's %d scenes on the atlas's device" % layout.n_scenes)
    elif shadows is not None:
        _check_shadows(shadows, lights)
    from .model_cloud import _refuse_cpu
    _refuse_cpu(atlas.device)
    dev, S, I = atlas.device, layout.n_scenes, layout.n_instances
    material = _check_lights(layout, lights, material)
    normals = atlas.normals if normals is None else normals
    for name, t, dtype, shape in (("albedo", albedo, torch.uint8, (S, H, W, 3)), ("instance", instance, torch.int32, (S, H, W)),
                                  ("face", face, torch.int32, (S, H, W)),
                                  ("normals", normals, torch.float32, (len(atlas.vertices_host), 3))) + \
            ((("out", out, torch.uint8, (S, H, W, 3)),) if out is not None else ()):
        if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous() and t.device == dev):
            raise ValueError("light_scenes: %s must be a contiguous %s tensor %s on the atlas's device" % (name, dtype, shape))
    desc, _keep = _lit_desc(atlas, layout, (H, W), pixel_offset, z_near)
    lit, normal, blocked, _map = _light_pass(desc, atlas, layout, (H, W), albedo, instance, face, lights, material, normals, out,
                                             shadows)
    return (lit, normal) if shadows is None else (lit, normal, blocked)


def work_offsets(atlas, layout):
    """int32 [I+1,2]: the prefix sums over the instances of (ossid_scene_work_items(nf), nv) of their meshes -- where an
    instance's triangle groups start in the flattened work list, and its vertex records in the workspace."""
    items = _lib.fn("ossid_scene_work_items")
    per_mesh = np.array([[items(int(nf)), int(nv)] for _v0, nv, _f0, nf in atlas.table_host], dtype=np.int64).reshape(-1, 2)
    out = np.zeros((layout.n_instances + 1, 2), dtype=np.int64)
    np.cumsum(per_mesh[layout.instance_mesh], axis=0, out=out[1:])
    if out[-1].max() > 1 << 30:
        raise ValueError("the layout makes %d triangle groups and %d vertex records, at most 2^30 each" % tuple(out[-1]))
    return np.ascontiguousarray(out.astype(np.int32))


def _check_layout(atlas, layout, sensor, background, hw, pixel_offset, z_near, depth_scale):
    if not isinstance(atlas, MeshAtlas) or not isinstance(layout, Layout):
        raise ValueError("render_scenes takes a MeshAtlas and a Layout")
    if layout.n_instances and (layout.instance_mesh.min() < 0 or layout.instance_mesh.max() >= atlas.n_meshes):
        raise ValueError("instance_mesh outside [0, %d)" % atlas.n_meshes)
    H, W = _render._check_frame(None, hw, pixel_offset, z_near)
    if not (float(depth_scale) > 0.0 and np.isfinite(depth_scale)):
        raise ValueError("depth_scale must be finite and > 0, got %r" % (depth_scale,))
    S = layout.n_scenes
    if sensor is not None and (not isinstance(sensor, Sensor) or len(sensor.thresholds) != S):
        raise ValueError("sensor must be a Sensor of the layout's %d scenes" % S)
    if background is not None:
        shape = tuple(background.shape)
        if shape not in ((H, W, 3), (1, H, W, 3), (S, H, W, 3)) or \
                (background.dtype != (torch.uint8 if torch.is_tensor(background) else np.uint8)):
            raise ValueError("background must be uint8 [H,W,3] or [S,H,W,3] = [%d,%d,%d,3], got %s %s"
                             % (S, H, W, background.dtype, shape))
    return H, W


def render_scenes(atlas, layout, hw, background=None, sensor=None, pixel_offset=0.0, z_near=0.05, depth_scale=1.0,
                  lights=None, material=None, shadows=None):
    """SPEC 13.2-13.6 -> SceneBatch of device tensors: the layout's scenes drawn with mutual occlusion, the sensor's depth
    (sensor=None: the clean sensor, quantisation only), the amodal masks and gt_info. pixel_offset 0 is this package's
    pixel convention, under which the render lines up with depth2xyz (as OnlineStream(mesh_pixel_offset=0.0) assumes).
    depth_scale is the BOP folder's: the 16-bit depth counts units of depth_scale millimetres (the atlas is in metres).
    An atlas with a textured mesh (SPEC 13.3) takes ossid_scene_render_textured and also returns lod, the mip level each
    pixel was fetched at (-1 where nothing is drawn or the winner is vertex-coloured). Seven launches on the current
    stream either way; nothing is read back.

    lights: a Lights of the layout's scenes (sample_lights, or Lights.neutral) lights the drawn pixels by one more launch
    after the render (SPEC 13.11): `color` is then the lit image, `albedo` the unlit one and `normal` f32 [S,H,W,3] the
    shading normals; material f32 [I,2] = (k_s, e) per instance, None for no highlights. Depth, instance, face, facing,
    the masks, gt_info and the sensor do not depend on the lights. With lights=None the function is the unlit one:
    the same launches, the same bits, albedo and normal None.

    shadows: a Shadows lets the lights cast shadows (SPEC 13.13-13.15): shadow_views places a view per light, two launches
    draw a depth map per (scene, light) and the shadowed pass takes the place of the shading pass. `blocked` u8 [S,H,W]
    then counts the blocked taps of each pixel's lights (0: fully lit) and `shadow_map` is the ShadowMaps drawn; both are
    None otherwise. With shadows=None the launches and bits are those of the function without it."""
    H, W = _check_layout(atlas, layout, sensor, background, hw, pixel_offset, z_near, depth_scale)
    if shadows is not None:
        _check_shadows(shadows, lights)
    from .model_cloud import _refuse_cpu
    _refuse_cpu(atlas.device)
    if lights is not None:
        material = _check_lights(layout, lights, material)
        normals = atlas.normals               # built here, ahead of the render's launches, on first use
    elif material is not None:
        raise ValueError("render_scenes: material is given without lights")
    dev = atlas.device
    S, I = layout.n_scenes, layout.n_instances
    offsets = work_offsets(atlas, layout)
    sensor = Sensor.clean(S) if sensor is None else sensor
    up = lambda a: torch.from_numpy(a).to(dev)
    d_mesh, d_T, d_first, d_cams, d_off = (up(layout.instance_mesh), up(layout.transforms.astype(np.float32)),
                                           up(layout.scene_first), up(layout.cams), up(offsets))
    d_thr, d_nr, d_rects = up(sensor.thresholds), up(sensor.n_rects), up(sensor.rects)
    bg = None
    if background is not None:
        bg = (background if torch.is_tensor(background) else torch.from_numpy(np.ascontiguousarray(background))).to(dev)
        bg = bg.reshape(-1, H, W, 3).contiguous()
    Wd = (W + 31) // 32
    color = torch.empty(S, H, W, 3, dtype=torch.uint8, device=dev)
    clean = torch.empty(S, H, W, dtype=torch.float32, device=dev)
    inst = torch.empty(S, H, W, dtype=torch.int32, device=dev)
    face = torch.empty(S, H, W, dtype=torch.int32, device=dev)
    facing = torch.empty(S, H, W, dtype=torch.float32, device=dev)
    amodal = torch.empty(I, H, Wd, dtype=torch.int32, device=dev)
    depth = torch.empty(S, H, W, dtype=torch.float32, device=dev)
    u16 = torch.empty(S, H, W, dtype=torch.uint16, device=dev)
    keep = torch.empty(S, H, W, dtype=torch.uint8, device=dev)
    gt_info = torch.empty(I, 12, dtype=torch.int32, device=dev)
    records, items = int(offsets[-1, 1]), int(offsets[-1, 0])
    need = int(_lib.fn("ossid_scene_workspace_bytes")(records, S, H, W))
    if need == 0:
        raise ValueError("render_scenes: bad sizes (%d records, %d scenes of %d x %d)" % (records, S, H, W))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    desc = _lib.SceneDesc(
        vertices=atlas.vertices.data_ptr(), colors=atlas.colors.data_ptr(), faces=atlas.faces.data_ptr(),
        meshes=atlas.table.data_ptr(), instance_mesh=d_mesh.data_ptr() if I else None,
        transforms=d_T.data_ptr() if I else None, scene_first=d_first.data_ptr(), cams=d_cams.data_ptr(),
        offsets=d_off.data_ptr(), background=None if bg is None else bg.data_ptr(), color_out=color.data_ptr(),
        depth_out=clean.data_ptr(), instance_out=inst.data_ptr(), face_out=face.data_ptr(), facing_out=facing.data_ptr(),
        amodal_out=amodal.data_ptr() if I else None, Vt=len(atlas.vertices_host), Ft=len(atlas.faces_host), K=atlas.n_meshes,
        I=I, S=S, H=H, W=W, Sb=0 if bg is None else int(bg.shape[0]), work_items=items, records=records,
        pixel_offset=float(pixel_offset), z_near=float(z_near))
    units, unit_inv = 1000.0 / float(depth_scale), float(depth_scale) / 1000.0
    lod = None
    with _lib.on_device(dev):
        if atlas.mips is None:
            _lib.check(_lib.fn("ossid_scene_render")(ctypes.byref(desc), ws.data_ptr(), ws.numel(), _lib.stream()),
                       "ossid_scene_render")
        else:
            lod = torch.empty(S, H, W, dtype=torch.int32, device=dev)
            tex = _lib.SceneTex(uvs=atlas.uvs.data_ptr(), mips=atlas.mips.data_ptr(), tex_table=atlas.tex_table.data_ptr(),
                                lod_out=lod.data_ptr(), mip_texels=atlas.mips.numel() // 4)
            _lib.check(_lib.fn("ossid_scene_render_textured")(ctypes.byref(desc), ctypes.byref(tex), ws.data_ptr(), ws.numel(),
                                                              _lib.stream()), "ossid_scene_render_textured")
        _lib.check(_lib.fn("ossid_scene_sensor")(clean.data_ptr(), facing.data_ptr(), S, H, W, d_thr.data_ptr(), d_nr.data_ptr(),
                                                 d_rects.data_ptr(), units, unit_inv, u16.data_ptr(), depth.data_ptr(),
                                                 keep.data_ptr(), _lib.stream()), "ossid_scene_sensor")
        _lib.check(_lib.fn("ossid_scene_gt_info")(amodal.data_ptr() if I else None, inst.data_ptr(), depth.data_ptr(),
                                                  d_first.data_ptr(), I, S, H, W, gt_info.data_ptr() if I else None,
                                                  _lib.stream()), "ossid_scene_gt_info")
    albedo = normal = blocked = shadow_map = None
    if lights is not None:
        albedo = color
        color, normal, blocked, shadow_map = _light_pass(desc, atlas, layout, (H, W), albedo, inst, face, lights, material,
                                                         normals, None, shadows)
    batch = SceneBatch(atlas, layout, (H, W), color, clean, depth, u16, inst, amodal, gt_info, depth_scale=depth_scale,
                       face=face, facing=facing, keep=keep, lod=lod, albedo=albedo, normal=normal, blocked=blocked,
                       shadow_map=shadow_map)
    batch.workspace_bytes = need
    return batch


def unpack_amodal(words, W):
    """Amodal bit masks int32 / uint32 [..., H, ceil(W/32)] -> bool [..., H, W]."""
    w = np.ascontiguousarray(_np(words)).view(np.uint32)
    bits = np.unpackbits(w.astype("<u4").view(np.uint8).reshape(w.shape[:-1] + (-1,)), axis=-1, bitorder="little")
    return bits[..., :W].astype(bool)


class SceneBatch:
    """What render_scenes returns; numpy arrays in place of the tensors make the same object without a device.
    color u8 [S,H,W,3]; depth_clean f32 [S,H,W] (metres, 0 = nothing drawn); depth f32 (the sensor's, metres) and
    depth_u16 (what the PNG stores: units of depth_scale millimetres); instance int32 [S,H,W] (index into the layout,
    -1 = nothing drawn); amodal int32 [I,H,ceil(W/32)] bit masks; gt_info int32 [I,12] (SPEC 13.5); optionally face,
    facing and keep; lod int32 [S,H,W] (the mip level fetched, -1 where nothing is drawn or the winner is vertex-
    coloured) from an atlas with a textured mesh, None otherwise. From a lit render (render_scenes(lights=...)) color is
    the lit image, albedo u8 [S,H,W,3] the unlit one and normal f32 [S,H,W,3] the shading normals (SPEC 13.11); both are
    None otherwise. With shadows (render_scenes(shadows=...)) blocked u8 [S,H,W] counts each pixel's blocked shadow-map
    taps and shadow_map is the ShadowMaps drawn (SPEC 13.13-13.14); both are None otherwise."""

    workspace_bytes = None

    def __init__(self, atlas, layout, hw, color, depth_clean, depth, depth_u16, instance, amodal, gt_info, depth_scale=1.0,
                 face=None, facing=None, keep=None, lod=None, albedo=None, normal=None, blocked=None, shadow_map=None):
        self.albedo, self.normal, self.blocked, self.shadow_map = albedo, normal, blocked, shadow_map
        self.atlas, self.layout, self.hw, self.depth_scale = atlas, layout, (int(hw[0]), int(hw[1])), float(depth_scale)
        self.color, self.depth_clean, self.depth, self.depth_u16 = color, depth_clean, depth, depth_u16
        self.instance, self.amodal, self.gt_info = instance, amodal, gt_info
        self.face, self.facing, self.keep, self.lod = face, facing, keep, lod
        S, I, (H, W) = layout.n_scenes, layout.n_instances, self.hw
        want = {"color": (S, H, W, 3), "depth_clean": (S, H, W), "depth": (S, H, W), "depth_u16": (S, H, W),
                "instance": (S, H, W), "amodal": (I, H, (W + 31) // 32), "gt_info": (I, 12)}
        for name, shape in want.items():
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError("SceneBatch: %s must be %s, got %s" % (name, shape, tuple(getattr(self, name).shape)))

    def _host(self):
        if getattr(self, "_host_cache", None) is None:
            H, W = self.hw
            self._host_cache = {
                "color": _np(self.color), "depth": _np(self.depth), "depth_u16": _np(self.depth_u16).view(np.uint16),
                "instance": _np(self.instance), "gt_info": _np(self.gt_info),
                "amodal": unpack_amodal(self.amodal, W).reshape(self.layout.n_instances, H, W)}
        return self._host_cache

    def _objects(self):
        """(scene, instance, index among the scene's objects) of every instance that is not the table."""
        table = self.atlas.index_of[TABLE_OBJ_ID]
        for s in range(self.layout.n_scenes):
            k = 0
            for i in range(int(self.layout.scene_first[s]), int(self.layout.scene_first[s + 1])):
                if self.layout.instance_mesh[i] != table:
                    yield s, i, k
                    k += 1

    def _frame(self, h, s, i):
        g = h["gt_info"][i]
        return {"img": h["color"][s], "depth": h["depth"][s], "cam_K": self.layout.cam_K(s),
                "obj_id": int(self.atlas.obj_ids[self.layout.instance_mesh[i]]), "pose_gt": self.layout.transforms[i].copy(),
                "mask_gt": h["amodal"][i], "mask_gt_visib": h["instance"][s] == i,
                "bbox_visib": tuple(int(v) for v in g[7:11]), "visib_fract": _visib_fract(int(g[1]), int(g[0])),
                "scene_id": s, "im_id": 0}

    def frames(self):
        """One dict per (scene, instance that is not the table), host arrays: img u8 [H,W,3], depth f32 [H,W] (the
        sensor's, metres), cam_K f64 [3,3], obj_id, pose_gt f64 [4,4], mask_gt and mask_gt_visib bool [H,W], bbox_visib
        (x, y, w, h), visib_fract, scene_id (the scene's index) and im_id (0): what OnlineStream.process,
        networkInference and pipeline.make_dtoid_sample take, less the model cloud, templates and hypotheses."""
        h = self._host()
        for s, i, _k in self._objects():
            yield self._frame(h, s, i)

    def write_bop(self, root, dataset_name, split="test", depth_scale=1.0, diameters=None, symmetries=False):
        """The standard BOP layout under <root>/<dataset_name> (millimetres): models/ and models_eval/ (obj_%06d.ply,
        vertex-coloured, or for an object the atlas draws from its texture with `comment TextureFile obj_%06d.png`,
        per-vertex texture_u texture_v and that PNG beside it; models_info.json), test_targets_bop19.json, and per scene
        <split>/%06d/ with rgb/, depth/ (16-bit), mask/,
        mask_visib/, scene_camera.json, scene_gt.json, scene_gt_info.json; every scene holds image 0. depth_scale must be
        the one the batch was rendered with. diameters: dict obj_id -> diameter in the atlas's unit; None computes them
        on the device (model_cloud.mesh_diameter). symmetries (False = off: models_info.json holds the diameter and the
        bounds only): True finds each object's symmetries from its mesh (symmetry.find_symmetries, SPEC.md section 17) and
        its entry gains `symmetries_discrete` / `symmetries_continuous`, translations and offsets in millimetres; a dict
        obj_id -> such a dict in the atlas's unit is written as given (an object without an entry gains nothing)."""
        from PIL import Image
        if float(depth_scale) != self.depth_scale:
            raise ValueError("write_bop: the batch's 16-bit depth was made with depth_scale = %r, not %r"
                             % (self.depth_scale, depth_scale))
        h = self._host()
        base = os.path.join(root, dataset_name)
        objects = [o for o in self.atlas.obj_ids if o != TABLE_OBJ_ID]
        if diameters is None:
            from .model_cloud import mesh_diameter
            diameters = {o: mesh_diameter(self.atlas.mesh_arrays(o)[0]) for o in objects}
        info = {}
        for o in objects:
            V, F, C = self.atlas.mesh_arrays(o)
            tex = self.atlas.texture_arrays(o)
            mm = V.astype(np.float64) * 1000.0
            lo, size = mm.min(0), mm.max(0) - mm.min(0)
            info[str(o)] = {"diameter": float(diameters[o]) * 1000.0, "min_x": float(lo[0]), "min_y": float(lo[1]),
                            "min_z": float(lo[2]), "size_x": float(size[0]), "size_y": float(size[1]), "size_z": float(size[2])}
            if symmetries is True:
                from .symmetry import find_symmetries
                mesh = _render.Mesh(V, F, device=self.atlas.device, colors=C, **(
                    {} if tex is None else {"uvs": tex[0], "texture": tex[1]}))
                models_info_entry(info[str(o)], find_symmetries(mesh, diameter=float(diameters[o])))
            elif symmetries:
                models_info_entry(info[str(o)], symmetries.get(o))
            for sub in ("models", "models_eval"):
                os.makedirs(os.path.join(base, sub), exist_ok=True)
                if tex is None:
                    write_ply(os.path.join(base, sub, "obj_%06d.ply" % o), mm, F, C)
                else:
                    write_ply_textured(os.path.join(base, sub, "obj_%06d.ply" % o), mm, F, tex[0], tex[1])
        for sub in ("models", "models_eval"):
            with open(os.path.join(base, sub, "models_info.json"), "w") as f:
                json.dump(info, f, indent=1)
        targets = []
        for s in range(self.layout.n_scenes):
            scene = os.path.join(base, split, "%06d" % s)
            for sub in ("rgb", "depth", "mask", "mask_visib"):
                os.makedirs(os.path.join(scene, sub), exist_ok=True)
            Image.fromarray(h["color"][s]).save(os.path.join(scene, "rgb", "%06d.png" % 0))
            Image.fromarray(h["depth_u16"][s]).save(os.path.join(scene, "depth", "%06d.png" % 0))
            gt, gt_info, count = [], [], {}
            for s2, i, k in self._objects():
                if s2 != s:
                    continue
                fr = self._frame(h, s, i)
                g = h["gt_info"][i]
                Image.fromarray(fr["mask_gt"].astype(np.uint8) * 255).save(os.path.join(scene, "mask", "%06d_%06d.png" % (0, k)))
                Image.fromarray(fr["mask_gt_visib"].astype(np.uint8) * 255).save(
                    os.path.join(scene, "mask_visib", "%06d_%06d.png" % (0, k)))
                T = fr["pose_gt"]
                gt.append({"cam_R_m2c": [float(v) for v in T[:3, :3].reshape(-1)],
                           "cam_t_m2c": [float(v) * 1000.0 for v in T[:3, 3]], "obj_id": fr["obj_id"]})
                gt_info.append({"bbox_obj": [int(v) for v in g[3:7]], "bbox_visib": [int(v) for v in g[7:11]],
                                "px_count_all": int(g[0]), "px_count_valid": int(g[2]), "px_count_visib": int(g[1]),
                                "visib_fract": fr["visib_fract"]})
                count[fr["obj_id"]] = count.get(fr["obj_id"], 0) + 1
            cam = {"0": {"cam_K": [float(v) for v in self.layout.cam_K(s).reshape(-1)], "depth_scale": self.depth_scale}}
            for name, obj in (("scene_camera.json", cam), ("scene_gt.json", {"0": gt}), ("scene_gt_info.json", {"0": gt_info})):
                with open(os.path.join(scene, name), "w") as f:
                    json.dump(obj, f, indent=1)
            targets += [{"scene_id": s, "im_id": 0, "obj_id": o, "inst_count": n} for o, n in sorted(count.items())]
        with open(os.path.join(base, "test_targets_bop19.json"), "w") as f:
            json.dump(targets, f, indent=1)
        return base


def models_info_entry(entry, symmetries, unit_to_mm=1000.0):
    """Adds an object's symmetries (symmetry.find_symmetries' dict, in the atlas's unit; None = nothing) to its
    models_info.json entry, translations and offsets in millimetres: the keys that are there keep their values and their
    place, an empty list adds no key. Returns the entry."""
    if symmetries:
        from .symmetry import scaled
        for k, v in scaled(symmetries, unit_to_mm).items():
            if v:
                entry[k] = v
    return entry


def _visib_fract(visib, amodal):
    return float(visib) / float(amodal) if amodal > 0 else 0.0


def write_ply(path, vertices, faces, colors):
    """ASCII PLY with x y z (repr of the float64) and uchar red green blue per vertex, and triangle faces."""
    V, F, C = np.asarray(vertices, dtype=np.float64), np.asarray(faces), np.asarray(colors)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                "property list uchar int vertex_indices\nend_header\n" % (len(V), len(F)))
        f.write("".join("%r %r %r %d %d %d\n" % (float(p[0]), float(p[1]), float(p[2]), c[0], c[1], c[2]) for p, c in zip(V, C)))
        f.write("".join("3 %d %d %d\n" % (t[0], t[1], t[2]) for t in F))


def write_ply_textured(path, vertices, faces, uvs, image, texture_name=None):
    """ASCII PLY with `comment TextureFile NAME`, x y z (repr of the float64) and texture_u texture_v (repr of the f32 as
    a double: it reads back to the same f32) per vertex, and triangle faces; the image u8 [Ht,Wt,3] is written beside it
    as the PNG NAME (default: the .ply's own name with .png). render.read_ply_textured returns the UVs (after
    astype(float32)) and the image byte for byte."""
    from PIL import Image
    V, F = np.asarray(vertices, dtype=np.float64), np.asarray(faces)
    U = np.asarray(uvs, dtype=np.float32)
    I = _render._check_texture(image, "write_ply_textured: image")
    if U.shape != (len(V), 2):
        raise ValueError("write_ply_textured: uvs must be [V,2] = [%d,2], got %s" % (len(V), U.shape))
    name = os.path.splitext(os.path.basename(path))[0] + ".png" if texture_name is None else str(texture_name)
    if not name.lower().endswith(".png") or os.path.basename(name) != name:
        raise ValueError("write_ply_textured: the texture is written as a PNG beside the model, got the name %r" % name)
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment TextureFile %s\nelement vertex %d\nproperty double x\nproperty double y\n"
                "property double z\nproperty float texture_u\nproperty float texture_v\nelement face %d\n"
                "property list uchar int vertex_indices\nend_header\n" % (name, len(V), len(F)))
        f.write("".join("%r %r %r %r %r\n" % (float(p[0]), float(p[1]), float(p[2]), float(t[0]), float(t[1]))
                        for p, t in zip(V, U)))
        f.write("".join("3 %d %d %d\n" % (t[0], t[1], t[2]) for t in F))
    Image.fromarray(I).save(os.path.join(os.path.dirname(os.path.abspath(path)), name))


def read_bop_frames(root, dataset_name, split="test"):
    """The frames of a BOP folder as SceneBatch.frames() yields them (depth in metres, pose_gt in metres): what
    write_bop wrote comes back bit for bit -- image, sensor depth, masks -- and the pose up to the JSON's float64."""
    from PIL import Image
    base = os.path.join(root, dataset_name, split)
    for name in sorted(os.listdir(base)):
        scene = os.path.join(base, name)
        if not (name.isdigit() and os.path.isdir(scene)):
            continue
        with open(os.path.join(scene, "scene_camera.json")) as f:
            cams = json.load(f)
        with open(os.path.join(scene, "scene_gt.json")) as f:
            gts = json.load(f)
        with open(os.path.join(scene, "scene_gt_info.json")) as f:
            infos = json.load(f)
        for im in sorted(gts, key=int):
            im_id, cam = int(im), cams[im]
            img = np.asarray(Image.open(os.path.join(scene, "rgb", "%06d.png" % im_id)).convert("RGB"))
            png = np.asarray(Image.open(os.path.join(scene, "depth", "%06d.png" % im_id)))
            depth = (png.astype(np.float64) * (float(cam.get("depth_scale", 1.0)) / 1000.0)).astype(np.float32)
            for k, (g, info) in enumerate(zip(gts[im], infos[im])):
                T = np.eye(4)
                T[:3, :3] = np.asarray(g["cam_R_m2c"], dtype=np.float64).reshape(3, 3)
                T[:3, 3] = np.asarray(g["cam_t_m2c"], dtype=np.float64) / 1000.0
                masks = [np.asarray(Image.open(os.path.join(scene, sub, "%06d_%06d.png" % (im_id, k)))) > 0
                         for sub in ("mask", "mask_visib")]
                yield {"img": img, "depth": depth, "cam_K": np.asarray(cam["cam_K"], dtype=np.float64).reshape(3, 3),
                       "obj_id": int(g["obj_id"]), "pose_gt": T, "mask_gt": masks[0], "mask_gt_visib": masks[1],
                       "bbox_visib": tuple(int(v) for v in info["bbox_visib"]), "visib_fract": float(info["visib_fract"]),
                       "scene_id": int(name), "im_id": im_id}


def read_models_dir(models_dir, scale=0.001, device=None):
    """obj_%06d.ply (or any *.ply, numbered in sorted order from 1) of a directory -> dict obj_id -> render.Mesh with
    whatever each model carries (render.load_mesh): vertex colours, a texture named by `comment TextureFile` and found
    beside the model, or both; scaled (BOP models are in millimetres)."""
    names = sorted(n for n in os.listdir(models_dir) if n.endswith(".ply"))
    if not names:
        raise ValueError("%s holds no .ply model" % models_dir)
    meshes = {}
    for k, n in enumerate(names):
        digits = "".join(c for c in os.path.splitext(n)[0] if c.isdigit())
        obj_id = int(digits) if n.startswith("obj_") and digits else k + 1
        meshes[obj_id] = _render.load_mesh(os.path.join(models_dir, n), scale=scale, device=device)
    return meshes
