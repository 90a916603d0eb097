"""Depth rendering of triangle meshes on the device (csrc/raster.hip, SPEC.md section 7), in place of the pyrender /
OpenGL rasterisation that scripts/online_learning.py reaches through zephyr.utils.renderer.Renderer:

    renderer = Renderer(K2meta(cam_K))                                             :485
    renderer.addObject(obj_id, ply_path, pose=pose, mm2m=True)                     :486-490
    renderer.obj_nodes[obj_id].matrix = pred_pose                                  :491
    color, depth = renderer.render(depth_only=True)                                :493

Renderer is the drop-in (host arrays out); render_depth is the device form that OnlineStream uses: a batch of poses in,
a device tensor out, three launches on the current stream and no host copy or synchronisation.
"""
import numpy as np
import torch

from . import _lib
from .hostutil import meta2K
from .ppf import _ply_walk


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def read_ply_mesh(path):
    """BOP-style PLY (ASCII or binary little-endian) -> (vertices f64 [V,3], faces int32 [F,3]). Faces come from the face
    element's list property vertex_indices (or vertex_index); polygons with more than three vertices are
    fan-triangulated (0, i, i+1). Normals are not required."""
    vert, lists = _ply_walk(path, lists_of="face")
    if vert is None:
        raise ValueError("%s: no vertex element" % path)
    missing = [k for k in ("x", "y", "z") if k not in vert]
    if missing:
        raise ValueError("%s: the vertex element lacks %s" % (path, " ".join(missing)))
    V = np.stack([vert["x"], vert["y"], vert["z"]], 1).reshape(-1, 3)
    if lists is None:
        raise ValueError("%s: no face element (a mesh is needed to render)" % path)
    rows = lists.get("vertex_indices", lists.get("vertex_index"))
    if rows is None:
        raise ValueError("%s: the face element has no vertex_indices / vertex_index list" % path)
    tris = []
    for k, r in enumerate(rows):
        if len(r) < 3:
            raise ValueError("%s: face %d has %d vertices" % (path, k, len(r)))
        if r.min() < 0 or r.max() >= len(V):
            raise ValueError("%s: face %d has a vertex index outside [0, %d)" % (path, k, len(V)))
        for i in range(1, len(r) - 1):
            tris.append((r[0], r[i], r[i + 1]))
    return V, np.asarray(tris, dtype=np.int32).reshape(-1, 3)


def _check_mesh(vertices, faces):
    V = np.asarray(vertices, dtype=np.float64)
    if V.ndim != 2 or V.shape[1] != 3 or len(V) < 1:
        raise ValueError("vertices must be [V,3] with V >= 1, got %s" % (V.shape,))
    F = np.asarray(faces)
    if F.size == 0:
        F = np.zeros((0, 3), dtype=np.int64)
    if F.ndim != 2 or F.shape[1] != 3 or not np.issubdtype(F.dtype, np.integer):
        raise ValueError("faces must be integers [F,3], got %s %s" % (F.dtype, F.shape))
    if len(V) > _lib.RASTER_MAX_VERTICES or len(F) > _lib.RASTER_MAX_FACES:
        raise ValueError("a mesh has at most %d vertices and %d faces, got %d and %d"
                         % (_lib.RASTER_MAX_VERTICES, _lib.RASTER_MAX_FACES, len(V), len(F)))
    if len(F) and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError("face index outside [0, %d)" % len(V))
    return V, np.ascontiguousarray(F, dtype=np.int32)


class Mesh:
    """A triangle mesh resident on the device: vertices f32(v * scale) (the product in float64), faces int32, and the
    rasteriser's workspace, grown on demand. scale = 0.001 is the Renderer's mm2m."""

    def __init__(self, vertices, faces, scale=1.0, device=None):
        V, F = _check_mesh(vertices, faces)
        self.scale = float(scale)
        self.n_vertices, self.n_faces = len(V), len(F)
        self.device = torch.device(device) if device is not None else _dev()
        self.vertices = torch.from_numpy((V * self.scale).astype(np.float32)).to(self.device).contiguous()
        self.faces = torch.from_numpy(F).to(self.device).contiguous()
        self._ws = None

    def workspace(self, n_poses):
        need = int(_lib.fn("ossid_raster_workspace_bytes")(self.n_vertices, self.n_faces, int(n_poses)))
        if need == 0:
            raise ValueError("mesh rendering: bad sizes (V %d, F %d, N %d)" % (self.n_vertices, self.n_faces, n_poses))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws


def _intrinsics(cam_K):
    K = np.asarray(cam_K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("cam_K must be [3,3], got %s" % (K.shape,))
    return tuple(float(np.float32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def render_depth(mesh, poses, cam_K, hw, pixel_offset=0.5, z_near=0.05, return_stats=False):
    """Depth (camera-space Z in the mesh's scaled units, 0 = nothing drawn) of `mesh` at every pose: poses [4,4] or
    [N,4,4] (numpy, or a tensor on any device) -> f32 device tensor [H,W] or [N,H,W]; with return_stats also the int32
    device tensor [N,4] ([4]) of SPEC 7's statistics. Nothing is copied to the host and nothing waits for the device."""
    T = poses if torch.is_tensor(poses) else torch.from_numpy(np.asarray(poses, dtype=np.float64))
    if T.dim() not in (2, 3) or tuple(T.shape[-2:]) != (4, 4):
        raise ValueError("poses must be [4,4] or [N,4,4], got %s" % (tuple(T.shape),))
    single = T.dim() == 2
    N = 1 if single else int(T.shape[0])
    H, W = int(hw[0]), int(hw[1])
    if not 1 <= N <= _lib.RASTER_MAX_POSES:
        raise ValueError("render_depth takes 1 to %d poses, got %d" % (_lib.RASTER_MAX_POSES, N))
    if H <= 0 or W <= 0 or H * W > _lib.RASTER_MAX_PIXELS:
        raise ValueError("render_depth: frame %d x %d is outside (0, %d] pixels" % (H, W, _lib.RASTER_MAX_PIXELS))
    if not 0.0 <= float(pixel_offset) <= 1.0:
        raise ValueError("pixel_offset must lie in [0, 1], got %r" % (pixel_offset,))
    if not (float(z_near) >= 0.0 and np.isfinite(z_near)):
        raise ValueError("z_near must be finite and >= 0, got %r" % (z_near,))
    fx, fy, cx, cy = _intrinsics(cam_K)
    dev = mesh.device
    T = T.to(dev, torch.float32).reshape(N, 4, 4).contiguous()
    ws = mesh.workspace(N)
    depth = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    stats = torch.empty(N, 4, dtype=torch.int32, device=dev) if return_stats else None
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_raster_depth")(mesh.vertices.data_ptr(), mesh.n_vertices,
                                           mesh.faces.data_ptr() if mesh.n_faces else None, mesh.n_faces, T.data_ptr(), N,
                                           fx, fy, cx, cy, H, W, float(pixel_offset), float(z_near), ws.data_ptr(),
                                           ws.numel(), depth.data_ptr(), None if stats is None else stats.data_ptr(),
                                           _lib.stream())
    _lib.check(rc, "ossid_raster_depth")
    if single:
        depth, stats = depth[0], (None if stats is None else stats[0])
    return (depth, stats) if return_stats else depth


class _Node:
    """What obj_nodes[obj_id] is to the caller: a holder of the object's pose (`matrix`, 4x4, assignable)."""

    def __init__(self, matrix):
        self.matrix = matrix

    @property
    def matrix(self):
        return self._matrix

    @matrix.setter
    def matrix(self, value):
        M = np.array(value, dtype=np.float64, copy=True)
        if M.shape != (4, 4):
            raise ValueError("a pose is [4,4], got %s" % (M.shape,))
        self._matrix = M


class Renderer:
    """zephyr.utils.renderer.Renderer as online_learning.py:485-493 uses it, depth only. meta_data is hostutil.K2meta's
    dict. Meshes are read and uploaded at the first render (addObject itself needs no device)."""

    def __init__(self, meta_data, width=640, height=480):
        self.K = meta2K(meta_data)
        self.width, self.height = int(width), int(height)
        self.obj_nodes, self.obj_paths, self.obj_scales, self._meshes = {}, {}, {}, {}

    def addObject(self, obj_id, model_path, pose=None, mm2m=False, simplify=False):
        """mm2m=True scales the model by 0.001 (millimetres to metres). `simplify` is accepted and ignored: this build
        renders the mesh as it is stored."""
        self.obj_nodes[obj_id] = _Node(np.eye(4) if pose is None else pose)
        self.obj_paths[obj_id] = model_path
        self.obj_scales[obj_id] = 0.001 if mm2m else 1.0
        self._meshes.pop(obj_id, None)

    def _mesh(self, obj_id):
        if obj_id not in self.obj_nodes:
            raise KeyError("Renderer: no object %r (addObject first)" % (obj_id,))
        if obj_id not in self._meshes:
            V, F = read_ply_mesh(self.obj_paths[obj_id])
            self._meshes[obj_id] = Mesh(V, F, scale=self.obj_scales[obj_id])
        return self._meshes[obj_id]

    def render(self, depth_only=False):
        """-> (None, depth f32 numpy [H,W] in the scaled units, 0 = background). Several objects share one image: the
        nearest positive depth per pixel."""
        if not depth_only:
            raise ValueError("Renderer.render: depth_only=False is not supported (this build renders depth only; "
                             "scripts/online_learning.py:493 passes depth_only=True)")
        out = None
        for obj_id, node in self.obj_nodes.items():
            d = render_depth(self._mesh(obj_id), node.matrix, self.K, (self.height, self.width))
            if out is None:
                out = d
            else:
                out = torch.where((d > 0) & ((out == 0) | (d < out)), d, out)
        if out is None:
            return None, np.zeros((self.height, self.width), dtype=np.float32)
        return None, out.cpu().numpy()


def blend(a, b, alpha=0.5):
    """Placeholder for zephyr.utils.renderer.blend, set by compat.install(renderer=True) only when no real module
    imports: a plain alpha blend of two images. The reference's loop imports the name and never calls it; how close this
    is to zephyr's own is unknown."""
    return np.asarray(a, dtype=np.float64) * (1.0 - alpha) + np.asarray(b, dtype=np.float64) * alpha
