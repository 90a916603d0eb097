"""Depth rendering of triangle meshes on the device (csrc/raster.hip, SPEC.md section 7), in place of the pyrender /
OpenGL rasterisation that scripts/online_learning.py reaches through zephyr.utils.renderer.Renderer:

    renderer = Renderer(K2meta(cam_K))                                             :485
    renderer.addObject(obj_id, ply_path, pose=pose, mm2m=True)                     :486-490
    renderer.obj_nodes[obj_id].matrix = pred_pose                                  :491
    color, depth = renderer.render(depth_only=True)                                :493

Renderer is the drop-in (host arrays out); render_depth is the device form that OnlineStream uses: a batch of poses in,
a device tensor out, three launches on the current stream and no host copy or synchronisation.

render_color is the same rasteriser with vertex colours (SPEC 7.11-7.12) or, for a mesh that carries UV coordinates and a
texture, with a mip-mapped bilinear texture fetch (SPEC 7.15-7.17), and render_templates makes the detector's templates out
of it (SPEC 7.13-7.14): what the reference renders offline with Blender, cuts out in datasets/render_dataset.py:251-331 and
loads in datasets/template_dataset.py:60-117. view_grid is the set of viewpoints. load_mesh reads a BOP .ply with whatever
it carries: vertex colours, a texture, or both.
"""
import os

import numpy as np
import torch

from . import _lib
from .hostutil import meta2K
from .ppf import _ply_walk


def read_ply_mesh(path, with_colors=False):
    """BOP-style PLY (ASCII or binary little-endian) -> (vertices f64 [V,3], faces int32 [F,3]). Faces come from the face
    element's list property vertex_indices (or vertex_index); polygons with more than three vertices are
    fan-triangulated (0, i, i+1). Normals are not required. with_colors=True also returns the vertex colours, u8 [V,3],
    from the properties red green blue (or diffuse_red diffuse_green diffuse_blue)."""
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
    F = np.asarray(tris, dtype=np.int32).reshape(-1, 3)
    if not with_colors:
        return V, F
    for names in (("red", "green", "blue"), ("diffuse_red", "diffuse_green", "diffuse_blue")):
        if all(k in vert for k in names):
            C = np.stack([vert[k] for k in names], 1).reshape(-1, 3)
            if C.min(initial=0.0) < 0.0 or C.max(initial=0.0) > 255.0 or np.any(C != np.rint(C)):
                raise ValueError("%s: vertex colours must be integers in [0, 255]" % path)
            return V, F, C.astype(np.uint8)
    raise ValueError("%s: the vertex element has no red green blue (or diffuse_red ...) properties" % path)


def load_mesh(path, scale=1.0, device=None):
    """A BOP .ply -> Mesh with whatever it carries (read_ply_textured): vertex colours, a texture, or both. Every refusal
    is a ValueError naming the file, before any device work."""
    m = read_ply_textured(path)
    return Mesh(m["vertices"], m["faces"], scale=scale, device=device, colors=m["colors"], uvs=m["uvs"], texture=m["texture"])


def read_ply_textured(path):
    """A BOP .ply -> {"vertices" f64 [V,3], "faces" int32 [F,3], "colors" u8 [V,3] or None, "uvs" f64 [V,2] or None,
    "texture" u8 [Ht,Wt,3] or None} on the host: vertex colours (read_ply_mesh's properties), a texture, or both.
    A texture is the image named by the header's `comment TextureFile NAME`, resolved beside the .ply and read as RGB, with
    per-vertex coordinates texture_u texture_v (or s t), or else a face-element list `texcoord` of six floats (u0 v0 u1 v1
    u2 v2, triangles only): vertices are then split, one per distinct (index, u, v) in first-seen order, the faces
    remapped, and the vertex cap checked after the split. Every refusal is a ValueError naming the file."""
    V, F = read_ply_mesh(path)
    comments = []
    vert, lists = _ply_walk(path, lists_of="face", comments=comments)
    C = None
    if all(k in vert for k in ("red", "green", "blue")) or all(k in vert for k in ("diffuse_red", "diffuse_green", "diffuse_blue")):
        C = read_ply_mesh(path, with_colors=True)[2]
    name = None
    for c in comments:
        tok = c.split(None, 1)
        if len(tok) == 2 and tok[0] == "TextureFile":
            name = tok[1].strip()
    U = None
    for ku, kv in (("texture_u", "texture_v"), ("s", "t")):
        if U is None and ku in vert and kv in vert:
            U = np.stack([vert[ku], vert[kv]], 1)
    rows = None if U is not None else lists.get("texcoord")
    if name is None or (U is None and rows is None):
        if C is None:
            raise ValueError("%s: the mesh has neither vertex colours nor a texture (comment TextureFile NAME with "
                             "texture_u texture_v, s t, or a face texcoord list)" % path)
        return {"vertices": V, "faces": F, "colors": C, "uvs": None, "texture": None}
    if rows is not None:
        idx = lists.get("vertex_indices", lists.get("vertex_index"))
        first, order, Fn = {}, [], np.empty((len(idx), 3), dtype=np.int32)
        for k, (r, tc) in enumerate(zip(idx, rows)):
            if len(r) != 3 or len(tc) != 6:
                raise ValueError("%s: face %d has %d vertices and a texcoord list of %d: a textured face is a triangle "
                                 "with six floats" % (path, k, len(r), len(tc)))
            for j in range(3):
                key = (int(r[j]), float(tc[2 * j]), float(tc[2 * j + 1]))
                if key not in first:
                    first[key] = len(order)
                    order.append(key)
                Fn[k, j] = first[key]
        if len(order) > _lib.RASTER_MAX_VERTICES:
            raise ValueError("%s: %d vertices after the split by texture coordinate, at most %d"
                             % (path, len(order), _lib.RASTER_MAX_VERTICES))
        src = np.array([k[0] for k in order], dtype=np.int64)
        U = np.array([k[1:] for k in order], dtype=np.float64).reshape(-1, 2)
        V, F, C = V[src], Fn, (None if C is None else C[src])
    if not np.isfinite(U).all():
        raise ValueError("%s: a texture coordinate is not finite" % path)
    image_path = os.path.join(os.path.dirname(os.path.abspath(path)), name)
    if not os.path.isfile(image_path):
        raise ValueError("%s: its texture %s is missing (looked for %s)" % (path, name, image_path))
    from PIL import Image
    with Image.open(image_path) as im:
        if max(im.size) > _lib.TEXTURE_MAX_SIDE:
            raise ValueError("%s: its texture %s is %d x %d, at most %d a side"
                             % (path, name, im.size[1], im.size[0], _lib.TEXTURE_MAX_SIDE))
        I = np.array(im.convert("RGB"), dtype=np.uint8)
    return {"vertices": V, "faces": F, "colors": C, "uvs": U, "texture": I}


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


def _check_colors(colors, n_vertices):
    """u8 [V,3], or floats in [0, 1] -> rint(255 c)."""
    C = np.asarray(colors)
    if C.shape != (n_vertices, 3):
        raise ValueError("colors must be [V,3] = [%d,3], got %s" % (n_vertices, C.shape))
    if C.dtype == np.uint8:
        return np.ascontiguousarray(C)
    if not np.issubdtype(C.dtype, np.floating):
        raise ValueError("colors must be uint8 or floats in [0, 1], got %s" % C.dtype)
    C = C.astype(np.float64)
    if not (np.isfinite(C).all() and C.min(initial=0.0) >= 0.0 and C.max(initial=0.0) <= 1.0):
        raise ValueError("float colors must lie in [0, 1]")
    return np.rint(255.0 * C).astype(np.uint8)


def _check_uvs(uvs, n_vertices):
    """f32 [V,2] = (u, v), v upwards; finite (values outside [0, 1] are legal: addressing clamps to the edge)."""
    U = np.asarray(uvs)
    if U.shape != (n_vertices, 2) or not (np.issubdtype(U.dtype, np.floating) or np.issubdtype(U.dtype, np.integer)):
        raise ValueError("uvs must be numbers [V,2] = [%d,2], got %s %s" % (n_vertices, U.dtype, U.shape))
    U = np.ascontiguousarray(U, dtype=np.float32)
    if not np.isfinite(U).all():
        raise ValueError("uvs must be finite")
    return U


def _check_texture(texture, what="texture"):
    """u8 [Ht,Wt,3] RGB, row 0 the top row of the image, sides in [1, TEXTURE_MAX_SIDE]."""
    I = np.asarray(texture)
    if I.ndim != 3 or I.shape[2] != 3 or I.dtype != np.uint8:
        raise ValueError("%s must be uint8 [Ht,Wt,3], got %s %s" % (what, I.dtype, I.shape))
    if not (1 <= I.shape[0] <= _lib.TEXTURE_MAX_SIDE and 1 <= I.shape[1] <= _lib.TEXTURE_MAX_SIDE):
        raise ValueError("%s: %d x %d is outside [1, %d] a side" % (what, I.shape[0], I.shape[1], _lib.TEXTURE_MAX_SIDE))
    return np.ascontiguousarray(I)


class Mesh:
    """A triangle mesh resident on the device: vertices f32(v * scale) (the product in float64), faces int32, optional
    vertex colours u8 [V,3], optional UV coordinates f32 [V,2] with a texture u8 [Ht,Wt,3] (both or neither; the mip chain
    of SPEC 7.15 is built once, here, and kept on the device as `mips`), and the rasteriser's workspaces, grown on demand.
    scale = 0.001 is the Renderer's mm2m."""

    colors = uvs = mips = None
    texture_hw = None
    _ws = _ws_color = None

    def __init__(self, vertices, faces, scale=1.0, device=None, colors=None, uvs=None, texture=None):
        V, F = _check_mesh(vertices, faces)
        C = None if colors is None else _check_colors(colors, len(V))
        if (uvs is None) != (texture is None):
            raise ValueError("a textured mesh needs both uvs and texture")
        U = None if uvs is None else _check_uvs(uvs, len(V))
        I = None if texture is None else _check_texture(texture)
        self.scale = float(scale)
        self.n_vertices, self.n_faces = len(V), len(F)
        self.device = torch.device(device) if device is not None else _lib._dev()
        self.vertices = torch.from_numpy((V * self.scale).astype(np.float32)).to(self.device).contiguous()
        self.faces = torch.from_numpy(F).to(self.device).contiguous()
        self.colors = None if C is None else torch.from_numpy(C).to(self.device).contiguous()
        self._ws = self._ws_color = None
        self.uvs = self.mips = self.texture_hw = None
        if I is not None:
            if self.device.type != "cuda":
                raise RuntimeError("a textured Mesh builds its mip chain on the GPU (got device %s)" % (self.device,))
            self.uvs =torch.from_numpy(U).to(self.device).contiguous()
            self.texture_hw = (int(I.shape[0]), int(I.shape[1]))
            image = torch.from_numpy(I).to(self.device).contiguous()
            need = int(_lib.fn("ossid_texture_mip_bytes")(*self.texture_hw))
            self.mips = torch.empty(need, dtype=torch.uint8, device=self.device)
            with _lib.on_device(self.device):
                rc = _lib.fn("ossid_texture_mips")(image.data_ptr(), self.texture_hw[0], self.texture_hw[1],
                                                   self.mips.data_ptr(), need, _lib.stream())
            _lib.check(rc, "ossid_texture_mips")

    @property
    def texture_levels(self):
        """Levels of the mip chain (the top level is texture_levels - 1); 0 without a texture."""
        return 0 if self.texture_hw is None else int(_lib.fn("ossid_texture_levels")(*self.texture_hw))

    def workspace(self, n_poses):
        need = int(_lib.fn("ossid_raster_workspace_bytes")(self.n_vertices, self.n_faces, int(n_poses)))
        if need == 0:
            raise ValueError("mesh rendering: bad sizes (V %d, F %d, N %d)" % (self.n_vertices, self.n_faces, n_poses))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def color_workspace(self, n_poses, H, W):
        need = int(_lib.fn("ossid_raster_color_workspace_bytes")(self.n_vertices, self.n_faces, int(n_poses), H, W))
        if need == 0:
            raise ValueError("mesh rendering: bad sizes (V %d, F %d, N %d, frame %d x %d)"
                             % (self.n_vertices, self.n_faces, n_poses, H, W))
        if self._ws_color is None or self._ws_color.numel() < need:
            self._ws_color = None                     # 8 bytes per sample: let go of the old one before asking for more
            self._ws_color = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws_color


def _intrinsics(cam_K):
    K = np.asarray(cam_K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("cam_K must be [3,3], got %s" % (K.shape,))
    return tuple(float(np.float32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))


def _check_frame(what, hw, pixel_offset=0.0, z_near=0.0):
    """The frame and sampling checks of every render, scenes included -> (H, W). `what` names the caller in the frame's
    message (None: nothing does)."""
    H, W = int(hw[0]), int(hw[1])
    if H <= 0 or W <= 0 or H * W > _lib.RASTER_MAX_PIXELS:
        raise ValueError("%sframe %d x %d is outside (0, %d] pixels"
                         % ("%s: " % what if what else "", H, W, _lib.RASTER_MAX_PIXELS))
    if not 0.0 <= float(pixel_offset) <= 1.0:
        raise ValueError("pixel_offset must lie in [0, 1], got %r" % (pixel_offset,))
    if not (float(z_near) >= 0.0 and np.isfinite(z_near)):
        raise ValueError("z_near must be finite and >= 0, got %r" % (z_near,))
    return H, W


def _check_call(what, poses, hw, pixel_offset, z_near):
    """The argument checks shared by render_depth and render_color -> (poses as a tensor, single, N, H, W)."""
    T = poses if torch.is_tensor(poses) else torch.from_numpy(np.asarray(poses, dtype=np.float64))
    if T.dim() not in (2, 3) or tuple(T.shape[-2:]) != (4, 4):
        raise ValueError("poses must be [4,4] or [N,4,4], got %s" % (tuple(T.shape),))
    single = T.dim() == 2
    N = 1 if single else int(T.shape[0])
    if not 1 <= N <= _lib.RASTER_MAX_POSES:
        raise ValueError("%s takes 1 to %d poses, got %d" % (what, _lib.RASTER_MAX_POSES, N))
    H, W = _check_frame(what, hw, pixel_offset, z_near)
    return T, single, N, H, W


def render_depth(mesh, poses, cam_K, hw, pixel_offset=0.5, z_near=0.05, return_stats=False):
    """Depth (camera-space Z in the mesh's scaled units, 0 = nothing drawn) of `mesh` at every pose: poses [4,4] or
    [N,4,4] (numpy, or a tensor on any device) -> f32 device tensor [H,W] or [N,H,W]; with return_stats also the int32
    device tensor [N,4] ([4]) of SPEC 7's statistics. Nothing is copied to the host and nothing waits for the device."""
    T, single, N, H, W = _check_call("render_depth", poses, hw, pixel_offset, z_near)
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


def _has_texture(mesh):
    return getattr(mesh, "mips", None) is not None and getattr(mesh, "uvs", None) is not None


def _textured(mesh, use_texture):
    """Which resolve a colour render of `mesh` takes: vertex colours when it has them, unless use_texture asks for the
    texture; the texture when that is all it has."""
    if use_texture and not _has_texture(mesh):
        raise ValueError("use_texture=True: the mesh has no texture (Mesh(..., uvs=..., texture=...), load_mesh(path))")
    return _has_texture(mesh) and (use_texture or getattr(mesh, "colors", None) is None)


def render_color(mesh, poses, cam_K, hw, pixel_offset=0.5, z_near=0.05, intrinsics=None, return_face_id=False,
                 return_stats=False, use_texture=False, return_lod=False):
    """Colour and depth of a vertex-coloured or texture-mapped `mesh` at every pose (SPEC 7.11-7.12, 7.15-7.17): poses as
    render_depth -> device tensors (color u8 [N,H,W,3], depth f32 [N,H,W][, face_id int32 [N,H,W]][, stats int32 [N,4]]
    [, lod int32 [N,H,W]]); a single [4,4] pose drops the leading axis. Colours are interpolated perspective-correctly and
    unlit; face_id is the index in the mesh's faces of the triangle seen, -1 where nothing is drawn. `intrinsics` [N,4]
    (fx, fy, cx, cy per pose) replaces cam_K, which may then be None. The depth equals render_depth's bit for bit. Nothing
    is copied to the host. A mesh with vertex colours is rendered from them; one with only a texture, or any textured one
    under use_texture=True, by a mip-mapped bilinear fetch at the perspective-correct (u, v). return_lod (textured
    renders only) adds the mip level each pixel was fetched at, -1 where nothing is drawn."""
    if getattr(mesh, "colors", None) is None and not _has_texture(mesh):
        raise ValueError("render_color: the mesh has no vertex colours and no texture (Mesh(..., colors=...) or "
                         "Mesh(..., uvs=..., texture=...), load_mesh(path))")
    textured = _textured(mesh, use_texture)
    if return_lod and not textured:
        raise ValueError("return_lod: the render is not textured (the mesh's vertex colours are used unless use_texture=True)")
    T, single, N, H, W = _check_call("render_color", poses, hw, pixel_offset, z_near)
    dev = mesh.device
    if intrinsics is None:
        key = _intrinsics(cam_K) + (N,)
        if getattr(mesh, "_cams", (None, None))[0] != key:        # kept: a repeated call uploads nothing (capturable)
            mesh._cams = (key, torch.from_numpy(np.tile(np.asarray(key[:4], dtype=np.float32), (N, 1))).to(dev))
        cams = mesh._cams[1]
    elif torch.is_tensor(intrinsics) and intrinsics.is_cuda:
        # a device tensor is used as it is and not read back; non-finite values make the pose's vertices unusable (7.2)
        if tuple(intrinsics.shape) != (N, 4):
            raise ValueError("intrinsics must be [N,4] = [%d,4] (fx, fy, cx, cy per pose), got %s" % (N, tuple(intrinsics.shape)))
        cams = intrinsics.to(dev, torch.float32).contiguous()
    else:
        cams = intrinsics.numpy() if torch.is_tensor(intrinsics) else np.asarray(intrinsics)
        if cams.shape != (N, 4):
            raise ValueError("intrinsics must be [N,4] = [%d,4] (fx, fy, cx, cy per pose), got %s" % (N, cams.shape))
        cams = np.ascontiguousarray(cams, dtype=np.float32)
        if not np.isfinite(cams).all():
            raise ValueError("intrinsics must be finite")
        cams = torch.from_numpy(cams).to(dev)
    T = T.to(dev, torch.float32).reshape(N, 4, 4).contiguous()
    ws = mesh.color_workspace(N, H, W)
    color = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    face = torch.empty(N, H, W, dtype=torch.int32, device=dev) if return_face_id else None
    stats = torch.empty(N, 4, dtype=torch.int32, device=dev) if return_stats else None
    lod = torch.empty(N, H, W, dtype=torch.int32, device=dev) if return_lod else None
    # the two entry points differ in the surface (colours | UVs and the mip chain) and in the textured one's lod_out
    head = (mesh.vertices.data_ptr(), mesh.n_vertices, mesh.faces.data_ptr() if mesh.n_faces else None, mesh.n_faces)
    frame = (T.data_ptr(), N, cams.data_ptr(), H, W, float(pixel_offset), float(z_near), ws.data_ptr(), ws.numel(),
             color.data_ptr(), depth.data_ptr(), _lib.ptr(face))
    if textured:
        what = "ossid_raster_textured"
        args = head + (mesh.uvs.data_ptr(), mesh.mips.data_ptr(), mesh.mips.numel()) + mesh.texture_hw + frame + (_lib.ptr(lod),)
    else:
        what = "ossid_raster_color"
        args = head + (mesh.colors.data_ptr(),) + frame
    with _lib.on_device(dev):
        rc = _lib.fn(what)(*args, _lib.ptr(stats), _lib.stream())
    _lib.check(rc, what)
    out = [color, depth] + ([face] if return_face_id else []) + ([stats] if return_stats else []) + \
          ([lod] if return_lod else [])
    return tuple(t[0] for t in out) if single else tuple(out)


# ---- templates from a mesh (SPEC 7.13-7.14) ------------------------------------------------------------------------------
def _icosphere_vertices(level):
    """Unit icosphere vertices in SPEC 7.14's order: the 12 of the icosahedron, then per subdivision the midpoints in
    the order the faces (and within a face the edges ab, bc, ca) first need them."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
             (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(v, dtype=np.float64) / np.sqrt(1.0 + g * g) for v in verts]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
             (9, 8, 1)]
    for _ in range(level):
        middle, nxt = {}, []
        for a, b, c in faces:
            m = []
            for i, j in ((a, b), (b, c), (c, a)):
                key = (min(i, j), max(i, j))
                if key not in middle:
                    p = verts[i] + verts[j]
                    verts.append(p / np.sqrt(p @ p))
                    middle[key] = len(verts) - 1
                m.append(middle[key])
            ab, bc, ca = m
            nxt.extend(((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)))
        faces = nxt
    return np.stack(verts)


def view_grid(level=2, inplane=1):
    """Object-to-camera rotations of the template viewpoints -> f64 [n_vertices * inplane, 3, 3]: cameras on the
    vertices p of an icosphere of subdivision `level` (12, 42, 162, 642 of them) looking at the origin. forward = -p,
    right = normalise(up x forward) with up = (0, 0, 1), or (0, 1, 0) when |up x forward| < 1e-6, down = forward x right;
    the rows of R are right, down, forward. Each view is followed by its `inplane` - 1 rotations about the optical axis
    by k 2 pi / inplane: view id = vertex * inplane + k."""
    level, inplane = int(level), int(inplane)
    if not 0 <= level <= 5:
        raise ValueError("view_grid: level must lie in [0, 5], got %d" % level)
    if inplane < 1:
        raise ValueError("view_grid: inplane must be >= 1, got %d" % inplane)
    out = []
    for p in _icosphere_vertices(level):
        fwd = -p
        right = np.cross((0.0, 0.0, 1.0), fwd)
        if np.sqrt(right @ right) < 1e-6:
            right = np.cross((0.0, 1.0, 0.0), fwd)
        right = right / np.sqrt(right @ right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        for k in range(inplane):
            a = k * 2.0 * np.pi / inplane
            c, s = (1.0, 0.0) if k == 0 else (np.cos(a), np.sin(a))
            out.append(np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ R)
    return np.stack(out)


def _frame_views(vertices, rotations, distance, cam_K, S, T, pad, z_near):
    """SPEC 7.14 in float64, on the device the (f32) vertices live on -> (intrinsics f64 [n,4] of the virtual cameras at
    S x S, template_z f64 [n]) as numpy."""
    fx, fy = float(cam_K[0][0]), float(cam_K[1][1])
    P = vertices.to(torch.float64)
    R = torch.from_numpy(rotations).to(P.device)
    m = np.empty(len(rotations))
    zmin = np.empty(len(rotations))
    for a in range(0, len(rotations), 16):                 # [16, V, 3] at a time
        C = torch.einsum("nij,vj->nvi", R[a:a + 16], P)
        Z = C[..., 2] + distance
        zmin[a:a + 16] = Z.min(1).values.cpu().numpy()
        Zs = torch.where(Z > 0, Z, torch.ones_like(Z))
        ext = torch.maximum((fx * C[..., 0] / Zs).abs(), (fy * C[..., 1] / Zs).abs())
        m[a:a + 16] = ext.max(1).values.cpu().numpy()
    if not (zmin > z_near).all():
        v = int(np.argmin(zmin))
        raise ValueError("render_templates: at distance = %g view %d has a vertex at Z = %g <= z_near = %g: raise `distance`"
                         % (distance, v, zmin[v], z_near))
    h = np.maximum(pad * m, 5.0)
    cams = np.stack([fx * S / (2.0 * h), fy * S / (2.0 * h), np.full(len(h), S / 2.0), np.full(len(h), S / 2.0)], 1)
    return cams, -distance * 2.0 * h / T


def render_templates(mesh, rotations=None, size=124, supersample=4, distance=0.8, cam_K=None, pad=1.1, z_near=0.05,
                     views_per_call=32, use_texture=False):
    """The detector's templates of a vertex-coloured or texture-mapped mesh (render_color's choice; SPEC 7.13-7.14) -> (img f32 [n,3,T,T] in [0, 1],
    mask f32 [n,1,T,T], info) on the mesh's device, T = size. View v shows the mesh under rotations[v] (default
    view_grid()) at `distance` on the optical axis, through a virtual camera derived from cam_K that frames the object
    with the margin `pad`, rendered at supersample x T and reduced by the exact box filter. info: "rotations" f64
    [n,3,3], "quats" f64 [n,4] (xyzw), "intrinsics" f32 [n,4] of the virtual cameras, "template_z" f64 [n], the value
    DtoidNet.forwardTestTime's z filter takes. views_per_call bounds the memory: 8 bytes x (supersample T)^2 per view."""
    if getattr(mesh, "colors", None) is None and not _has_texture(mesh):
        raise ValueError("render_templates: the mesh has no vertex colours and no texture (Mesh(..., colors=...) or "
                         "Mesh(..., uvs=..., texture=...), load_mesh(path))")
    _textured(mesh, use_texture)
    if cam_K is None:
        raise ValueError("render_templates: cam_K is required (the camera the templates will be matched under)")
    _intrinsics(cam_K)                                     # refuses what is not [3,3]
    K = np.asarray(cam_K, dtype=np.float64)
    T, s, per = int(size), int(supersample), int(views_per_call)
    if not 1 <= s <= 8:
        raise ValueError("supersample must lie in [1, 8], got %r" % (supersample,))
    if not 1 <= T <= 512:
        raise ValueError("size must lie in [1, 512], got %r" % (size,))
    if not 1 <= per <= _lib.RASTER_MAX_POSES:
        raise ValueError("views_per_call must lie in [1, %d], got %r" % (_lib.RASTER_MAX_POSES, views_per_call))
    if not (float(distance) > 0.0 and np.isfinite(distance)):
        raise ValueError("distance must be finite and > 0, got %r" % (distance,))
    if not (float(pad) > 0.0 and np.isfinite(pad)):
        raise ValueError("pad must be finite and > 0, got %r" % (pad,))
    _check_frame("render_templates", (s * T, s * T), 0.5, z_near)
    R = view_grid() if rotations is None else np.array(rotations, dtype=np.float64)
    if R.ndim != 3 or R.shape[1:] != (3, 3) or len(R) < 1:
        raise ValueError("rotations must be [n,3,3] with n >= 1, got %s" % (R.shape,))
    S, n = s * T, len(R)
    cams, template_z = _frame_views(mesh.vertices, R, float(distance), K, S, T, float(pad), float(z_near))
    cams = cams.astype(np.float32)
    poses = np.tile(np.eye(4), (n, 1, 1))
    poses[:, :3, :3], poses[:, 2, 3] = R, float(distance)
    dev = mesh.device
    img = torch.empty(n, 3, T, T, dtype=torch.float32, device=dev)
    mask = torch.empty(n, 1, T, T, dtype=torch.float32, device=dev)
    for a in range(0, n, per):
        b = min(n, a + per)
        color, depth = render_color(mesh, poses[a:b], None, (S, S), 0.5, z_near, intrinsics=cams[a:b], use_texture=use_texture)
        with _lib.on_device(dev):
            rc = _lib.fn("ossid_template_reduce")(color.data_ptr(), depth.data_ptr(), b - a, T, s, img[a:b].data_ptr(),
                                                  mask[a:b].data_ptr(), _lib.stream())
        _lib.check(rc, "ossid_template_reduce")
    from .pipeline import _rotmat_to_quat
    info = {"rotations": R, "quats": np.stack([_rotmat_to_quat(r) for r in R]), "intrinsics": cams, "template_z": template_z}
    return img, mask, info


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
            # the drop-in stays depth only; colour is reached through render_color / render_templates
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
