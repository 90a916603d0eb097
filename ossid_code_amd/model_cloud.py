"""The scorer's model cloud from the object's mesh, on the device (csrc/model_cloud.hip, SPEC.md section 9) -- what
scripts/online_learning.py loads from a file that neither tree can make:

    model_data_path = os.path.join(args.zephyr_model_data, "model_cloud_{:02d}.npz")   scripts/online_learning.py:303-311
    model_points, model_colors, model_normals = data["model_points"], data["model_colors"], data["model_normals"]

sample_model_cloud takes a vertex-coloured or texture-mapped render.Mesh and returns a ModelCloud: points on the surface that
is visible from outside, flat normals turned outwards by what the rasteriser saw, colours interpolated from the vertices (or
fetched from the texture at one mip level, SPEC 9.4.1), evenly spread and ordered so that every prefix is itself an even
sample. The definition is this build's own (parity with zephyr's clouds is
unpinned); every stage is bit-equal to the numpy restatement tests/ref_model_cloud.py.

The cloud is in the MESH's frame and units. A BOP .ply is in the BOP frame: a YCB-V run that takes these clouds must not
also apply modelPointsShiftYcbv2Bop. Mesh(..., scale=0.001) gives metres, the unit of the reference's clouds.
"""
import numpy as np
import torch

from . import _lib
from . import render as _render

BASE_FOCAL, PAD = 1000.0, 1.1          # 9.2: the views are framed as SPEC 7.14 frames a template


def _refuse_cpu(dev):
    if torch.device(dev).type != "cuda":
        raise RuntimeError("the OSSID hot path runs on the GPU only (got device %s)" % (dev,))


def camera_centres(rotations, distance):
    """c_v = -R_v^T t_v with t_v = (0, 0, distance), float64 [n,3]: the views' camera centres in the mesh's frame."""
    R = np.asarray(rotations, dtype=np.float64)
    t = np.array([0.0, 0.0, float(distance)])
    return np.ascontiguousarray(-(np.swapaxes(R, 1, 2) @ t))


# ---- the stages (SPEC 9.2-9.6), each one C-ABI call ---------------------------------------------------------------------------
def face_votes(mesh, face_id, centres, votes=None):
    """SPEC 9.2: face_id int32 device [n,H,W] (render_color's), centres f64 [n,3] -> votes int32 device [F,2], ADDED to
    `votes` when one is passed (chunks of views accumulate)."""
    _refuse_cpu(mesh.device)
    dev = mesh.device
    if face_id.dim() != 3 or face_id.dtype != torch.int32 or not face_id.is_cuda:
        raise ValueError("face_id must be an int32 device tensor [n,H,W], got %s %s" % (face_id.dtype, tuple(face_id.shape)))
    n, H, W = (int(v) for v in face_id.shape)
    C = np.ascontiguousarray(centres, dtype=np.float64)
    if C.shape != (n, 3) or not np.isfinite(C).all():
        raise ValueError("centres must be finite [n,3] = [%d,3], got %s" % (n, C.shape))
    if mesh.n_faces < 1 or not 1 <= n <= _lib.RASTER_MAX_POSES:
        raise ValueError("face_votes: needs F >= 1 and 1 <= n <= %d views, got F %d, n %d" % (_lib.RASTER_MAX_POSES, mesh.n_faces, n))
    if votes is None:
        votes = torch.zeros(mesh.n_faces, 2, dtype=torch.int32, device=dev)
    Cd = torch.from_numpy(C).to(dev)
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_cloud_votes")(face_id.contiguous().data_ptr(), n, H, W, mesh.vertices.data_ptr(), mesh.n_vertices,
                                          mesh.faces.data_ptr(), mesh.n_faces, Cd.data_ptr(), votes.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_cloud_votes")
    return votes


def face_weights(mesh, votes):
    """SPEC 9.3: votes int32 device [F,2] -> (weights int64 [F], prefix int64 [F], normals f32 [F,3]) on the device.
    prefix[-1] = Wt; 0 means no usable face."""
    _refuse_cpu(mesh.device)
    dev, F = mesh.device, mesh.n_faces
    if tuple(votes.shape) != (F, 2) or votes.dtype != torch.int32:
        raise ValueError("votes must be int32 [F,2] = [%d,2], got %s %s" % (F, votes.dtype, tuple(votes.shape)))
    need = int(_lib.fn("ossid_cloud_workspace_bytes")(F))
    if need == 0:
        raise ValueError("face_weights: F = %d is outside [1, %d]" % (F, _lib.RASTER_MAX_FACES))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    weights = torch.empty(F, dtype=torch.int64, device=dev)
    prefix = torch.empty(F, dtype=torch.int64, device=dev)
    normals = torch.empty(F, 3, dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_cloud_weights")(mesh.vertices.data_ptr(), mesh.n_vertices, mesh.faces.data_ptr(), F,
                                            votes.contiguous().data_ptr(), ws.data_ptr(), ws.numel(), weights.data_ptr(),
                                            prefix.data_ptr(), normals.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_cloud_weights")
    return weights, prefix, normals


def default_texture_lod(mesh, n_points):
    """SPEC 9.4.1's host rule, f64: the smallest mip level whose texel on the surface is at least half the cloud's nominal
    spacing sqrt(total area / n_points). The texel of level l measures 2^l x the median over the faces with positive UV
    area of sqrt(area_3d / area_uv_texels), area_uv_texels the face's UV area times Ht Wt. At most the top level; 0 when
    no face has a positive UV area."""
    P = mesh.vertices.cpu().numpy().astype(np.float64)
    uv = mesh.uvs.cpu().numpy().astype(np.float64)
    Fc = mesh.faces.cpu().numpy().astype(np.int64)
    Ht, Wt = mesh.texture_hw
    g = np.cross(P[Fc[:, 1]] - P[Fc[:, 0]], P[Fc[:, 2]] - P[Fc[:, 0]])
    a3 = 0.5 * np.sqrt((g * g).sum(1))
    e1, e2 = uv[Fc[:, 1]] - uv[Fc[:, 0]], uv[Fc[:, 2]] - uv[Fc[:, 0]]
    at = 0.5 * np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) * float(Wt) * float(Ht)
    pos = np.isfinite(at) & (at > 0.0) & np.isfinite(a3)
    if not pos.any():
        return 0
    texel = float(np.median(np.sqrt(a3[pos] / at[pos])))
    spacing = float(np.sqrt(a3[np.isfinite(a3)].sum() / float(n_points)))
    lod, top = 0, mesh.texture_levels - 1
    while lod < top and texel < 0.5 * spacing:         # exact doublings: no logarithm
        texel, lod = 2.0 * texel, lod + 1
    return lod


def face_candidates(mesh, votes, prefix, normals, K, use_texture=False, texture_lod=0):
    """SPEC 9.4: K stratified samples of the weighted faces -> dict of device tensors: points f32 [K,3], normals f32 [K,3],
    colors f32 [K,3] in [0, 1], face int32 [K]. The colours come from the vertex colours, or (a mesh with only a texture,
    or use_texture=True) from the texture at mip level texture_lod (SPEC 9.4.1)."""
    _refuse_cpu(mesh.device)
    dev, F, K = mesh.device, mesh.n_faces, int(K)
    if not 1 <= K <= _lib.CLOUD_MAX_CANDIDATES:
        raise ValueError("K must lie in [1, %d], got %d" % (_lib.CLOUD_MAX_CANDIDATES, K))
    if mesh.colors is None and not _render._has_texture(mesh):
        raise ValueError("face_candidates: the mesh has no vertex colours and no texture")
    if _render._textured(mesh, use_texture):
        lod = int(texture_lod)
        if not 0 <= lod < mesh.texture_levels:
            raise ValueError("texture_lod must lie in [0, %d], got %r" % (mesh.texture_levels - 1, texture_lod))
        out = {"points": torch.empty(K, 3, dtype=torch.float32, device=dev), "normals": torch.empty(K, 3, dtype=torch.float32, device=dev),
               "colors": torch.empty(K, 3, dtype=torch.float32, device=dev), "face": torch.empty(K, dtype=torch.int32, device=dev)}
        with _lib.on_device(dev):
            rc = _lib.fn("ossid_cloud_candidates_textured")(
                mesh.vertices.data_ptr(), mesh.n_vertices, mesh.faces.data_ptr(), F, mesh.uvs.data_ptr(), mesh.mips.data_ptr(),
                mesh.mips.numel(), mesh.texture_hw[0], mesh.texture_hw[1], lod, votes.contiguous().data_ptr(), prefix.data_ptr(),
                normals.data_ptr(), K, out["points"].data_ptr(), out["normals"].data_ptr(), out["colors"].data_ptr(),
                out["face"].data_ptr(), _lib.stream())
        _lib.check(rc, "ossid_cloud_candidates_textured")
        return out
    out = {"points": torch.empty(K, 3, dtype=torch.float32, device=dev), "normals": torch.empty(K, 3, dtype=torch.float32, device=dev),
           "colors": torch.empty(K, 3, dtype=torch.float32, device=dev), "face": torch.empty(K, dtype=torch.int32, device=dev)}
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_cloud_candidates")(mesh.vertices.data_ptr(), mesh.n_vertices, mesh.faces.data_ptr(), F,
                                               mesh.colors.data_ptr(), votes.contiguous().data_ptr(), prefix.data_ptr(),
                                               normals.data_ptr(), K, out["points"].data_ptr(), out["normals"].data_ptr(),
                                               out["colors"].data_ptr(), out["face"].data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_cloud_candidates")
    return out


def fps(points, m):
    """SPEC 9.5: farthest-point sampling of m of the K <= 32768 points [K,3] (numpy or tensor, cast to f32), from point 0,
    the lowest index among equal maxima -> (selection int32 [m] in pick order, radius f32 [m]) on the device; radius[j] is
    the largest squared distance to the earlier picks when pick j was chosen, radius[0] = +inf. Non-finite points are
    refused."""
    P = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32))
    if P.dim() != 2 or P.shape[1] != 3:
        raise ValueError("points must be [K,3], got %s" % (tuple(P.shape),))
    K, m = int(P.shape[0]), int(m)
    if not 1 <= m <= _lib.CLOUD_MAX_POINTS or not m <= K <= _lib.CLOUD_MAX_CANDIDATES:
        raise ValueError("fps: needs 1 <= m <= %d and m <= K <= %d, got m = %d, K = %d"
                         % (_lib.CLOUD_MAX_POINTS, _lib.CLOUD_MAX_CANDIDATES, m, K))
    P = P.to(torch.float32)
    if not bool(torch.isfinite(P).all()):
        raise ValueError("fps: the points must be finite")
    if not P.is_cuda:
        P = P.to(_lib._dev())
    P = P.contiguous()
    sel = torch.empty(m, dtype=torch.int32, device=P.device)
    rad = torch.empty(m, dtype=torch.float32, device=P.device)
    with _lib.on_device(P.device):
        rc = _lib.fn("ossid_cloud_fps")(P.data_ptr(), K, m, sel.data_ptr(), rad.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_cloud_fps")
    return sel, rad


def mesh_diameter(mesh):
    """SPEC 9.6: the largest distance between two vertices (what models_info.json calls `diameter`), float, in the mesh's
    scaled units. mesh: a render.Mesh, or vertices [V,3] (cast to f32). V <= 262144."""
    if isinstance(mesh, _render.Mesh):
        P = mesh.vertices
    else:
        P = mesh if torch.is_tensor(mesh) else torch.from_numpy(np.asarray(mesh, dtype=np.float64).astype(np.float32))
        if P.dim() != 2 or P.shape[1] != 3:
            raise ValueError("vertices must be [V,3], got %s" % (tuple(P.shape),))
    V = int(P.shape[0])
    if not 1 <= V <= _lib.MESH_DIAMETER_MAX_VERTICES:
        raise ValueError("mesh_diameter takes 1 to %d vertices, got %d" % (_lib.MESH_DIAMETER_MAX_VERTICES, V))
    if not P.is_cuda:
        if isinstance(mesh, _render.Mesh):
            _refuse_cpu(P.device)
        P = P.to(_lib._dev())
    P = P.to(torch.float32).contiguous()
    out = torch.empty(2, dtype=torch.float64, device=P.device)
    with _lib.on_device(P.device):
        rc = _lib.fn("ossid_mesh_diameter")(P.data_ptr(), V, out.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_mesh_diameter")
    return float(out[1])


# ---- the cloud ----------------------------------------------------------------------------------------------------------------
class ModelCloud:
    """model_points / model_normals / model_colors: f32 [M,3] device tensors in pick order (any prefix is an even sample),
    colours RGB in [0, 1]; diameter: the mesh's (SPEC 9.6), in the same units."""

    def __init__(self, model_points, model_normals, model_colors, diameter):
        self.model_points, self.model_normals, self.model_colors = model_points, model_normals, model_colors
        self.diameter = float(diameter)

    def __len__(self):
        return int(self.model_points.shape[0])

    def as_dict(self):
        """The keys scoring.networkInference takes."""
        return {"model_points": self.model_points, "model_normals": self.model_normals, "model_colors": self.model_colors}

    def save(self, path):
        """The reference's model_cloud_XX.npz: model_points / model_colors / model_normals as float64 [M,3], plus
        `diameter`."""
        np.savez(path, model_points=self.model_points.cpu().numpy().astype(np.float64),
                 model_colors=self.model_colors.cpu().numpy().astype(np.float64),
                 model_normals=self.model_normals.cpu().numpy().astype(np.float64), diameter=np.float64(self.diameter))


def _check_caps(mesh, n_points, oversample, level, view_size, views_per_call, use_texture=False, texture_lod=None):
    """SPEC 9.1, before any launch -> (M, K, level, S, views per call)."""
    M, over, level, S, per = int(n_points), int(oversample), int(level), int(view_size), int(views_per_call)
    if not 1 <= M <= _lib.CLOUD_MAX_POINTS:
        raise ValueError("n_points must lie in [1, %d], got %r" % (_lib.CLOUD_MAX_POINTS, n_points))
    if over < 1 or over * M > _lib.CLOUD_MAX_CANDIDATES:
        raise ValueError("oversample * n_points must lie in [n_points, %d], got %r * %d" % (_lib.CLOUD_MAX_CANDIDATES, oversample, M))
    if not 0 <= level <= 3:
        raise ValueError("level must lie in [0, 3], got %r" % (level,))
    if not 16 <= S <= 1024:
        raise ValueError("view_size must lie in [16, 1024], got %r" % (view_size,))
    if not 1 <= per <= _lib.RASTER_MAX_POSES:
        raise ValueError("views_per_call must lie in [1, %d], got %r" % (_lib.RASTER_MAX_POSES, views_per_call))
    if not isinstance(mesh, _render.Mesh) or (getattr(mesh, "colors", None) is None and not _render._has_texture(mesh)):
        raise ValueError("sample_model_cloud: needs a render.Mesh with vertex colours or a texture (Mesh(..., colors=...), "
                         "Mesh(..., uvs=..., texture=...), load_mesh(path))")
    if _render._textured(mesh, use_texture) and texture_lod is not None and not 0 <= int(texture_lod) < mesh.texture_levels:
        raise ValueError("texture_lod must lie in [0, %d], got %r" % (mesh.texture_levels - 1, texture_lod))
    if mesh.n_faces < 1:
        raise ValueError("sample_model_cloud: the mesh has no faces")
    if not bool(torch.isfinite(mesh.vertices).all()):
        raise ValueError("sample_model_cloud: the mesh has a non-finite vertex")
    return M, over * M, level, S, per


def sample_model_cloud(mesh, n_points=2048, oversample=16, level=2, view_size=512, views_per_call=32, return_info=False,
                       use_texture=False, texture_lod=None):
    """SPEC section 9: a vertex-coloured or texture-mapped render.Mesh -> ModelCloud of n_points points (with return_info
    also the dict below). A mesh with only a texture, or any textured one under use_texture=True, takes its colours from
    the texture at mip level texture_lod (None: default_texture_lod's rule, SPEC 9.4.1; info["texture_lod"] tells). The mesh is rendered from the view_grid(level) viewpoints at view_size^2; a face takes part iff some sample
    shows it, its normal points to the side it was seen from, K = oversample * n_points candidates are spread over the
    faces by area, and farthest-point sampling keeps n_points of them, in pick order.

    info: "votes" int32 [F,2], "weights" / "prefix" int64 [F], "face_normals" f32 [F,3], "candidates" {points, normals,
    colors, face}, "selection" int32 [M], "radius" f32 [M] (device tensors); "rotations" f64 [n,3,3], "intrinsics" f32
    [n,4] (fx, fy, cx, cy of the virtual cameras), "distance", "z_near" (floats), "centres" f64 [n,3] (numpy)."""
    M, K, level, S, per = _check_caps(mesh, n_points, oversample, level, view_size, views_per_call, use_texture, texture_lod)
    _refuse_cpu(mesh.device)
    dev = mesh.device
    textured = _render._textured(mesh, use_texture)
    lod = None if not textured else (default_texture_lod(mesh, M) if texture_lod is None else int(texture_lod))
    P = mesh.vertices.cpu().numpy().astype(np.float64)
    r = float(np.sqrt((P * P).sum(1).max()))
    if not r > 0.0:
        raise ValueError("sample_model_cloud: no usable face (every vertex lies at the origin)")
    R = _render.view_grid(level)
    distance, z_near = 4.0 * r, r
    base = np.array([[BASE_FOCAL, 0.0, 0.0], [0.0, BASE_FOCAL, 0.0], [0.0, 0.0, 1.0]])
    cams, _tz = _render._frame_views(mesh.vertices, R, distance, base, S, S, PAD, z_near)
    cams = cams.astype(np.float32)
    centres = camera_centres(R, distance)
    poses = np.tile(np.eye(4), (len(R), 1, 1))
    poses[:, :3, :3], poses[:, 2, 3] = R, distance
    votes = torch.zeros(mesh.n_faces, 2, dtype=torch.int32, device=dev)
    for a in range(0, len(R), per):
        b = min(len(R), a + per)
        _c, _d, face_id = _render.render_color(mesh, poses[a:b], None, (S, S), 0.5, z_near, intrinsics=cams[a:b],
                                               return_face_id=True, use_texture=use_texture)
        face_votes(mesh, face_id, centres[a:b], votes)
    weights, prefix, normals = face_weights(mesh, votes)
    if int(prefix[-1]) == 0:
        raise ValueError("sample_model_cloud: no usable face (none was seen, or every face that was seen has no area)")
    cand = face_candidates(mesh, votes, prefix, normals, K, use_texture=use_texture, texture_lod=lod or 0)
    selection, radius = fps(cand["points"], M)
    idx = selection.long()
    # 9.6 has a cap of its own: a larger mesh still gets its cloud, without a diameter
    diameter = mesh_diameter(mesh) if mesh.n_vertices <= _lib.MESH_DIAMETER_MAX_VERTICES else float("nan")
    cloud = ModelCloud(cand["points"][idx], cand["normals"][idx], cand["colors"][idx], diameter)
    if not return_info:
        return cloud
    info = {"votes": votes, "weights": weights, "prefix": prefix, "face_normals": normals, "candidates": cand,
            "selection": selection, "radius": radius, "rotations": R, "intrinsics": cams, "distance": distance,
            "z_near": z_near, "centres": centres, "texture_lod": lod}
    return cloud, info
