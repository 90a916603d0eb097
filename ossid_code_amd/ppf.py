"""Point-pair-feature pose hypotheses on the device (csrc/ppf.hip, SPEC.md section 6), in place of MVTec Halcon's surface
matching that scripts/online_learning.py reaches through zephyr.utils.halcon_wrapper.PPFModel:

    PPFModel(full_model_path[, ModelSamplingDist=0.03])                                           :295-301
    poses, scores, seconds = ppf_model.find_surface_model(scene_pc * 1000.0[, DensePoseRefinement='false',
                                                          SceneSamplingDist=0.03, RefPtRate=0.2])  :418 / :446

DensePoseRefinement='true' refines every hypothesis against the scene (csrc/ppf_refine.hip, SPEC.md 6.9); the drop-in's
default stays 'false', compat.install(ppf=True, ppf_dense_refinement=True) maps PPFModelDense, whose default is Halcon's
'true'.

find_surface_model is the drop-in (host arrays in, host arrays out, the caller's units); find_hypotheses is the device
form that OnlineStream uses: depth image + mask in, device tensors out, one launch chain and no host copy.
"""
import os
import time

import numpy as np
import torch

from . import _lib

NORMAL_RADIUS_REL = 2.0          # SPEC 6.3: scene normal radius in units of the scene sampling step
REFINE_SAMPLING_REL = 0.02       # SPEC 6.9: refinement sampling step in units of D
REFINE_STEPS = 5
ACCEPTED = ("SceneSamplingDist", "RefPtRate", "NumResult", "DensePoseRefinement", "PoseClusterDistRel", "NormalRadiusRel")


def dense_flag(v):
    """DensePoseRefinement: 'true' / 'false' in any letter case or a bool -> bool; anything else raises."""
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, str) and v.lower() in ("true", "false"):
        return v.lower() == "true"
    raise ValueError("find_surface_model: DensePoseRefinement=%r is not 'true' or 'false'" % (v,))


def _f32(a, dev):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    return t.to(dev, torch.float32).contiguous()


def _call(name, *args):
    with torch.cuda.device(_lib._dev()):
        rc = _lib.fn(name)(*args)
    _lib.check(rc, name)


def _ply_walk(path, lists_of=None, comments=None):
    """The header / body walk shared by read_ply, render.read_ply_mesh and render.load_mesh -> (vertex columns
    {name: f64 [V]} or None, {property name: list of arrays, one per row -- int64, or f64 for a list of floats} of the list
    properties of element `lists_of`, or None when that element is absent / not asked for). Elements and properties nobody
    asked for are skipped. The text of every `comment` line of the header is appended to `comments` when a list is passed
    (BOP names a model's texture in `comment TextureFile NAME`)."""
    types = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
             "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
             "double": "f8", "float64": "f8"}
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: PLY header without end_header" % path)
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                if tok and tok[0] == "comment" and comments is not None:
                    comments.append(line.decode("ascii", "replace").strip()[len("comment"):].strip())
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append([tok[1], int(tok[2]), []])
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1][2].append((tok[4], ("list", types[tok[2]], types[tok[3]])))
                else:
                    elements[-1][2].append((tok[2], types[tok[1]]))
            elif tok[0] == "end_header":
                break
        if fmt not in ("ascii", "binary_little_endian"):
            raise ValueError("%s: PLY format %r is not supported (ascii, binary_little_endian)" % (path, fmt))
        body = f.read()
    vert, lists = None, None
    if fmt == "ascii":
        lines = body.decode("ascii").split("\n")
        pos = 0
        for name, n, props in elements:
            rows = []
            for _ in range(n):
                while not lines[pos].strip():
                    pos += 1
                rows.append(lines[pos].split())
                pos += 1
            if name == "vertex":
                names = [p[0] for p in props]
                if any(isinstance(p[1], tuple) for p in props):
                    raise ValueError("%s: list property on the vertex element" % path)
                vert = {nm: np.array([float(r[k]) for r in rows]) for k, nm in enumerate(names)}
            elif name == lists_of:
                lists = {p[0]: [] for p in props if isinstance(p[1], tuple)}
                for r in rows:
                    k = 0
                    for pn, t in props:
                        if isinstance(t, tuple):
                            cnt = int(r[k])
                            if t[2] in ("f4", "f8"):
                                lists[pn].append(np.array([float(q) for q in r[k + 1:k + 1 + cnt]], dtype=np.float64))
                            else:
                                lists[pn].append(np.array([int(float(q)) for q in r[k + 1:k + 1 + cnt]], dtype=np.int64))
                            k += 1 + cnt
                        else:
                            k += 1
    else:
        pos = 0
        for name, n, props in elements:
            if all(not isinstance(p[1], tuple) for p in props):
                dt = np.dtype([(p[0], "<" + p[1]) for p in props])
                arr = np.frombuffer(body, dtype=dt, count=n, offset=pos)
                pos += n * dt.itemsize
                if name == "vertex":
                    vert = {nm: arr[nm].astype(np.float64) for nm in dt.names}
            else:
                if name == "vertex":
                    raise ValueError("%s: list property on the vertex element" % path)
                keep = name == lists_of
                if keep:
                    lists = {p[0]: [] for p in props if isinstance(p[1], tuple)}
                for _ in range(n):
                    for pn, t in props:
                        if isinstance(t, tuple):
                            cnt = np.frombuffer(body, dtype="<" + t[1], count=1, offset=pos)[0]
                            pos += np.dtype(t[1]).itemsize
                            if keep:
                                lists[pn].append(np.frombuffer(body, dtype="<" + t[2], count=int(cnt), offset=pos)
                                                 .astype(np.float64 if t[2] in ("f4", "f8") else np.int64))
                            pos += int(cnt) * np.dtype(t[2]).itemsize
                        else:
                            pos += np.dtype(t).itemsize
    return vert, lists


def read_ply(path):
    """BOP-style PLY (ASCII or binary little-endian) -> (points f64 [V,3], normals f64 [V,3]) from the vertex element's
    x y z nx ny nz; every other element and property (faces, colours, texture coordinates) is skipped."""
    vert, _ = _ply_walk(path)
    if vert is None:
        raise ValueError("%s: no vertex element" % path)
    missing = [k for k in ("x", "y", "z", "nx", "ny", "nz") if k not in vert]
    if missing:
        raise ValueError("%s: the vertex element lacks %s (PPF needs x y z nx ny nz)" % (path, " ".join(missing)))
    return (np.stack([vert["x"], vert["y"], vert["z"]], 1), np.stack([vert["nx"], vert["ny"], vert["nz"]], 1))


def _sample(dev, rel, diam, cap, points=None, normals=None, depth=None, mask=None, cam_K=None):
    """ossid_ppf_sample -> dict of device tensors idx [cap], pts [cap,3], nrm [cap,3] (model), count [1], stats [8]."""
    if points is not None:
        n_in = int(points.shape[0])
        H = W = 0
    else:
        H, W = int(depth.shape[0]), int(depth.shape[1])
        n_in = H * W
    ws_bytes = int(_lib.fn("ossid_ppf_sample_workspace_bytes")(n_in))
    if ws_bytes == 0:
        raise ValueError("PPF sampling: bad input size %d" % n_in)
    out = {"ws": torch.empty(ws_bytes, dtype=torch.uint8, device=dev),
           "idx": torch.empty(cap, dtype=torch.int32, device=dev), "pts": torch.empty(cap, 3, dtype=torch.float32, device=dev),
           "nrm": torch.empty(cap, 3, dtype=torch.float32, device=dev) if normals is not None else None,
           "count": torch.empty(1, dtype=torch.int32, device=dev), "stats": torch.empty(8, dtype=torch.float32, device=dev)}
    K = np.asarray(cam_K if cam_K is not None else np.eye(3), dtype=np.float64)
    _call("ossid_ppf_sample", points.data_ptr() if points is not None else None,
          normals.data_ptr() if normals is not None else None, n_in,
          depth.data_ptr() if depth is not None else None, mask.data_ptr() if mask is not None else None, H, W,
          float(np.float32(K[0, 0])), float(np.float32(K[1, 1])), float(np.float32(K[0, 2])), float(np.float32(K[1, 2])),
          float(np.float32(rel)), float(diam), cap, out["ws"].data_ptr(), ws_bytes, out["idx"].data_ptr(),
          out["pts"].data_ptr(), out["nrm"].data_ptr() if out["nrm"] is not None else None, out["count"].data_ptr(),
          out["stats"].data_ptr(), _lib.stream())
    return out


class PPFModel:
    """A surface model for point-pair-feature matching (SPEC 6), built once on the device. `model` is a .ply path (BOP
    models: x y z nx ny nz on the vertex element) or an array [V,3], which then needs `normals` [V,3]. All lengths are in
    the model's units; scenes must come in the same units (the drop-in: mm; OnlineStream: m)."""

    def __init__(self, model, ModelSamplingDist=0.03, normals=None):
        if isinstance(model, (str, bytes, os.PathLike)):
            points, normals = read_ply(model)
        else:
            points = np.asarray(model, dtype=np.float64)
            if normals is None:
                raise ValueError("PPFModel: an array model needs normals [V,3] (or pass a .ply path with nx ny nz)")
        points, normals = np.asarray(points, dtype=np.float64), np.asarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape or len(points) == 0:
            raise ValueError("PPFModel: points and normals must both be [V,3] with V > 0")
        if not float(ModelSamplingDist) > 0.0:
            raise ValueError("PPFModel: ModelSamplingDist must be > 0")
        dev = _lib._dev()
        self.device = dev
        self.sampling_dist = float(ModelSamplingDist)
        cap = _lib.PPF_MAX_MODEL_POINTS
        Pd, Nd = _f32(points, dev), _f32(normals, dev)
        s = _sample(dev, ModelSamplingDist, 0.0, cap, points=Pd, normals=Nd)
        Ms = int(s["count"].item())
        if Ms > cap:
            raise ValueError("PPFModel: ModelSamplingDist=%g keeps %d model points, more than the %d this build takes; "
                             "raise ModelSamplingDist" % (ModelSamplingDist, Ms, cap))
        if Ms < 2:
            raise ValueError("PPFModel: ModelSamplingDist=%g keeps %d model point(s)" % (ModelSamplingDist, Ms))
        stats = s["stats"].cpu().numpy()
        self.Ms, self.D, self.h = Ms, np.float32(stats[6]), np.float32(stats[7])
        self.idx = s["idx"][:Ms]
        self.points, self.normals = s["pts"][:Ms].contiguous(), s["nrm"][:Ms].contiguous()
        words = int(_lib.fn("ossid_ppf_model_table_words")(Ms, float(self.h), float(self.D)))
        if words == 0:
            raise ValueError("PPFModel: ModelSamplingDist=%g gives more than 128 distance bins" % ModelSamplingDist)
        self.offsets = torch.empty(words, dtype=torch.int32, device=dev)
        self.entries = torch.empty(max(1, Ms * (Ms - 1)), dtype=torch.int32, device=dev)
        ws = torch.empty(words, dtype=torch.int32, device=dev)
        _call("ossid_ppf_model_table", self.points.data_ptr(), self.normals.data_ptr(), Ms, float(self.h), float(self.D),
              self.offsets.data_ptr(), self.entries.data_ptr(), int(self.entries.numel()), ws.data_ptr(), 4 * words,
              _lib.stream())
        self.chunks = (Ms + 1023) // 1024
        self.refine, self.refine_reason = self._refine_surface(Pd, Nd)

    DENSE_DEFAULT = "false"              # find_surface_model's DensePoseRefinement default (PPFModelDense: 'true')

    def _refine_surface(self, Pd, Nd):
        """SPEC 6.9's refinement surface and its grid -> (dict, None), or (None, reason) when it cannot be built."""
        cap = _lib.PPF_MAX_REFINE_MODEL_POINTS
        s = _sample(self.device, REFINE_SAMPLING_REL, float(self.D), cap, points=Pd, normals=Nd)
        Mr = int(s["count"].item())
        if Mr > cap:
            return None, ("the refinement sampling (%g D) keeps %d model points, more than the %d this build takes"
                          % (REFINE_SAMPLING_REL, Mr, cap))
        if Mr < 6:
            return None, "the refinement sampling keeps %d model point(s)" % Mr
        h = np.float32(s["stats"][7].item())
        gb = int(_lib.fn("ossid_ppf_refine_grid_bytes")(Mr, REFINE_STEPS, float(self.D), float(h)))
        if gb == 0:
            return None, "no refinement grid for D=%g, h=%g" % (self.D, h)
        grid = torch.empty(gb, dtype=torch.uint8, device=self.device)
        pts, nrm = s["pts"][:Mr].contiguous(), s["nrm"][:Mr].contiguous()
        _call("ossid_ppf_refine_model_grid", pts.data_ptr(), nrm.data_ptr(), Mr, REFINE_STEPS, float(self.D), float(h),
              grid.data_ptr(), gb, _lib.stream())
        return {"Mr": Mr, "h": h, "idx": s["idx"][:Mr], "points": pts, "normals": nrm, "grid": grid,
                "steps": REFINE_STEPS}, None

    def _refine(self, source, r, steps=REFINE_STEPS):
        """SPEC 6.9 on the hypotheses of one _run (device tensors, no host copy) -> dict of device tensors."""
        R, dev = self.refine, self.device
        cap = _lib.PPF_MAX_REFINE_SCENE_POINTS
        s = _sample(dev, REFINE_SAMPLING_REL, float(self.D), cap, **source)
        NR = int(r["poses"].shape[0])
        wsb = int(_lib.fn("ossid_ppf_refine_workspace_bytes")(cap, NR))
        if wsb == 0:
            raise ValueError("find_surface_model: NumResult=%d is more than this build refines" % NR)
        out = {"sample": s, "ws": torch.empty(wsb, dtype=torch.uint8, device=dev),
               "poses": torch.empty(NR, 4, 4, dtype=torch.float64, device=dev),
               "scores": torch.empty(NR, dtype=torch.float64, device=dev),
               "pairs": torch.empty(NR, dtype=torch.int32, device=dev), "steps": torch.empty(NR, dtype=torch.int32, device=dev),
               "status": torch.empty(4, dtype=torch.int32, device=dev)}
        _call("ossid_ppf_refine", s["pts"].data_ptr(), s["count"].data_ptr(), cap, R["grid"].data_ptr(), int(R["grid"].numel()),
              R["Mr"], r["poses"].data_ptr(), r["info"].data_ptr(), NR, int(steps), float(self.D), float(R["h"]),
              out["ws"].data_ptr(), wsb, out["poses"].data_ptr(), out["scores"].data_ptr(), out["pairs"].data_ptr(),
              out["steps"].data_ptr(), out["status"].data_ptr(), _lib.stream())
        return out

    def _need_refine(self):
        if getattr(self, "refine", None) is None:
            raise ValueError("find_surface_model: DensePoseRefinement='true' needs the model's refinement surface, which "
                             "this model does not hold (%s)" % (getattr(self, "refine_reason", None) or "not built"))

    # ---- the device form -----------------------------------------------------------------------------------------------
    def _run(self, source, SceneSamplingDist=0.05, RefPtRate=0.2, NumResult=100, PoseClusterDistRel=0.1,
             NormalRadiusRel=NORMAL_RADIUS_REL, normals=None):
        """The launch chain on one scene source (dict for _sample) -> dict of device tensors of every stage."""
        for nm, v in (("SceneSamplingDist", SceneSamplingDist), ("RefPtRate", RefPtRate),
                      ("PoseClusterDistRel", PoseClusterDistRel), ("NormalRadiusRel", NormalRadiusRel)):
            if not float(v) > 0.0:
                raise ValueError("find_surface_model: %s must be > 0, got %r" % (nm, v))
        if float(RefPtRate) > 1.0:
            raise ValueError("find_surface_model: RefPtRate must be <= 1, got %r" % (RefPtRate,))
        if int(NumResult) <= 0:
            raise ValueError("find_surface_model: NumResult must be >= 1")
        dev, cap = self.device, _lib.PPF_MAX_SCENE_SAMPLES
        step = max(1, int(np.floor(1.0 / float(RefPtRate) + 0.5)))
        s = _sample(dev, SceneSamplingDist, float(self.D), cap, **source)
        h = np.float32(np.float32(SceneSamplingDist) * self.D)
        if normals is None:
            nrm = torch.empty(cap, 3, dtype=torch.float32, device=dev)
            ok = torch.empty(cap, dtype=torch.uint8, device=dev)
            _call("ossid_ppf_scene_normals", s["pts"].data_ptr(), s["count"].data_ptr(), cap,
                  float(np.float32(np.float32(NormalRadiusRel) * h)), nrm.data_ptr(), ok.data_ptr(), _lib.stream())
        else:
            nrm, ok = (_f32(normals[0], dev), torch.as_tensor(np.asarray(normals[1]), dtype=torch.uint8).to(dev))
            nrm = torch.cat([nrm, torch.zeros(cap - nrm.shape[0], 3, device=dev)]).contiguous()
            ok = torch.cat([ok, torch.zeros(cap - ok.shape[0], dtype=torch.uint8, device=dev)]).contiguous()
        max_ref = (cap + step - 1) // step
        vws = int(_lib.fn("ossid_ppf_vote_workspace_bytes")(cap, step, self.Ms))
        vw = torch.empty(vws, dtype=torch.uint8, device=dev)
        peaks = torch.empty(max_ref, 3, dtype=torch.int32, device=dev)
        cand = torch.empty(max_ref, 4, 4, dtype=torch.float64, device=dev)
        _call("ossid_ppf_vote", s["pts"].data_ptr(), nrm.data_ptr(), ok.data_ptr(), s["count"].data_ptr(), cap, step,
              self.points.data_ptr(), self.normals.data_ptr(), self.Ms, float(self.h), float(self.D),
              self.offsets.data_ptr(), self.entries.data_ptr(), vw.data_ptr(), vws, peaks.data_ptr(), cand.data_ptr(),
              _lib.stream())
        poses = torch.empty(int(NumResult), 4, 4, dtype=torch.float64, device=dev)
        scores = torch.empty(int(NumResult), dtype=torch.float64, device=dev)
        info = torch.empty(4, dtype=torch.int32, device=dev)
        _call("ossid_ppf_cluster", peaks.data_ptr(), cand.data_ptr(), s["count"].data_ptr(), cap, step, self.Ms,
              float(self.D), float(np.float32(PoseClusterDistRel)), int(NumResult), poses.data_ptr(), scores.data_ptr(),
              info.data_ptr(), _lib.stream())
        return {"sample": s, "normals": nrm, "normals_ok": ok, "ref_step": step, "peaks": peaks, "cand_poses": cand,
                "poses": poses, "scores": scores, "info": info, "h": h}

    def find_hypotheses(self, depth, mask, cam_K, SceneSamplingDist=0.05, RefPtRate=0.2, NumResult=100,
                        PoseClusterDistRel=0.1, NormalRadiusRel=NORMAL_RADIUS_REL, DensePoseRefinement=False):
        """Device form: depth f32 [H,W] (the model's units, 0 = invalid), mask [H,W] (bool / u8; pixel used iff mask
        && depth > 0), cam_K [3,3] -> device tensors (poses f64 [NumResult,4,4], scores f64 [NumResult], info int32 [4]
        = results, sampled scene points, candidates, clusters). Rows past info[0] are zero. Nothing is copied to the host:
        a scene over the sample cap shows as info[1] > PPF_MAX_SCENE_SAMPLES (check_info raises on it).
        DensePoseRefinement=True refines the hypotheses against the same pixels (SPEC 6.9): poses and scores are then the
        refined ones, sorted by refined score, and a fourth tensor, the refinement status int32 [4], follows
        (check_refine raises when the refinement scene was over its cap)."""
        dense = dense_flag(DensePoseRefinement)
        if dense:
            self._need_refine()
        dev = self.device
        D = _f32(depth, dev)
        M = (mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask)))
        if D.dim() != 2 or tuple(M.shape) != tuple(D.shape):
            raise ValueError("find_hypotheses: depth and mask must both be [H,W]")
        M = M.to(dev).to(torch.uint8).contiguous()
        source = {"depth": D, "mask": M, "cam_K": cam_K}
        r = self._run(source, SceneSamplingDist, RefPtRate, NumResult, PoseClusterDistRel, NormalRadiusRel)
        if not dense:
            return r["poses"], r["scores"], r["info"]
        f = self._refine(source, r)
        return f["poses"], f["scores"], r["info"], f["status"]

    # ---- the drop-in ---------------------------------------------------------------------------------------------------
    def find_surface_model(self, scene_pc, **kwargs):
        """Halcon's find_surface_model as online_learning.py:418 / :446 call it: scene_pc [N,3] in the model's units ->
        (poses np.float64 [n,4,4] in those units, scores np.float64 [n], seconds), n <= NumResult, best first.
        Keywords: SceneSamplingDist (0.05), RefPtRate (0.2), NumResult (100), DensePoseRefinement ('false'; 'true' /
        'false' in any case or a bool; 'true' refines every hypothesis, SPEC 6.9, and `seconds` includes it),
        PoseClusterDistRel (0.1), NormalRadiusRel (2.0); anything else raises."""
        unknown = sorted(set(kwargs) - set(ACCEPTED))
        if unknown:
            raise ValueError("find_surface_model: unknown keyword(s) %s; accepted: %s" % (", ".join(unknown), ", ".join(ACCEPTED)))
        dense = dense_flag(kwargs.pop("DensePoseRefinement", self.DENSE_DEFAULT))
        if dense:
            self._need_refine()
        P = np.asarray(scene_pc, dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != 3 or len(P) == 0:
            raise ValueError("find_surface_model: scene_pc must be [N,3] with N > 0")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        source = {"points": _f32(P, self.device)}
        r = self._run(source, **kwargs)
        f = self._refine(source, r) if dense else r
        info = check_info(r["info"], kwargs.get("SceneSamplingDist", 0.05))
        if dense:
            check_refine(f["status"])
        n = info[0]
        poses, scores = f["poses"][:n].cpu().numpy(), f["scores"][:n].cpu().numpy()
        return poses, scores, time.perf_counter() - t0


class PPFModelDense(PPFModel):
    """PPFModel whose find_surface_model defaults to Halcon's DensePoseRefinement='true' (compat.install(ppf=True,
    ppf_dense_refinement=True)): the LM-O call :446, which passes no keyword, gets refined hypotheses."""
    DENSE_DEFAULT = "true"


def check_info(info, scene_sampling_dist):
    """info of a find (device int32 [4]) -> host list; raises when the scene had more sampled points than the cap."""
    v = [int(x) for x in info.cpu().numpy()]
    if v[1] > _lib.PPF_MAX_SCENE_SAMPLES:
        raise ValueError("find_surface_model: SceneSamplingDist=%g keeps %d scene points, more than the %d this build "
                         "takes; raise SceneSamplingDist or shrink the mask" % (scene_sampling_dist, v[1],
                                                                                 _lib.PPF_MAX_SCENE_SAMPLES))
    return v


def check_refine(status):
    """status of a refinement (device int32 [4]) -> host list; raises when the refinement scene was over its cap."""
    v = [int(x) for x in status.cpu().numpy()]
    if v[0] != 0:
        raise ValueError("find_surface_model: DensePoseRefinement: the refinement sampling (%g D) keeps %d scene points, "
                         "more than the %d this build takes; shrink the mask or pass DensePoseRefinement='false'"
                         % (REFINE_SAMPLING_REL, v[1], _lib.PPF_MAX_REFINE_SCENE_POINTS))
    return v
