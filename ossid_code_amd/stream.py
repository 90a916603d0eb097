"""The per-frame online loop of OSSID, hot-path steps only, kept on the device end to end -- the synthetic counterpart of
scripts/online_learning.py:314-591 (SURVEY.md 8d cfg-5, 8e "full online stream"):

    detect (DtoidNet.forwardTestTime)                       :346
    -> pose hypotheses (GIVEN per frame, or device PPF with OnlineStream(ppf_models=...), :384-418 / :441-447, and
       the keypoint-feature hypotheses of --use_sift_hypos with OnlineStream(feature_models=...), :427-437, put in
       front of the PPF ones as :437 does)
    -> per-hypothesis ADD/ADI (:452) -> Zephyr score (networkInference, :464) -> argmax (:466-469)
       (with OnlineStream(max_instances=K > 1): the best K distinct poses instead, SPEC.md section 16 -- this build's own
       step, the reference keeps one pose per frame -- and every step below once per pick)
    -> optional ICP refinement of the chosen pose (icpRefinement, :471-480; OnlineStream(icp_max_dist=...))
    -> predicted depth (:485-493: the mesh rasteriser of SPEC.md section 7 with OnlineStream(meshes=...), otherwise
       the point-splat stand-in) -> visibility mask (:500)
    -> if score > threshold: pseudo-label joins the finetune set (:506-516)
    -> when the set reaches the next multiple of finetune_interval: finetune DTOID (:517-533)

Multi-GPU (one process per GPU): the loop is sequential by construction -- the finetune trigger depends on the running count
of confident frames and later frames must see the updated detector -- so frames are dispatched in SPECULATIVE WINDOWS of one
frame per rank with frozen weights, results are committed in frame order, and when the trigger falls inside a window the
frames behind it are discarded, all ranks run the data-parallel finetune (gradient mean over RCCL), and the next window
starts right after the trigger frame. With deterministic per-frame work this reproduces the single-process result.
"""
import time

import numpy as np
import torch

from . import bop_eval, features, model_cloud, pipeline, ppf, render, symmetry
from .hostutil import K2meta
from .scoring import networkInference, pose_errors, select_instances


class SpeculativeWindow:
    """In-order commit logic of the speculative multi-GPU stream, free of any device work (unit-testable):

        w = SpeculativeWindow(n_frames, world, finetune_interval)
        while not w.done:
            frames = w.window()                  # <= world frame ids, one per rank, all scored with the current weights
            trigger = w.commit(confident_flags)  # flags of those frames, in order; returns the training-set size if a
                                                 # finetune fires now (the frames behind the trigger frame are re-issued)
    """

    def __init__(self, n_frames, world, finetune_interval, cumulative=True):
        self.n_frames, self.world, self.interval, self.cumulative = n_frames, world, finetune_interval, cumulative
        self.next_frame = 0
        self.train_set = []
        self.next_finetune = finetune_interval
        self.committed = []           # (frame, confident) in commit order
        self.discarded = 0

    @property
    def done(self):
        return self.next_frame >= self.n_frames

    def window(self):
        return list(range(self.next_frame, min(self.next_frame + self.world, self.n_frames)))

    def commit(self, flags):
        frames = self.window()
        assert len(flags) == len(frames)
        for i, (f, c) in enumerate(zip(frames, flags)):
            self.committed.append((f, bool(c)))
            self.next_frame = f + 1
            if c:
                self.train_set.append(f)
                if len(self.train_set) == self.next_finetune:
                    self.discarded += len(frames) - i - 1      # scored with weights that are about to change
                    size = len(self.train_set)
                    if self.cumulative:
                        self.next_finetune += self.interval
                    else:
                        self.train_set = []
                    return size
        return None


class OnlineStream:
    """One GPU's worth of the loop. `detector` is a dtoid.DtoidNet (eval), `scorer` a zephyr.PointNet2SSG (eval),
    `score_dataset` a zephyr.ScoreDataset; `finetune_fn(samples)` is called with the accumulated pseudo-labelled samples.
    icp_max_dist (None = off): refine the argmax pose by point-to-point ICP (pipeline.icp_refine) against the device row
    uv_original[best] before rendering, timed under times["icp"]; "pred_pose" is then the refined pose and "pred_err" its
    ADD / ADI, recomputed as online_learning.py:482 does after ICP, and the result carries "icp" (fitness, inlier_rmse,
    iterations, the unrefined pose and its error).
    ppf_models (None = off): dict obj_id -> ppf.PPFModel built in metres; hypotheses then come from the frame's depth
    inside the DTOID boxes (ppf.PPFModel.find_hypotheses, mask as online_learning.py:384-405 builds it), timed under
    times["ppf"], `frame["pose_hypos"]` is not read, and the result carries "n_hypos" and the hypotheses ("ppf_hypos"). ppf_kwargs go to find_hypotheses
    ({"DensePoseRefinement": True} refines the hypotheses, SPEC.md 6.9).
    feature_models (None = off): dict obj_id -> features.FeatureModel built in metres; its hypotheses (SPEC.md section 11,
    from the frame's image and depth inside the same mask) are put in front of the PPF ones, timed under times["sift"],
    and the result carries "n_feature_hypos"; with feature models only, `frame["pose_hypos"]` is not read either and a
    frame without any hypothesis gets one identity pose.
    meshes (None = off): dict obj_id -> render.Mesh in metres; the pseudo-label step then renders the mesh of
    frame["obj_id"] at the chosen pose (render.render_depth, pixel_offset = mesh_pixel_offset: 0 is this package's pixel
    convention, under which the render lines up with the observed depth) instead of splatting the model points. A frame
    WITHOUT "model_points" whose object's mesh has vertex colours or a texture is scored with the mesh's own cloud
    (model_cloud.sample_model_cloud(mesh), SPEC.md section 9), built at the object's first frame and kept;
    a frame that carries its cloud is processed exactly as without meshes.
    max_instances (1 = off: no launch, number or result key changes): a frame may show several instances of its object.
    Per frame K = min(max_instances, frame.get("inst_count", max_instances)); with K > 1 the scored hypotheses go through
    scoring.select_instances (SPEC.md section 16: the best K that are different objects in space, timed under
    times["select"]), the picks are refined by one icp_refine call, rendered by one render_depth call (meshes) or splat one
    by one, and each gets its visibility mask against the observed depth -- an instance in front of another makes the
    observed depth nearer, so the hidden part is not visible -- and, if confident, its pseudo-label. The existing result
    keys then describe pick 0 (the argmax: bit for bit what max_instances=1 returns) and the result also carries
    "selected" and "owner" (host int32 arrays over the scored hypotheses, as select_instances returns them) and
    "instances", one dict per pick with pred_pose, pred_score, pred_err, confident, pred_mask_visib, sample and, with ICP,
    icp. A frame whose K is 1 is processed as without max_instances and carries none of the three.
    instance_sep_rel: two poses nearer than instance_sep_rel x the object's diameter (max over model points, min over
    symmetries) are one instance. The default 0.2 is the extent of one PPF pose cluster (SPEC.md 6.6: 0.1 of the diameter
    in translation plus 12 degrees, which move a point at radius D/2 by 0.105 D); nobody has tuned it. Thin objects that
    stack (plates, lids: neighbours a fraction of the diameter apart) need a smaller value.
    symmetries: dict obj_id -> f64 [S,4,4] (bop_eval.symmetry_transformations) in the unit of model_points -- BOP's
    models_info is in millimetres, the caller converts; an object without an entry has none. "auto" (needs meshes=...):
    each object's symmetries are found from its mesh at its first frame (symmetry.find_symmetries, SPEC.md section 17, in
    the mesh's unit; an object without a mesh has none) and kept, passed where a dict's entry is passed, and an object
    found to have any symmetry is scored with ADI as under symmetric=True.
    diameters: dict obj_id -> length in that unit; otherwise frame["diameter"], otherwise
    model_cloud.mesh_diameter(model_points) at the object's first frame, kept.
    frame["pose_gt"] may be [G,4,4]: pp_err and every pred_err are then the minimum over the G instances."""

    def __init__(self, detector, scorer, score_dataset, confident_threshold=20.0, symmetric=False, finetune_fn=None,
                 icp_max_dist=None, ppf_models=None, ppf_kwargs=None, meshes=None, mesh_pixel_offset=0.0,
                 feature_models=None, feature_kwargs=None, max_instances=1, instance_sep_rel=0.2, symmetries=None,
                 diameters=None):
        self.detector, self.scorer, self.dataset = detector, scorer, score_dataset
        self.threshold, self.symmetric, self.finetune_fn = confident_threshold, symmetric, finetune_fn
        self.icp_max_dist = icp_max_dist
        self.ppf_models, self.ppf_kwargs = ppf_models, dict(ppf_kwargs or {})
        self.meshes, self.mesh_pixel_offset = meshes, float(mesh_pixel_offset)
        self.feature_models, self.feature_kwargs = feature_models, dict(feature_kwargs or {})
        self._clouds = {}
        self.max_instances, self.instance_sep_rel = int(max_instances), float(instance_sep_rel)
        if self.max_instances != max_instances or self.max_instances < 1:
            raise ValueError("max_instances must be an integer >= 1, got %r" % (max_instances,))
        if not (np.isfinite(self.instance_sep_rel) and self.instance_sep_rel >= 0.0):
            raise ValueError("instance_sep_rel must be finite and >= 0, got %r" % (instance_sep_rel,))
        self.symmetries, self.diameters, self._diameters = symmetries, diameters, {}
        if isinstance(symmetries, str):
            if symmetries != "auto" or meshes is None:
                raise ValueError('symmetries must be a dict, None or "auto" with meshes=..., got %r' % (symmetries,))
            self._found = {}
        keys = ("detect", "pose_err", "score", "pseudo_label") + (("icp",) if icp_max_dist is not None else ()) + \
            (("ppf",) if ppf_models is not None else ()) + (("sift",) if feature_models is not None else ()) + \
            (("select",) if self.max_instances > 1 else ())
        self.times = {k: 0.0 for k in keys}
        self.n_processed = 0

    def _timed(self, key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.times[key] += time.perf_counter() - t0
        return out

    def _with_cloud(self, frame):
        """The frame itself if it carries model_points; otherwise a copy with the cloud of its object's mesh."""
        if "model_points" in frame:
            return frame
        obj = int(frame["obj_id"])
        mesh = None if self.meshes is None else self.meshes.get(obj)
        if mesh is None or (getattr(mesh, "colors", None) is None and getattr(mesh, "mips", None) is None):
            raise KeyError("frame of object %d has no model_points, and OnlineStream(meshes=...) holds no vertex-coloured "
                           "or textured mesh of it to sample them from" % obj)
        if obj not in self._clouds:
            cloud = model_cloud.sample_model_cloud(mesh)
            # host arrays, as the frames of a stream carry them (pose_errors and the ICP take numpy)
            self._clouds[obj] = {k: v.cpu().numpy() for k, v in cloud.as_dict().items()}
        return {**frame, **self._clouds[obj]}

    def process(self, frame):
        """frame: dict with img uint8 [H,W,3], depth [H,W], cam_K, limg [n_t,3,124,124], lmask [n_t,1,124,124], obj_id,
        pose_hypos [N,4,4], pose_gt [4,4] or [G,4,4], model_points/normals/colors [M,3]; optional inst_count, diameter.
        Returns the per-frame result dict."""
        dev = next(self.detector.parameters()).device
        frame = self._with_cloud(frame)
        self.n_processed += 1
        img_t = torch.from_numpy(np.ascontiguousarray(frame["img"])).to(dev).permute(2, 0, 1).float().div_(255.0)[None]
        batch = {"img": img_t, "obj_id": torch.tensor([int(frame["obj_id"])]), "limg": frame["limg"][None].to(dev),
                 "lmask": frame["lmask"][None].to(dev)}
        det = self._timed("detect", lambda: self.detector.forwardTestTime(batch))
        n_feat = None
        if self.ppf_models is None and self.feature_models is None:
            hypos = frame["pose_hypos"]
        else:
            hypos = None if self.ppf_models is None else self._timed("ppf", lambda: self._ppf_hypotheses(frame, det))
            if self.feature_models is not None:
                feat = self._timed("sift", lambda: self._feature_hypotheses(frame, det))
                n_feat = len(feat)
                hypos = feat if hypos is None else np.concatenate([feat, hypos], axis=0)       # :437
                if len(hypos) == 0:
                    hypos = np.eye(4)[None]
        pp_err = self._timed("pose_err", lambda: self._pose_errors(hypos, frame))
        data = {k: frame[k] for k in ("img", "depth", "cam_K", "model_points", "model_normals", "model_colors")}
        data["pose_hypos"], data["pp_err"] = hypos, pp_err
        poses, scores, errs, uv = self._timed("score", lambda: networkInference(self.scorer, self.dataset, data))
        K = min(self.max_instances, max(1, int(frame.get("inst_count", self.max_instances))))
        if K > 1:
            return self._finish_instances(frame, det, hypos, n_feat, poses, scores, errs, uv, K)
        best = int(scores.argmax())
        pred_pose, pred_score = poses[best], float(scores.max())
        H, W = frame["depth"].shape
        pred_err = float(np.asarray(errs)[best])
        icp = None
        if self.icp_max_dist is not None:
            def refine():
                out, fit, rmse, its = pipeline.icp_refine(frame["depth"], uv[best], pred_pose, frame["cam_K"],
                                                          frame["model_points"], max_dist=self.icp_max_dist)
                T = out[0].cpu().numpy()
                err = self._pose_errors(T[None], frame)                                               # :482
                return T, float(err[0]), float(fit[0]), float(rmse[0]), int(its[0])
            refined, refined_err, fit, rmse, its = self._timed("icp", refine)
            icp = {"fitness": fit, "inlier_rmse": rmse, "iterations": its, "pose_unrefined": pred_pose,
                   "err_unrefined": pred_err}
            pred_pose, pred_err = refined, refined_err

        def pseudo():
            if self.meshes is not None:
                pred_depth = render.render_depth(self.meshes[int(frame["obj_id"])], pred_pose, frame["cam_K"], (H, W),
                                                 pixel_offset=self.mesh_pixel_offset)
                return pipeline.visibility_and_iou(frame["depth"], pred_depth)[:2]
            pred_depth = pipeline.render_depth_points(pred_pose, frame["model_points"], frame["cam_K"], (H, W), radius=1)
            return pipeline.visibility_and_iou(frame["depth"], pred_depth)[:2]
        _pred_mask, pred_mask_visib = self._timed("pseudo_label", pseudo)
        confident = pred_score > self.threshold
        sample = None
        if confident:
            sample = pipeline.make_dtoid_sample(frame["img"], frame["depth"], pred_mask_visib.float(), frame["cam_K"])
        return {"pred_pose": pred_pose, "pred_score": pred_score, "pred_err": pred_err,
                "confident": confident, "dtoid_score": det["pred_scores"][:1], "dtoid_bbox": det["pred_bbox"][:1],
                "pred_mask_visib": pred_mask_visib, "sample": sample, **({"icp": icp} if icp is not None else {}),
                **({"n_hypos": len(hypos), "ppf_hypos": hypos} if self.ppf_models is not None else {}),
                **({"n_hypos": len(hypos), "n_feature_hypos": n_feat} if n_feat is not None else {})}

    def _symmetries(self, obj):
        """The object's symmetry transformations f64 [S,4,4], or None: the caller's dict, or with "auto" what
        symmetry.find_symmetries makes of its mesh, found once."""
        if self.symmetries is None:
            return None
        if not isinstance(self.symmetries, str):
            return self.symmetries.get(obj)
        if obj not in self._found:
            mesh = self.meshes.get(obj)
            found = None if mesh is None else symmetry.find_symmetries(mesh)
            self._found[obj] = bop_eval.symmetry_transformations(found) if found and symmetry.has_symmetry(found) else None
        return self._found[obj]

    def _symmetric(self, frame):
        if isinstance(self.symmetries, str) and self._symmetries(int(frame["obj_id"])) is not None:
            return True
        return self.symmetric

    def _pose_errors(self, hypos, frame):
        """ADD / ADI of the hypotheses against frame["pose_gt"]; against [G,4,4] the minimum over the G instances."""
        gt, symmetric = frame["pose_gt"], self._symmetric(frame)
        if len(np.shape(gt)) != 3:
            return pose_errors(hypos, gt, frame["model_points"], symmetric)
        if np.shape(gt)[0] < 1:
            raise ValueError("pose_gt must hold at least one pose, got %s" % (np.shape(gt),))
        return np.minimum.reduce([pose_errors(hypos, g, frame["model_points"], symmetric) for g in gt])

    def _diameter(self, frame):
        obj = int(frame["obj_id"])
        if self.diameters is not None and obj in self.diameters:
            return float(self.diameters[obj])
        if "diameter" in frame:
            return float(frame["diameter"])
        if obj not in self._diameters:
            self._diameters[obj] = model_cloud.mesh_diameter(frame["model_points"])
        return self._diameters[obj]

    def _finish_instances(self, frame, det, hypos, n_feat, poses, scores, errs, uv, K):
        """process() from the scores on for a frame with K > 1: the K best distinct poses, each refined, rendered, masked
        and pseudo-labelled; pick 0 is the argmax and fills the single-instance keys."""
        obj = int(frame["obj_id"])
        syms = self._symmetries(obj)
        sep = self.instance_sep_rel * self._diameter(frame)
        sel, _count, own = self._timed("select", lambda: select_instances(poses, scores, frame["model_points"], K, sep,
                                                                          symmetries=syms))
        selected, owner = sel.cpu().numpy(), own.cpu().numpy()
        picks = [int(p) for p in selected if p >= 0]
        if not picks or picks[0] != int(scores.argmax()):
            raise ValueError("OnlineStream: the frame's scores hold a NaN; the instances cannot be ranked")
        H, W = frame["depth"].shape
        flat, errs = np.asarray(scores).reshape(-1), np.asarray(errs)
        pred_poses = [poses[p] for p in picks]
        pred_scores = [float(flat[p]) for p in picks]
        pred_errs = [float(errs[p]) for p in picks]
        icps = [None] * len(picks)
        if self.icp_max_dist is not None:
            def refine():
                out, fit, rmse, its = pipeline.icp_refine(frame["depth"], uv[picks], np.stack(pred_poses), frame["cam_K"],
                                                          frame["model_points"], max_dist=self.icp_max_dist)
                T = out.cpu().numpy()
                return T, self._pose_errors(T, frame), fit.cpu().numpy(), rmse.cpu().numpy(), its.cpu().numpy()   # :482
            refined, refined_err, fit, rmse, its = self._timed("icp", refine)
            for i in range(len(picks)):
                icps[i] = {"fitness": float(fit[i]), "inlier_rmse": float(rmse[i]), "iterations": int(its[i]),
                           "pose_unrefined": pred_poses[i], "err_unrefined": pred_errs[i]}
                pred_poses[i], pred_errs[i] = refined[i], float(refined_err[i])

        def pseudo():
            if self.meshes is not None:
                depths = render.render_depth(self.meshes[obj], np.stack(pred_poses), frame["cam_K"], (H, W),
                                             pixel_offset=self.mesh_pixel_offset)
            else:
                depths = [pipeline.render_depth_points(T, frame["model_points"], frame["cam_K"], (H, W), radius=1)
                          for T in pred_poses]
            return [pipeline.visibility_and_iou(frame["depth"], d)[1] for d in depths]
        masks = self._timed("pseudo_label", pseudo)
        instances = []
        for i in range(len(picks)):
            confident = pred_scores[i] > self.threshold
            sample = None
            if confident:
                sample = pipeline.make_dtoid_sample(frame["img"], frame["depth"], masks[i].float(), frame["cam_K"])
            instances.append({"pred_pose": pred_poses[i], "pred_score": pred_scores[i], "pred_err": pred_errs[i],
                              "confident": confident, "pred_mask_visib": masks[i], "sample": sample,
                              **({"icp": icps[i]} if icps[i] is not None else {})})
        first = instances[0]
        return {"pred_pose": first["pred_pose"], "pred_score": first["pred_score"], "pred_err": first["pred_err"],
                "confident": first["confident"], "dtoid_score": det["pred_scores"][:1], "dtoid_bbox": det["pred_bbox"][:1],
                "pred_mask_visib": first["pred_mask_visib"], "sample": first["sample"],
                **({"icp": first["icp"]} if "icp" in first else {}),
                **({"n_hypos": len(hypos), "ppf_hypos": hypos} if self.ppf_models is not None else {}),
                **({"n_hypos": len(hypos), "n_feature_hypos": n_feat} if n_feat is not None else {}),
                "selected": selected, "owner": owner, "instances": instances}

    def _detection_mask(self, frame, det):
        """online_learning.py:384-405: the mask from the expanded DTOID boxes -> (depth f32 [H,W], mask u8 [H,W])."""
        depth = np.asarray(frame["depth"], dtype=np.float32)
        H, W = depth.shape
        mask = np.zeros((H, W), dtype=np.uint8)
        boxes = det["final_bbox"][0].detach().cpu().numpy().reshape(-1, 4)
        scores = det["final_score"][0].detach().cpu().numpy().reshape(-1)
        for (x1, y1, x2, y2), sc in zip(boxes, scores):
            if sc < 0.5 and (mask.astype(bool) & (depth > 0)).any():
                continue
            x1, y1, x2, y2 = pipeline.expand_box(x1, y1, x2, y2, H, W, 1.2)
            mask[int(y1):int(y2), int(x1):int(x2)] = 1
        return depth, mask

    def _feature_hypotheses(self, frame, det):
        """online_learning.py:427-435 on the device -> poses f64 [n,4,4], n >= 0."""
        depth, mask = self._detection_mask(frame, det)
        model = self.feature_models[int(frame["obj_id"])]
        poses, _scores, info = model.find_hypotheses(depth, frame["img"], mask, frame["cam_K"], **self.feature_kwargs)
        n, found = (int(v) for v in info[:2].cpu().numpy())
        if found > features.MAX_KEYPOINTS:
            raise ValueError("OnlineStream: the frame has %d keypoints, more than the %d the feature stage takes; raise "
                             "feature_kwargs['contrast']" % (found, features.MAX_KEYPOINTS))
        return poses[:n].cpu().numpy()

    def _ppf_hypotheses(self, frame, det):
        """The mask of :384-405 and :441-447 (PPF on the masked depth)."""
        depth, mask = self._detection_mask(frame, det)
        model = self.ppf_models[int(frame["obj_id"])]
        out = model.find_hypotheses(depth, mask, frame["cam_K"], **self.ppf_kwargs)
        poses, info = out[0], out[2]
        n = ppf.check_info(info, self.ppf_kwargs.get("SceneSamplingDist", 0.05))[0]
        if len(out) > 3:     # DensePoseRefinement: the refined hypotheses, best refined score first
            ppf.check_refine(out[3])
        if n == 0:           # nothing found: one identity hypothesis, as online_learning.py:429-430 does for SIFT
            return np.eye(4)[None]
        return poses[:n].cpu().numpy()

    def run(self, frames, finetune_interval=8):
        """Sequential loop on this GPU (world 1); returns (results, window bookkeeping)."""
        win = SpeculativeWindow(len(frames), 1, finetune_interval)
        results, samples = [], []
        while not win.done:
            f = win.window()[0]
            r = self.process(frames[f])
            results.append(r)
            for inst in r.get("instances", (r,)):              # every confident instance's pseudo-label
                if inst["sample"] is not None:
                    samples.append((frames[f], inst["sample"]))
            fired = win.commit([r["confident"]])
            if fired is not None and self.finetune_fn is not None:
                self.finetune_fn(samples)
        return results, win


def run_speculative(frames, process_fn, finetune_fn, finetune_interval, dist=None, group=None):
    """The multi-GPU stream, SPMD: every rank calls this with the same `frames`. process_fn(frame) -> (confident, sample)
    scores one frame with this rank's (replicated) weights; finetune_fn(train_set) is entered by ALL ranks together with the
    identical, frame-ordered list of (frame_id, sample) and is expected to run the data-parallel finetune (GradSync).
    Per window: one frame per rank, an all_gather of the confident flags, in-order commit, an all_gather_object-free
    sample exchange (each confident sample is broadcast from the rank that produced it: a 480x640 sample is ~5 MB, one
    xGMI hop). Returns the committed [(frame_id, confident)] and the SpeculativeWindow (for .discarded)."""
    world = dist.get_world_size(group) if dist is not None and dist.is_initialized() else 1
    rank = dist.get_rank(group) if world > 1 else 0
    win = SpeculativeWindow(len(frames), world, finetune_interval)
    train = []
    while not win.done:
        ids = win.window()
        mine = ids[rank] if rank < len(ids) else None
        confident, sample = process_fn(frames[mine]) if mine is not None else (False, None)
        if world > 1:
            flag = torch.tensor([1 if confident else 0], dtype=torch.int32)
            if dist.get_backend(group) == "nccl":
                flag = flag.cuda()
            flags = [torch.zeros_like(flag) for _ in range(world)]
            dist.all_gather(flags, flag, group=group)
            flags = [bool(int(f)) for f in flags][: len(ids)]
        else:
            flags = [bool(confident)]
        n_before = len(win.committed)
        fired = win.commit(flags)
        for f, c in win.committed[n_before:]:
            if not c:
                continue
            src = f - ids[0]
            if world > 1:
                sample_f = _broadcast_sample(sample if src == rank else None, src, dist, group)
            else:
                sample_f = sample
            train.append((f, sample_f))
        if fired is not None:
            finetune_fn(train)
    return win.committed, win


def _broadcast_sample(sample, src, dist, group):
    """Sends a dict of tensors from rank `src` to everyone: the (small) key/shape/dtype header as an object, the payload as
    tensor broadcasts on the group's device."""
    header = [None]
    if sample is not None:
        header = [[(k, tuple(v.shape), v.dtype, v.is_cuda) for k, v in sample.items() if torch.is_tensor(v)]]
    dist.broadcast_object_list(header, src=src, group=group)
    out = {}
    for k, shape, dtype, on_gpu in header[0]:
        if sample is not None:
            t = sample[k].contiguous()
        else:           # same device kind as the sender's tensor (device tensors stay on the device: RCCL, or gloo's CUDA path)
            t = torch.empty(shape, dtype=dtype, device="cuda" if on_gpu else "cpu")
        dist.broadcast(t, src=src, group=group)
        out[k] = t
    return out
