"""Pre-training of the DTOID detector on rendered scenes (SPEC.md section 15): the counterpart of the reference's
python/ossid/train.py over datasets/dtoid_dataset.py:97-236, whose BlenderProc HDF5 renders are in neither tree. The
scenes are scenes.render_scenes's (SPEC 13), the batches are made on the device by one launch of csrc/pretrain.hip
(ossid_scene_dtoid_batch) and the step is finetune.finetune_step, so a folder of BOP models is enough to produce the
checkpoint scripts/online_learning.py:153-167 starts from (--dtoid_weights_path; :161-162 loads ckpt['state_dict']).

    scene_batch        T (scene, instance) targets of a SceneBatch -> img / mask / bbox_gt / heatmap, no read-back
    select_targets     the targets worth training on, from one read-back of gt_info
    sample_jitter      photometric jitter rows (host; build-defined)
    ScenePretrainSet   iterator of D14 batches: layouts, sensor, render, selection, templates
    split_objects      the reference's train / validation split by object id (dtoid_dataset.py:38-39)
    DtoidPretrainer    step / validate / save / load

All paths cite /root/reference/python/ossid.
"""
import numpy as np
import torch

from .. import _lib, scenes, synth
from ..pipeline import HEATMAP_SIGMA
from . import finetune

MIN_VISIB, MIN_PX = 0.25, 400        # select_targets' defaults (build-defined, SPEC 15.4)
MAX_REDRAWS = 8                      # refreshes in a row without a batch before ScenePretrainSet gives up


def _need(ok, what):
    if not ok:
        raise ValueError(what)


def _shape(x):
    return tuple(int(v) for v in (x.shape if hasattr(x, "shape") else np.shape(x)))


def scene_batch(scene_batch, targets, heatmap_hw=(29, 39), jitter=None):
    """SPEC 15.1-15.3. scene_batch: what scenes.render_scenes returned (device tensors); targets int32 [T,2] = (scene,
    instance), numpy or a device tensor; jitter f32 [T,8] (sample_jitter's rows) or None -> dict of device tensors img f32
    [T,3,H,W], mask f32 [T,1,H,W], bbox_gt f32 [T,1,5], heatmap f64 [T,1,hh,hw]: the rows pipeline.make_dtoid_sample +
    collate give for the same frames, less xyz (DtoidNet.forward reads none). One launch on the current stream; nothing
    is read back and nothing synchronises. Bad sizes raise ValueError before the device is touched."""
    sb = scene_batch                    # (the issue's parameter name is the function's own)
    _need(isinstance(sb, scenes.SceneBatch), "scene_batch must be a scenes.SceneBatch")
    H, W = sb.hw
    S, I = sb.layout.n_scenes, sb.layout.n_instances
    _need(len(tuple(heatmap_hw)) == 2 and int(heatmap_hw[0]) > 0 and int(heatmap_hw[1]) > 0,
          "heatmap_hw must be two positive sizes, got %r" % (tuple(heatmap_hw),))
    hh, hw = int(heatmap_hw[0]), int(heatmap_hw[1])
    shp = _shape(targets)
    _need(len(shp) == 2 and shp[1] == 2 and shp[0] >= 1, "targets must be [T,2] with T >= 1, got %s" % (shp,))
    T = shp[0]
    _need(jitter is None or _shape(jitter) == (T, 8), "jitter must be [T,8] = [%d,8], got %s" % (T, jitter is None or _shape(jitter)))
    _need(H > 0 and W > 0 and H * W < 1 << 30, "the frame must have 0 < H*W < 2^30 pixels, got %d x %d" % (H, W))
    _need(I >= 1, "the scene batch has no instance")
    _need(torch.is_tensor(sb.color) and torch.is_tensor(sb.instance) and torch.is_tensor(sb.gt_info),
          "scene_batch must hold device tensors (scenes.render_scenes), not host arrays")
    dev = sb.color.device
    from ..model_cloud import _refuse_cpu
    _refuse_cpu(dev)
    tg = targets if torch.is_tensor(targets) else torch.from_numpy(np.ascontiguousarray(targets, dtype=np.int32))
    tg = tg.to(dev, torch.int32).contiguous()
    jt = None
    if jitter is not None:                   # the seed column travels as bits: no arithmetic touches it on the way
        jt = jitter if torch.is_tensor(jitter) else torch.from_numpy(np.ascontiguousarray(jitter, dtype=np.float32))
        _need(jt.dtype == torch.float32, "jitter must be float32")
        jt = jt.to(dev).contiguous()
    color, inst, info = sb.color.contiguous(), sb.instance.contiguous(), sb.gt_info.contiguous()
    img = torch.empty(T, 3, H, W, dtype=torch.float32, device=dev)
    mask = torch.empty(T, 1, H, W, dtype=torch.float32, device=dev)
    bbox = torch.empty(T, 1, 5, dtype=torch.float32, device=dev)
    heat = torch.empty(T, 1, hh, hw, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_scene_dtoid_batch")(color.data_ptr(), inst.data_ptr(), info.data_ptr(), S, H, W, I, tg.data_ptr(), T,
                                                None if jt is None else jt.data_ptr(), hh, hw, HEATMAP_SIGMA, img.data_ptr(),
                                                mask.data_ptr(), bbox.data_ptr(), heat.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_scene_dtoid_batch")
    return {"img": img, "mask": mask, "bbox_gt": bbox, "heatmap": heat}


def select_targets(scene_batch, obj_ids=None, min_visib=MIN_VISIB, min_px=MIN_PX):
    """SPEC 15.4 -> int32 [n,2] = (scene, instance) rows, in draw-list order, of the instances that are not the table, are
    of an object in obj_ids (None: any), show at least min_px pixels and at least min_visib of their amodal pixels
    (px_count_visib / px_count_all in f64, the visib_fract frames() reports). Reads gt_info back once: the only sync."""
    _need(isinstance(scene_batch, scenes.SceneBatch), "scene_batch must be a scenes.SceneBatch")
    wanted = None if obj_ids is None else {int(o) for o in obj_ids}
    info = scenes._np(scene_batch.gt_info)
    atlas, layout = scene_batch.atlas, scene_batch.layout
    rows = []
    for s, i, _k in scene_batch._objects():
        if wanted is not None and int(atlas.obj_ids[layout.instance_mesh[i]]) not in wanted:
            continue
        n_all, n_visib = int(info[i, 0]), int(info[i, 1])
        if n_visib >= int(min_px) and scenes._visib_fract(n_visib, n_all) >= float(min_visib):
            rows.append((s, i))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def sample_jitter(T, rng, strength=1.0):
    """SPEC 15.5 (build-defined) -> f32 [T,8] = (g_r, g_g, g_b, b_r, b_g, b_b, a, seed) rows for scene_batch, drawn from the
    caller's Generator in this order: the common gain U(1 - 0.3s, 1 + 0.3s) [T], the per-channel gain
    U(1 - 0.1s, 1 + 0.1s) [T,3] (g = common * channel, in f64, rounded to f32), the bias U(-0.1s, 0.1s) [T,3], the noise
    amplitude U(0, 0.06s) [T], the seed, 32 random bits [T], stored as the f32 of those bits."""
    T, s = int(T), float(strength)
    _need(T >= 1, "T must be >= 1, got %r" % (T,))
    _need(isinstance(rng, np.random.Generator), "rng must be a numpy.random.Generator")
    _need(0.0 <= s <= 1.0, "strength must lie in [0, 1], got %r" % (strength,))
    common = rng.uniform(1.0 - 0.3 * s, 1.0 + 0.3 * s, T)
    channel = rng.uniform(1.0 - 0.1 * s, 1.0 + 0.1 * s, (T, 3))
    bias = rng.uniform(-0.1 * s, 0.1 * s, (T, 3))
    amp = rng.uniform(0.0, 0.06 * s, T)
    seed = rng.integers(0, 1 << 32, T, dtype=np.uint64).astype(np.uint32)
    out = np.empty((T, 8), dtype=np.float32)
    out[:, 0:3], out[:, 3:6], out[:, 6] = common[:, None] * channel, bias, amp
    out.view(np.uint32)[:, 7] = seed
    return out


def split_objects(obj_ids):
    """dtoid_dataset.py:38-39 -> (train ids, validation ids, shared): train on id % 4 != 0, validate on id % 4 == 0. When
    that leaves either side empty both sides are all the objects and shared is True: the caller validates on the training
    objects, on scenes of another seed, and says so."""
    ids = sorted({int(o) for o in obj_ids})
    _need(len(ids) >= 1 and ids[0] >= 1, "obj_ids must be integers >= 1, got %r" % (list(obj_ids),))
    train, val = [o for o in ids if o % 4 != 0], [o for o in ids if o % 4 == 0]
    if not train or not val:
        return ids, list(ids), True
    return train, val, False


class ScenePretrainSet:
    """An endless iterator of D14 batches (the dict DtoidNet.forward takes) of freshly rendered scenes, SPEC 15.6. Each
    refresh samples scenes_per_refresh layouts of objects_per_scene objects (scenes.sample_layouts, 13.7) and a sensor
    (13.8), renders them over a smooth random background per scene, selects the targets (select_targets) and shuffles them
    with the set's own Generator; they are cut into batches of batch_size, the incomplete last one dropped (drop_last).
    Per target the global template is a uniformly random view of its object and the local template the single closest
    view to the ground-truth rotation (dtoid_dataset.py:197-211), gathered on the device by index_select over the bank's
    views. A refresh that yields no batch draws again, at most MAX_REDRAWS times, then raises RuntimeError. Everything
    random comes from numpy.random.default_rng(seed): the same seed gives the same batches, bit for bit.

    bank: a pipeline.TemplateBank holding the templates and view quaternions (add_mesh) of every object trained on.
    obj_ids: the objects whose instances are targets (None: all of the atlas); the scenes hold all the atlas's objects
    either way. jitter: sample_jitter's strength, 0 or None for none. background=False leaves the background black.
    lights=True lights every refresh's scenes (scenes.sample_lights, SPEC 13.11-13.12) from a Generator of its own,
    derived from (seed, refresh number), so that no other draw moves: with the same seed the batches differ from the
    unlit set's in img alone. shadows=True (or a scenes.Shadows) lets those lights cast shadows (SPEC 13.13-13.15); it
    needs lights=True and draws nothing random: again img alone differs. rest=True rests every refresh's objects on a
    table (scenes.sample_layouts(placement="rest"), SPEC 13.16-13.18): other layouts from other draws, one more launch and
    one read-back per refresh, and once per object the support pass."""

    def __init__(self, atlas, bank, cam_K, hw, objects_per_scene, scenes_per_refresh, batch_size, seed, obj_ids=None,
                 jitter=1.0, heatmap_hw=(29, 39), min_visib=MIN_VISIB, min_px=MIN_PX, drop_last=True, background=True,
                 lights=False, shadows=False, rest=False):
        _need(isinstance(atlas, scenes.MeshAtlas), "atlas must be a scenes.MeshAtlas")
        self.rest = bool(rest)
        self.lights = bool(lights)
        self.shadows = shadows if isinstance(shadows, scenes.Shadows) else (scenes.Shadows() if shadows else None)
        _need(self.shadows is None or self.lights, "shadows are cast by lights: shadows needs lights=True")
        self.atlas, self.bank, self.cam_K = atlas, bank, np.asarray(cam_K, dtype=np.float64)
        self.hw = (int(hw[0]), int(hw[1]))
        _need(self.cam_K.shape == (3, 3), "cam_K must be [3,3]")
        _need(self.hw[0] > 0 and self.hw[1] > 0, "hw must be two positive sizes, got %r" % (tuple(hw),))
        self.n_objects, self.n_scenes, self.batch_size = int(objects_per_scene), int(scenes_per_refresh), int(batch_size)
        _need(self.n_objects >= 1 and self.n_scenes >= 1 and self.batch_size >= 1,
              "objects_per_scene, scenes_per_refresh and batch_size must be >= 1")
        objects = [o for o in atlas.obj_ids if o != scenes.TABLE_OBJ_ID]
        self.obj_ids = objects if obj_ids is None else sorted(int(o) for o in obj_ids)
        _need(len(self.obj_ids) >= 1 and set(self.obj_ids) <= set(objects), "obj_ids must name objects of the atlas, got %r" % (self.obj_ids,))
        missing = [o for o in self.obj_ids if o not in bank.img or o not in bank.quats]
        _need(not missing, "the template bank lacks templates or view rotations of objects %s (TemplateBank.add_mesh)" % missing)
        self.jitter = 0.0 if jitter is None else float(jitter)
        _need(0.0 <= self.jitter <= 1.0, "jitter must lie in [0, 1], got %r" % (jitter,))
        self.heatmap_hw = (int(heatmap_hw[0]), int(heatmap_hw[1]))
        self.min_visib, self.min_px, self.drop_last, self.background = float(min_visib), int(min_px), bool(drop_last), bool(background)
        self.seed, self.rng = int(seed), np.random.default_rng(int(seed))
        self.refreshes, self.render_batch = 0, None
        self._queue = []
        # the views of every object back to back: one index_select per batch gathers templates of mixed objects
        self._first, n = {}, 0
        for o in self.obj_ids:
            self._first[o], n = n, n + int(bank.img[o].shape[0])
        self._views = {o: int(bank.img[o].shape[0]) for o in self.obj_ids}
        self._timg = torch.cat([bank.img[o] for o in self.obj_ids])
        self._tmask = torch.cat([bank.mask[o] for o in self.obj_ids])

    def __iter__(self):
        return self

    def _backgrounds(self, S):
        """u8 [S,H,W,3] on the device: synth._smooth_field per scene on a grid of 16-pixel cells, enlarged bilinearly on
        the device. The field is host numpy and its cost grows with the pixel count; profiles/pretrain_producer.json
        splits a refresh into its parts, this one among them."""
        H, W = self.hw
        h, w = (H + 15) // 16, (W + 15) // 16
        small = np.stack([synth._smooth_field(self.rng, h, w, 3, 1) for _ in range(S)]).astype(np.float32)
        t = torch.from_numpy(small).to(self.atlas.device).permute(0, 3, 1, 2)
        t = torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)
        return (t * 255.0).round_().clamp_(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def draw_targets(self):
        """The first draws of a refresh -> (layout, sensor), host only unless the set rests its objects (then the drop's
        launch and read-back). The backgrounds, then plan's draws, follow."""
        layout = scenes.sample_layouts(self.atlas, self.n_scenes, self.n_objects, self.cam_K, self.hw, self.rng,
                                       placement="rest" if self.rest else "free")
        sensor = scenes.sample_sensor(self.n_scenes, self.hw, self.rng)
        return layout, sensor

    def plan(self, layout, targets):
        """The shuffle, template choice and jitter of a refresh (host only): targets int32 [n,2] in draw-list order ->
        (targets in batch order, global view ids, local view ids -- both indices into the set's concatenated views --,
        obj ids, jitter rows or None). Draw order: the permutation, per target the global view, then the jitter rows."""
        order = self.rng.permutation(len(targets))
        targets = np.ascontiguousarray(targets[order])
        objs = np.array([self.atlas.obj_ids[layout.instance_mesh[i]] for _s, i in targets], dtype=np.int64)
        gidx = np.array([self._first[o] + int(self.rng.integers(self._views[o])) for o in objs], dtype=np.int64)
        lidx = np.array([self._first[o] + int(self.bank.nearest_views(o, layout.transforms[i][:3, :3])[0])
                         for o, (_s, i) in zip(objs, targets)], dtype=np.int64)
        jit = sample_jitter(len(targets), self.rng, self.jitter) if self.jitter > 0.0 and len(targets) else None
        return targets, gidx, lidx, objs, jit

    def _refresh(self):
        for _ in range(MAX_REDRAWS):
            layout, sensor = self.draw_targets()
            bg = self._backgrounds(self.n_scenes) if self.background else None
            lights = material = None
            if self.lights:
                # a stream of its own per refresh: the set's Generator, and with it every other draw, is untouched
                lrng = np.random.default_rng(np.random.SeedSequence(self.seed, spawn_key=(self.refreshes,)))
                lights, material = scenes.sample_lights(layout, lrng)
            batch = scenes.render_scenes(self.atlas, layout, self.hw, background=bg, sensor=sensor, lights=lights,
                                         material=material, shadows=self.shadows)
            self.refreshes += 1
            targets = select_targets(batch, self.obj_ids, self.min_visib, self.min_px)
            n = len(targets) // self.batch_size * self.batch_size if self.drop_last else len(targets)
            if n == 0:
                continue
            targets, gidx, lidx, objs, jit = self.plan(layout, targets)
            dev = self.atlas.device
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)    # one upload per array and refresh
            d_t, d_g, d_l, d_j = up(targets), up(gidx), up(lidx), up(jit)
            self.render_batch = batch
            for k in range(0, n, self.batch_size):
                e = min(k + self.batch_size, n)
                self._queue.append((batch, d_t[k:e], d_g[k:e], d_l[k:e], None if d_j is None else d_j[k:e], objs[k:e], targets[k:e]))
            return
        raise RuntimeError("ScenePretrainSet: %d refreshes in a row gave no batch of %d eligible targets (min_visib %g, min_px "
                           "%d, %d scenes of %d objects)" % (MAX_REDRAWS, self.batch_size, self.min_visib, self.min_px,
                                                             self.n_scenes, self.n_objects))

    def __next__(self):
        if not self._queue:
            self._refresh()
        batch, d_t, d_g, d_l, d_j, objs, targets = self._queue.pop(0)
        out = scene_batch(batch, d_t, self.heatmap_hw, d_j)
        out["gimg"], out["gmask"] = self._timg.index_select(0, d_g), self._tmask.index_select(0, d_g)
        out["limg"], out["lmask"] = self._timg.index_select(0, d_l), self._tmask.index_select(0, d_l)
        out["obj_id"], out["targets"] = objs, targets                          # host arrays: who is in the batch
        return out


class DtoidPretrainer:
    """The training loop of train.py on a ScenePretrainSet: the online loop's optimiser and step
    (online_learning.py:258-263, :650-679; finetune.FlatParams + FusedAMSGrad + finetune_step) in train mode, validation
    by numbers the model and det_eval already produce, and the checkpoint online_learning.py:161-162 loads."""

    def __init__(self, model, train_set, val_set=None, lr=1e-4, weight_decay=1e-6):
        _lib.require_cuda(next(model.parameters()))
        self.model, self.train_set, self.val_set = model, train_set, val_set
        self.flat = finetune.FlatParams(model)
        self.optimizer = finetune.FusedAMSGrad(self.flat, lr=lr, weight_decay=weight_decay)
        self.iteration = 0

    def step(self):
        """One optimiser step on the train set's next batch -> the detached loss (a device scalar)."""
        self.model.train()
        loss = finetune.finetune_step(self.model, next(self.train_set), self.optimizer)
        self.iteration += 1
        return loss

    def validate(self, n_batches=4):
        """-> {"seg_IoU": the mean over the targets of n_batches validation batches of DtoidNet.forward's seg_IoU in eval
        mode, "AP": the 11-point AP at IoU 0.5 (det_eval, SPEC 10) of forwardTestTime's best box per validation target,
        all the bank's test views as local templates, against the target's bbox_visib box, one class (a target for
        which no box comes back has no detection), "n": the targets}."""
        from .. import det_eval
        _need(self.val_set is not None, "validate needs a val_set")
        model, bank = self.model, self.val_set.bank
        was_training = model.training
        model.eval()
        model.clearCache()
        ious, det_box, det_score, det_image, gt_box = [], [], [], [], []
        with torch.no_grad():
            for _ in range(int(n_batches)):
                b = next(self.val_set)
                ious.append(model(b)["seg_IoU"].reshape(1) * len(b["obj_id"]))        # a batch's mean, weighted by its size
                for k, o in enumerate(b["obj_id"]):
                    limg, lmask = bank.all_local(int(o))
                    out = model.forwardTestTime({"img": b["img"][k:k + 1], "limg": limg[None], "lmask": lmask[None], "obj_id": [int(o)]})
                    scores = out["pred_scores"].reshape(-1)
                    if scores.numel():                                                 # no box at all: a target without a detection
                        top = scores.argmax()
                        det_box.append(out["pred_bbox"].reshape(-1, 4)[top].reshape(1, 4))
                        det_score.append(scores[top].reshape(1))
                        det_image.append(len(gt_box))
                    gt_box.append(b["bbox_gt"][k, :, :4])
        model.clearCache()
        model.train(was_training)
        n, nd = len(gt_box), len(det_box)
        boxes = torch.cat(det_box).float().cpu().numpy() if nd else np.zeros((0, 4), np.float32)
        scores = torch.cat(det_score).float().cpu().numpy() if nd else np.zeros(0, np.float32)
        if nd == 0:
            return {"seg_IoU": float(torch.cat(ious).sum()) / n, "AP": 0.0, "n": n}
        res = det_eval.evaluate({"boxes": boxes, "scores": scores, "classes": np.zeros(nd, np.int64), "images": np.asarray(det_image, np.int64)},
                                {"boxes": torch.cat(gt_box).cpu().numpy(), "classes": np.zeros(n, np.int64), "images": np.arange(n, dtype=np.int64)},
                                ["object"], iou_thresholds=(0.5,), n_images=n)
        return {"seg_IoU": float(torch.cat(ious).sum()) / n, "AP": float(res["AP11"][0, 0]), "n": n}

    def save(self, path):
        """{"state_dict", "iteration", "optimizer"}: the first is what online_learning.py:161-162 loads. The parameters are
        views of one flat buffer; they are saved as tensors of their own."""
        state = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        torch.save({"state_dict": state, "iteration": self.iteration, "optimizer": self.optimizer.state_dict()}, path)

    def load(self, path):
        """Resume from save's file: weights and buffers, the optimiser's moments and step, the iteration. The train set's
        own state is the caller's (a set of the same seed, advanced by as many batches, continues the same run)."""
        ckpt = torch.load(path, map_location=self.flat.param.device)
        self.model.load_state_dict(ckpt["state_dict"])        # copies into the flat buffer's views: nothing is re-homed
        opt = ckpt["optimizer"]
        for name in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            getattr(self.optimizer, name).copy_(opt[name])
        self.optimizer.step_count = int(opt["step"])
        self.iteration = int(ckpt["iteration"])
        from . import network
        network.PARAM_EPOCH[0] += 1                            # packed test-time plans are rebuilt from the new weights
        self.model.clearCache()
        return self
