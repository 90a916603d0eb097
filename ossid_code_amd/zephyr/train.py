"""Fitting PointNet2SSG on this build's own features (SPEC.md 12).

The reference only LOADS scorer checkpoints (scripts/online_learning.py:171-227); they were trained by the un-vendored
`zephyr` package on its own featurizer, and neither its training loop nor its loss is in the reference tree. Everything here
is therefore build-defined and unpinned: the loss below is a plain choice, not zephyr's.

Plain torch on [B] vectors: the hot path is the module's training-mode forward and backward (csrc/pn2_train.hip).
"""
import numpy as np
import torch
import torch.nn.functional as F

from ..hostutil import K2meta
from . import score_dataset as _sd


def scorer_loss(scores, pp_err, sigma=0.01):
    """binary_cross_entropy_with_logits(scores[:, 0], exp(-pp_err / sigma)): a hypothesis at the ground truth has target 1,
    one sigma (metres of ADD / ADI) away 1/e. With this loss the reference's `> 20` confidence threshold is not calibrated
    (OnlineStream takes confident_threshold from the caller)."""
    pp_err = torch.as_tensor(pp_err, dtype=scores.dtype, device=scores.device)
    return F.binary_cross_entropy_with_logits(scores[:, 0], torch.exp(-pp_err / sigma))


class ScorerTrainer:
    """One optimisation step per frame: featurize every hypothesis (no free-space filtering in training), draw the dropout
    mask on the host, forward, loss, backward, optimizer.step()."""

    def __init__(self, model, dataset, optimizer, loss_fn=scorer_loss, generator=None):
        self.model, self.dataset, self.optimizer, self.loss_fn, self.generator = model, dataset, optimizer, loss_fn, generator

    def featurize(self, data):
        """data: the dict networkInference takes -> point_x [N, M, 8] on the model's device."""
        dev = self.model.device
        img = data["img"]
        img = img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img))
        with torch.no_grad():
            rgbd = _sd.stage_frame(img, data["depth"], dev, blur=img.dtype == torch.uint8)
            tab = _sd.stage_model(data["model_points"], data["model_normals"], data["model_colors"], dev)
            T = _sd._f32(data["pose_hypos"], dev).reshape(-1, 4, 4)
            px, _ = _sd.featurize(rgbd, T, tab, _sd._cam(K2meta(data["cam_K"])), interp=getattr(self.dataset, "interp", 0),
                                  want_uv=False)
        return px

    def step_features(self, point_x, pp_err):
        """The step on ready features; returns the loss as a float."""
        self.model.train()
        keep = self.model.draw_keep_mask(point_x.shape[0], self.generator)
        self.optimizer.zero_grad(set_to_none=True)
        scores = self.model({"point_x": point_x}, keep_mask=keep)
        loss = self.loss_fn(scores, pp_err)
        loss.backward()
        self.optimizer.step()
        return float(loss.detach())

    def step(self, data):
        if "pp_err" not in data:
            raise ValueError("training needs data['pp_err'] (scoring.pose_errors)")
        return self.step_features(self.featurize(data), data["pp_err"])
