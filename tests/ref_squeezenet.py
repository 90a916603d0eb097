"""Plain float64 restatement of DTOID's two SqueezeNet-1.1 template encoders in training mode, the yardstick of
ossid_code_amd/dtoid/train_encoders.py (TemplateEncoderTrain).

TemplateFeatExtract: 4-channel 3x3/s2 stem -> ReLU -> max-pool -> Fire x2 -> (tap 1, 128 x 30 x 30) -> max-pool -> Fire x2
-> max-pool -> Fire x4 -> (tap 2, 512 x 7 x 7); output cat(BN(tap 2), bilinear 30 -> 7 of BN(tap 1)). TemplateFeatExtractGlobal
adds two VALID 3x3 convolutions, each followed by ELU and a training BatchNorm. Max-pools are 3/2/0 with ceil_mode; every
BatchNorm normalises by the batch's biased variance and moves its running statistics by the unbiased one.

Written with torch double ops on the CPU, functionally over the module's parameters. The piecewise-linear decisions -- one
mask per ReLU, one argmax per max-pool window -- can be supplied from outside (a float32 device run's), in which case the
restatement follows them instead of taking its own: the result is then the float64 value of the function the device
differentiated, and it is continuous in the inputs, so a device run can be held to hard bounds against it even where a
decision sits within rounding of its kink. Every decision also comes back with its float64 margin (|pre-activation| for a
ReLU, top-1 minus top-2 of the window for a max-pool) and its layer's scale.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


def pool_out(n, k, stride, pad, ceil_mode):
    """nn.MaxPool2d's output size (a ceil-mode window must start inside the input or its left padding)."""
    o = -(-(n + 2 * pad - k) // stride) + 1 if ceil_mode else (n + 2 * pad - k) // stride + 1
    return o - 1 if ceil_mode and (o - 1) * stride >= n + pad else o


def pool_windows(x, k, stride, pad, ceil_mode):
    """x [B,C,H,W] -> windows [B,C,Ho,Wo,k*k] (position dy * k + dx); positions outside the input hold -inf."""
    B, C, H, W = x.shape
    Ho, Wo = pool_out(H, k, stride, pad, ceil_mode), pool_out(W, k, stride, pad, ceil_mode)
    Hp, Wp = (Ho - 1) * stride + k, (Wo - 1) * stride + k
    xp = F.pad(x, (pad, Wp - W - pad, pad, Hp - H - pad), value=float("-inf"))
    return xp.unfold(2, k, stride).unfold(3, k, stride).reshape(B, C, Ho, Wo, k * k)


def maxpool(x, k, stride, pad, ceil_mode, argmax=None):
    """Max-pool by gathering each window at its argmax (first maximum wins unless `argmax` [B,C,Ho,Wo] is given).
    -> (y, argmax used, own argmax, margin = top-1 minus top-2 of each window)."""
    win = pool_windows(x, k, stride, pad, ceil_mode)
    wd = win.detach()
    own = wd.argmax(-1)                                   # (first occurrence of the maximum)
    top = wd.topk(2, dim=-1).values
    margin = top[..., 0] - top[..., 1]
    use = own if argmax is None else argmax.to(torch.int64)
    return win.gather(-1, use.unsqueeze(-1)).squeeze(-1), use, own, margin


class _Run:
    def __init__(self, decisions):
        self.given = decisions or {}
        self.own, self.margin, self.scale = {}, {}, {}

    def relu(self, name, p):
        pd = p.detach()
        self.own[name] = pd > 0
        self.margin[name] = pd.abs()
        self.scale[name] = float(pd.abs().max())
        m = self.given.get(name)
        return p * (self.own[name] if m is None else m.to(torch.bool)).to(p.dtype)

    def pool(self, name, x, k, stride, pad, ceil_mode):
        y, _, own, margin = maxpool(x, k, stride, pad, ceil_mode, self.given.get(name))
        self.own[name], self.margin[name] = own, margin
        self.scale[name] = float(x.detach().abs().max())
        return y


def batchnorm_train(x, weight, bias, running_mean, running_var, eps, momentum):
    """Training BatchNorm2d: (y, new running mean, new running var)."""
    n = x.numel() // x.shape[1]
    mean = x.mean((0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
    y = (x - mean.view(1, -1, 1, 1)) / torch.sqrt(var + eps).view(1, -1, 1, 1) * weight.view(1, -1, 1, 1) + bias.view(1, -1, 1, 1)
    rm = (1 - momentum) * running_mean + momentum * mean.detach()
    rv = (1 - momentum) * running_var + momentum * var.detach() * n / (n - 1)
    return y, rm, rv


def encoder_train(mod, img, gout, decisions=None, buffers=None):
    """One training pass of a TemplateFeatExtract / TemplateFeatExtractGlobal `mod` on templates `img` [B,4,h,w], its
    output differentiated against `gout`, all in float64 on the CPU.

    decisions: optional {name: tensor} -- a bool mask per ReLU ("stem", "<stage>.squeeze", "<stage>.expand" -- the latter
    over cat(expand1x1, expand3x3)) and an argmax [B,C,Ho,Wo] (window position dy * k + dx) per max-pool ("<stage>"), where
    <stage> is the child's name, e.g. "backbone_1.1"; a name left out takes the restatement's own decision.
    buffers: optional {name: tensor} of running statistics to start from (default: the module's).
    Returns a dict: out, grads {parameter name: gradient} (the parameters the pass uses), running {buffer name: new value},
    decisions (its own), margin and scale {decision name: ...}."""
    # (by identity: the Fire modules are shared with mod.backbone, whose names named_parameters() reports for them)
    P = {id(p): p.detach().double().cpu().clone().requires_grad_(True) for p in mod.parameters()}
    prm = lambda name: P[id(mod.get_parameter(name))]      # noqa: E731
    bufs = {n: b.detach().double().cpu().clone() for n, b in mod.named_buffers() if b.dtype.is_floating_point}
    if buffers is not None:
        bufs.update({n: b.detach().double().cpu().clone() for n, b in buffers.items() if b.dtype.is_floating_point})
    run = _Run(decisions)
    running = {}

    def bn(name, x):
        m = mod.get_submodule(name)
        mom = 0.1 if m.momentum is None else m.momentum
        y, rm, rv = batchnorm_train(x, prm(name + ".weight"), prm(name + ".bias"), bufs[name + ".running_mean"],
                                    bufs[name + ".running_var"], m.eps, mom)
        running[name + ".running_mean"], running[name + ".running_var"] = rm, rv
        return y

    def conv(name, x, **kw):
        return F.conv2d(x, prm(name + ".weight"), prm(name + ".bias"), **kw)

    x = run.relu("stem", conv("backbone_0.0", img.detach().double().cpu(), stride=2))
    taps = []
    for part in ("backbone_1", "backbone_2"):
        for j, m in enumerate(mod.get_submodule(part)):
            name = "%s.%d" % (part, j)
            if isinstance(m, nn.MaxPool2d):
                g = lambda v: v if isinstance(v, int) else v[0]      # noqa: E731
                x = run.pool(name, x, g(m.kernel_size), g(m.stride), g(m.padding), bool(m.ceil_mode))
            elif isinstance(m, nn.ReLU):
                continue                                              # the stem's, applied above
            else:
                s = run.relu(name + ".squeeze", conv(name + ".squeeze", x))
                x = run.relu(name + ".expand", torch.cat([conv(name + ".expand1x1", s), conv(name + ".expand3x3", s, padding=1)], 1))
        taps.append(x)
    x1, x2 = taps
    x1n, x2n = bn("norm_1", x1), bn("norm_2", x2)
    out = torch.cat([x2n, F.interpolate(x1n, size=(x2.shape[2], x2.shape[3]), mode="bilinear", align_corners=False)], 1)
    if hasattr(mod, "final_conv_1"):
        out = bn("final_norm_1", F.elu(conv("final_conv_1", out)))
        out = bn("final_norm_2", F.elu(conv("final_conv_2", out)))
    out.backward(gout.detach().double().cpu())
    grads = {n: P[id(p)].grad for n, p in mod.named_parameters() if P[id(p)].grad is not None}
    return dict(out=out.detach(), grads=grads, running=running, decisions=run.own, margin=run.margin, scale=run.scale)
