"""Plain float64 restatement of DTOID's image backbone (ImageFeatExtract) in training mode, the yardstick of
Network._backbone_train_hip (ossid_code_amd/dtoid/network.py) and of the kernels under it (csrc/stem.hip, csrc/conv.hip,
csrc/dense_bwd.hip, csrc/train.hip).

conv0 (7x7 / stride 2 / pad 3, no bias) -> x0 + dw_xcorr(x0, g), g [B or 1, 64, 3, 3] the global template feature ->
norm0 - ReLU - MaxPool(3, 2, 1) -> denseblock1 (6 layers) -> transition1 -> denseblock2 (12) -> transition2 -> denseblock3 (24)
-> transition3 -> denseblock4 (16) -> norm5 (no ReLU) -> c1 (1x1, 1024 -> 640, bias) -> ELU -> n1. A dense layer is norm1 -
ReLU - 1x1 - norm2 - ReLU - 3x3 on the concatenation of everything before it; a transition is norm - ReLU - 1x1 -
AvgPool(2, 2), transition3's pool with stride 1. Every BatchNorm normalises by the batch's biased variance and moves its
running statistics by the unbiased one.

Written with torch ops on the CPU, functionally over the module's parameters, in the style of tests/ref_squeezenet.py, whose
_Run, maxpool and batchnorm_train it uses. The piecewise-linear decisions -- one mask per ReLU ("norm0",
"denseblock3.denselayer7.norm2", "transition2.norm", ...), one argmax per max-pool window ("pool0") -- can be supplied from
outside (a float32 device run's); the result is then the float64 value of the function the device differentiated. With
dtype=torch.float32 the same code runs in float32 on the same decisions: the distance of that run from the float64 one is
the error of plain float32 arithmetic on this function, the yardstick a device run is bounded by.
"""
import torch
import torch.nn.functional as F

from ref_squeezenet import _Run, batchnorm_train

# decision / stage name -> the child of ImageFeatExtract that holds it (torchvision's densenet121 child order, cut in three)
STAGES = {"conv0": "backdense_0.0", "norm0": "backdense_1.0", "denseblock1": "backdense_1.3", "transition1": "backdense_2.0",
          "denseblock2": "backdense_2.1", "transition2": "backdense_2.2", "denseblock3": "backdense_2.3",
          "transition3": "backdense_2.4", "denseblock4": "backdense_2.5", "norm5": "backdense_2.6", "c1": "c1", "n1": "n1"}
BLOCK_LAYERS = {"denseblock1": 6, "denseblock2": 12, "denseblock3": 24, "denseblock4": 16}


def module_name(name):
    """"denseblock3.denselayer7.norm2" -> "backdense_2.3.denselayer7.norm2" (the name ImageFeatExtract reports)."""
    head, _, rest = name.partition(".")
    return STAGES[head] + ("." + rest if rest else "")


def decision_names():
    """Every decision of one pass, in forward order."""
    names = ["norm0", "pool0"]
    for i in (1, 2, 3, 4):
        blk = "denseblock%d" % i
        for li in range(1, BLOCK_LAYERS[blk] + 1):
            names += ["%s.denselayer%d.norm1" % (blk, li), "%s.denselayer%d.norm2" % (blk, li)]
        if i < 4:
            names.append("transition%d.norm" % i)
    return names


def dw_xcorr(x, k):
    """x [B,C,H,W] + per-image, per-channel 3x3 cross-correlation with k [B or 1,C,3,3], padding 1."""
    B, C, H, W = x.shape
    kk = k.expand(B, -1, -1, -1).reshape(B * C, 1, 3, 3)
    return F.conv2d(x.reshape(1, B * C, H, W), kk, padding=1, groups=B * C).view(B, C, H, W)


def backbone_train(ife, image, g, gout, decisions=None, buffers=None, dtype=torch.float64, pool_stride=None):
    """One training pass of the ImageFeatExtract `ife` on `image` [B,3,H,W] and the global template feature `g`
    [B or 1,64,3,3], its output differentiated against `gout`, in `dtype` on the CPU.

    decisions: optional {name: tensor} -- a bool mask per ReLU, an argmax [B,64,Ho,Wo] (window position dy * 3 + dx, the
    window starting one pixel outside) for "pool0"; a name left out takes the pass's own decision.
    buffers: optional {buffer name: tensor} of running statistics to start from (default: the module's).
    pool_stride: optional {"transition3": 2, ...} -- a deliberately different function, for the tests' sensitivity checks.
    Returns a dict: out, grads {parameter name: gradient, "g": the gradient with respect to g}, running {buffer name: new
    value}, decisions (its own), margin and scale {decision name: ...}, pre {decision name: the value decided on -- a ReLU's
    input, the max-pool's input}."""
    cvt = lambda t: t.detach().to(dtype).cpu().clone()      # noqa: E731
    P = {n: cvt(p).requires_grad_(True) for n, p in ife.named_parameters()}
    bufs = {n: cvt(b) for n, b in ife.named_buffers() if b.dtype.is_floating_point}
    if buffers is not None:
        bufs.update({n: cvt(b) for n, b in buffers.items() if b.dtype.is_floating_point})
    gk = cvt(g).requires_grad_(True)
    run = _Run(decisions)
    running, pre = {}, {}

    def bn(name, x):
        mn = module_name(name)
        m = ife.get_submodule(mn)
        mom = 0.1 if m.momentum is None else m.momentum
        y, rm, rv = batchnorm_train(x, P[mn + ".weight"], P[mn + ".bias"], bufs[mn + ".running_mean"], bufs[mn + ".running_var"],
                                    m.eps, mom)
        running[mn + ".running_mean"], running[mn + ".running_var"] = rm, rv
        return y

    def bn_relu(name, x):
        p = bn(name, x)
        pre[name] = p.detach()
        return run.relu(name, p)

    def weight(name):
        return P[module_name(name) + ".weight"]

    x0 = F.conv2d(cvt(image), weight("conv0"), stride=2, padding=3)
    x = bn_relu("norm0", x0 + dw_xcorr(x0, gk))
    pre["pool0"] = x.detach()
    x = run.pool("pool0", x, 3, 2, 1, False)
    for i in (1, 2, 3, 4):
        blk = "denseblock%d" % i
        for li in range(1, BLOCK_LAYERS[blk] + 1):
            ln = "%s.denselayer%d" % (blk, li)
            y = F.conv2d(bn_relu(ln + ".norm1", x), weight(ln + ".conv1"))
            x = torch.cat([x, F.conv2d(bn_relu(ln + ".norm2", y), weight(ln + ".conv2"), padding=1)], 1)
        if i < 4:
            tn = "transition%d" % i
            stride = (pool_stride or {}).get(tn, 1 if i == 3 else 2)
            x = F.avg_pool2d(F.conv2d(bn_relu(tn + ".norm", x), weight(tn + ".conv")), 2, stride)
    out = bn("n1", F.elu(F.conv2d(bn("norm5", x), P["c1.weight"], P["c1.bias"])))
    go = cvt(gout)
    if go.shape != out.shape:                               # (only under pool_stride)
        go = go[:, :, :out.shape[2], :out.shape[3]].contiguous()
    out.backward(go)
    grads = {n: p.grad for n, p in P.items()}
    grads["g"] = gk.grad
    return dict(out=out.detach(), grads=grads, running=running, decisions=run.own, margin=run.margin, scale=run.scale, pre=pre)
