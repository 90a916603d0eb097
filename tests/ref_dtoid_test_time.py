"""A float64 restatement of DTOID's TEST-TIME path at its real sizes (test infrastructure only).

The repo's own modules -- ImageFeatExtract, both SqueezeNet template encoders, CorrelationModel, ClassificationModel,
RegressionModel -- deep-copied to float64 and run on the CPU under oracle.dtoid_oracle.cpu_ops(), with
normalizeImageRange in front of the image. In eval mode nothing before post-processing takes a hard decision (ReLU,
max-pool values, ELU, sigmoid are continuous, BatchNorm is a fixed affine, nearest up-sampling a fixed index map), so a
float32 implementation has to agree with this element by element to float32-level accuracy.

Two things are restated rather than taken from torch:
  - the nearest up-sampling of the decoder gathers with the product's own index map, min(floorf(dst * ((float)src /
    dst)), src - 1) evaluated in float32 (csrc/segtail.hip src_index, csrc/conv.hip's fused up-sampling): `up_index`.
    tests/test_ref_dtoid_test_time.py holds that map to F.interpolate(mode="nearest") on float32 index-coded tensors;
  - the network's BatchNorm statistics: random weights with arbitrary statistics make 120 chained layers vanish or
    explode, so `build_network` calibrates every BatchNorm of the backbone and the encoders with one float64 pass over a
    calibration image (each takes its input's batch statistics, as a train-mode pass with momentum=None stores them) and
    shrinks `running_var` of a few channels (PERTURB) so that the error amplification of a small variance is exercised. The head carries gen_golden_dtoid.seeded_state weights, the
    weights of the stored reference fixtures tests/golden/dtoid_head_full*.npz.
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_dtoid import seeded_state  # noqa: E402

from oracle import dtoid_oracle  # noqa: E402
from ossid_code_amd import dtoid  # noqa: E402
from ossid_code_amd.dtoid.backbones import DenseBlock, Transition  # noqa: E402
from ossid_code_amd.dtoid.model import normalizeImageRange  # noqa: E402

IMG, GRID = (480, 640), (29, 39)
TEMPLATE = 124
HEAD_SEED = 4321          # the seed of tests/golden/dtoid_head_full.npz and dtoid_head_full_nt21.npz
NET_SEED = 77             # torch.manual_seed of the backbone / encoder initialisation
CAL_SEED = 5              # calibration image and templates
# BatchNorm channels whose calibrated running_var is divided by 100: (module path, channels)
PERTURB = [
    ("image_feature_extractor.backdense_1.0", (3, 40)),                                  # norm0
    ("image_feature_extractor.backdense_1.3.denselayer3.norm1", (7, 100)),
    ("image_feature_extractor.backdense_2.3.denselayer10.norm2", (5,)),
    ("image_feature_extractor.backdense_2.2.norm", (11, 400)),                          # transition2
    ("image_feature_extractor.backdense_2.6", (17,)),                                    # norm5
    ("template_feature_extractor.norm_2", (9,)),
]


def up_index(n_src, n_dst):
    """The product's nearest index along one axis: min(floorf(dst * ((float)n_src / (float)n_dst)), n_src - 1), float32."""
    scale = np.float32(n_src) / np.float32(n_dst)
    idx = np.floor(np.arange(n_dst, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, n_src - 1))


def nearest(x, size):
    """F.interpolate(x, size, mode="nearest") as an explicit gather with up_index (any dtype)."""
    iy, ix = up_index(x.shape[2], int(size[0])), up_index(x.shape[3], int(size[1]))
    return x[:, :, iy][:, :, :, ix]


def build_network(img_size=IMG, heatmap_size=GRID, head_seed=HEAD_SEED):
    """dtoid.Network (float32, CPU, eval) with seeded backbone / encoders, calibrated and perturbed BatchNorm statistics and
    the fixtures' head weights. Deterministic: the GPU tests build the same network."""
    torch.manual_seed(NET_SEED)
    net = dtoid.Network(img_size=img_size, heatmap_size=heatmap_size)
    for i, m in enumerate((net.correlation_model, net.classification, net.regression)):
        m.load_state_dict(seeded_state(m, head_seed + i))
    # every BatchNorm of the backbone and the encoders gets an affine of its own (torch initialises all of them to 1 / 0:
    # two dense layers' norm1 over the same channels would then be interchangeable, and a kernel reading the wrong one
    # would go unnoticed)
    g = torch.Generator().manual_seed(NET_SEED + 1)
    with torch.no_grad():
        for mod in (net.image_feature_extractor, net.template_feature_extractor, net.template_feature_extractor_global):
            for bn in mod.modules():
                if isinstance(bn, nn.BatchNorm2d):
                    bn.weight.copy_(1.0 + 0.2 * torch.randn(bn.weight.shape, generator=g))
                    bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=g))
    calibrate(net)
    return net.eval()


def calibration_inputs():
    """(image [1,3,480,640], templates [4,4,124,124]): the calibration pass's input. Template 0 is also the global template
    of every make_inputs set: the global template modulates the stem, and statistics calibrated under one global template
    do not hold under another one of this randomly initialised network (the final map grew from std 1 to 30)."""
    g = torch.Generator().manual_seed(CAL_SEED)
    img = torch.rand(1, 3, *IMG, generator=g)
    rgb = torch.rand(4, 3, TEMPLATE, TEMPLATE, generator=g)
    mask = (torch.rand(4, 1, TEMPLATE, TEMPLATE, generator=g) > 0.3).float()
    return img, template_batch(rgb, mask), (rgb, mask)


def template_batch(rgb, mask):
    """[n,4,h,w] encoder input from [0, 1] templates and their masks (DtoidNet._template_features)."""
    return torch.cat([normalizeImageRange(rgb), mask], 1)


def _calibrate_one(mod, prefix, *args):
    """One float64 pass of a copy of `mod` in which every BatchNorm, just before it runs, takes its input's batch mean and
    (unbiased) variance as running statistics -- what a train-mode pass with momentum=None stores -- with the PERTURB
    channels' variance divided by 100 right there, so that every later BatchNorm is calibrated on the perturbed
    activations. (Perturbing after a plain train-mode pass instead leaves the later layers' statistics stale: the
    final feature map then reached 4e3.) The statistics are copied back into `mod`; returns the float64 copy."""
    m64 = copy.deepcopy(mod).double().eval()
    small = {prefix + n: c for n, c in PERTURB}
    names = {b: n for n, b in m64.named_modules() if isinstance(b, nn.BatchNorm2d)}

    def hook(bn, inp):
        x = inp[0]
        bn.running_mean.copy_(x.mean((0, 2, 3)))
        bn.running_var.copy_(x.var((0, 2, 3), unbiased=True))
        chans = small.get(prefix + names[bn])
        if chans is not None:
            bn.running_var[list(chans)] *= 0.01
    handles = [b.register_forward_pre_hook(hook) for b in names]
    with torch.no_grad(), dtoid_oracle.cpu_ops():
        m64(*[a.double() for a in args])
    for h in handles:
        h.remove()
    with torch.no_grad():
        for dst, src in zip([b for b in mod.modules() if isinstance(b, nn.BatchNorm2d)], names):
            dst.running_mean.copy_(src.running_mean)
            dst.running_var.copy_(src.running_var)
    return m64


def calibrate(net):
    img, tmpl, _ = calibration_inputs()
    _calibrate_one(net.template_feature_extractor, "template_feature_extractor.", tmpl)
    gmod = _calibrate_one(net.template_feature_extractor_global, "template_feature_extractor_global.", tmpl[:1])
    with torch.no_grad(), dtoid_oracle.cpu_ops():
        g = gmod(tmpl[:1].double())
    _calibrate_one(net.image_feature_extractor, "image_feature_extractor.", normalizeImageRange(img.double()), g)


class Ref64:
    """Float64 copies of a Network's modules (built once; the Network itself is left untouched)."""

    def __init__(self, net):
        self.ife = copy.deepcopy(net.image_feature_extractor).double().eval()
        self.enc_local = copy.deepcopy(net.template_feature_extractor).double().eval()
        self.enc_global = copy.deepcopy(net.template_feature_extractor_global).double().eval()
        self.corr = copy.deepcopy(net.correlation_model).double().eval()
        self.cls = copy.deepcopy(net.classification).double().eval()
        self.reg = copy.deepcopy(net.regression).double().eval()

    def backbone(self, image, g, raw=True, taps=None):
        """image [B,3,H,W] (in [0, 1] when raw), g [1 or B,64,3,3] -> [B,640,h,w]. taps: pool0, each dense block's whole
        output, each transition, the final map -- FusedBackbone's taps."""
        ife = self.ife
        x = image.double()
        if raw:
            x = normalizeImageRange(x)
        g = g.double()
        if g.shape[0] == 1 and x.shape[0] > 1:
            g = g.expand(x.shape[0], -1, -1, -1)
        seq = list(ife.backdense_1) + list(ife.backdense_2)
        with torch.no_grad(), dtoid_oracle.cpu_ops():
            x0 = ife.backdense_0(x)
            x = x0 + dtoid.ops.dw_xcorr(x0, g)
            for m in seq[:3]:
                x = m(x)
            if taps is not None:
                taps.append(x)
            for m in seq[3:]:
                x = m(x)
                if taps is not None and isinstance(m, (DenseBlock, Transition)):
                    taps.append(x)
            out = ife.n1(F.elu(ife.c1(x)))
        if taps is not None:
            taps.append(out)
        return out

    def encoder(self, which, tmpl, taps=None):
        """tmpl [n,4,h,w] -> local [n,640,7,7] / global [n,64,3,3]. taps: FusedTemplateEncoder's taps (stem after its
        ReLU, each max-pool and Fire module, each final convolution)."""
        mod = self.enc_local if which == "local" else self.enc_global
        with torch.no_grad():
            x = mod.backbone_0(tmpl.double())
            xs = []
            for part in (mod.backbone_1, mod.backbone_2):
                for m in part:
                    x = m(x)
                    if taps is not None:        # the only ReLU is the stem's: that tap is the stem's output
                        taps.append(x)
                xs.append(x)
            x1, x2 = xs
            xf = torch.cat([mod.norm_2(x2), F.interpolate(mod.norm_1(x1), size=x2.size(3), mode="bilinear",
                                                          align_corners=False)], 1)
            if hasattr(mod, "final_conv_1"):
                for conv, bn in ((mod.final_conv_1, mod.final_norm_1), (mod.final_conv_2, mod.final_norm_2)):
                    xf = bn(F.elu(conv(xf)))
                    if taps is not None:
                        taps.append(xf)
        return xf

    def head(self, feat, tmpl, img_size=None):
        """CorrelationModel (nearest up-sampling by up_index) + both detection trunks. feat [1 or n,640,h,w], tmpl
        [n,640,7,7] -> dict x2, heat, seg, cls [n,A,2], reg [n,A,4]."""
        corr = self.corr
        img_size = corr.img_size if img_size is None else img_size
        f, t = feat.double(), tmpl.double()
        if f.shape[0] == 1 and t.shape[0] > 1:
            f = f.expand(t.shape[0], -1, -1, -1)
        cab = lambda conv, bn, x: bn(F.elu(conv(x)))       # noqa: E731
        with torch.no_grad(), dtoid_oracle.cpu_ops():
            t2 = cab(corr.c2, corr.n2, cab(corr.c1, corr.n1, t))
            dot3x3 = dtoid.ops.dw_xcorr(f, t2)
            avg = F.avg_pool2d(t, 7)
            parts = [cab(corr.corr_conv_dot, corr.norm_corr_dot, f * avg), cab(corr.corr_conv_sub, corr.norm_corr_sub, f - avg),
                     cab(corr.corr_conv_dot3x3, corr.norm_corr_dot3x3, dot3x3)]
            x2 = cab(corr.cf, corr.nf, torch.cat(parts, 1))
            heat = torch.sigmoid(corr.corr_conv_heatmap(x2))
            s = x2
            for i in (1, 2, 3):
                s = cab(getattr(corr, "s%d" % i), getattr(corr, "ns%d" % i), s)
                s = nearest(s, (2 * s.shape[2], 2 * s.shape[3]))
            s = nearest(cab(corr.s4, corr.ns4, s), img_size)
            seg = corr.seg_final(cab(corr.s5, corr.ns5, s))
            cls = self.cls(x2)[0]
            reg = self.reg(x2)
        return dict(x2=x2, heat=heat, seg=seg, cls=cls, reg=reg)

    def head_sub(self, feat, tmpl):
        """norm_corr_sub(ELU(corr_conv_sub(feat - avg_t))) alone: [n,256,h,w]."""
        corr = self.corr
        f, t = feat.double(), tmpl.double()
        with torch.no_grad():
            avg = F.avg_pool2d(t, 7)
            return corr.norm_corr_sub(F.elu(corr.corr_conv_sub(f - avg)))

    def head_dot(self, feat, tmpl):
        """norm_corr_dot(ELU(corr_conv_dot(feat * avg_t))) alone: [n,256,h,w]."""
        corr = self.corr
        f, t = feat.double(), tmpl.double()
        with torch.no_grad():
            avg = F.avg_pool2d(t, 7)
            return corr.norm_corr_dot(F.elu(corr.corr_conv_dot(f * avg)))


def make_inputs(seed, B=1, n_t=21, img=IMG):
    """(images [B,3,H,W] in [0, 1], template rgb [n_t,3,124,124] in [0, 1], masks [n_t,1,124,124]). Template 0 -- the
    global template, as DtoidNet takes it -- is the calibration's (calibration_inputs)."""
    g = torch.Generator().manual_seed(seed)
    images = torch.rand(B, 3, *img, generator=g)
    rgb = torch.rand(n_t, 3, TEMPLATE, TEMPLATE, generator=g)
    mask = (torch.rand(n_t, 1, TEMPLATE, TEMPLATE, generator=g) > 0.3).float()
    _, _, (rgb0, mask0) = calibration_inputs()
    rgb[0], mask[0] = rgb0[0], mask0[0]
    return images, rgb, mask
