"""Independent numpy restatement of SPEC.md section 15.1-15.3 (the detector's pre-training batch from a rendered scene
batch), the yardstick of csrc/pretrain.hip -- test infrastructure. It imports nothing from the package. Every float32
step is written out on float32 arrays, so each operation rounds once (numpy does not fuse); the hash runs on uint32
arrays, which wrap; the heat map is float64 in the order 15.2 states, its exponential the chain of fused multiply-adds
15.2 writes out (what the device's math library evaluates; a correctly rounded exponential such as numpy's differs from
it in the last bit for about one argument in twelve), each fused step computed exactly in rationals and rounded once."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
SIGMA = float(np.sqrt(1.5))
EMPTY_BOX = (float(1 << 30), float(1 << 30), -1.0, -1.0, -1.0)


def unit_image(color_hw3):
    """u8 [H,W,3] -> f32 [3,H,W] = (float)u8 / 255.0f"""
    return np.moveaxis(color_hw3.astype(F32) / F32(255.0), 2, 0)


def noise_unit(seed, H, W):
    """u of 15.3's steps 4-6 -> f32 [3,H,W]; seed is the row's last entry read as its 32 bits."""
    p = np.arange(H * W, dtype=np.uint32).reshape(1, H, W)
    c = np.arange(3, dtype=np.uint32).reshape(3, 1, 1)
    k = np.uint32(seed) + np.uint32(0x9E3779B9) * (np.uint32(3) * p + c)
    k = k ^ (k >> np.uint32(16))
    k = k * np.uint32(0x7FEB352D)
    k = k ^ (k >> np.uint32(15))
    k = k * np.uint32(0x846CA68B)
    k = k ^ (k >> np.uint32(16))
    assert k.dtype == np.uint32
    return (k >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)


def jitter_image(v, row):
    """15.3 on v f32 [3,H,W] with row f32 [8] -> (clamped f32 [3,H,W], the value before the clamp)."""
    row = np.asarray(row, dtype=F32)
    g, b, a = row[0:3].reshape(3, 1, 1), row[3:6].reshape(3, 1, 1), row[6]
    seed = row[7:8].view(np.uint32)[0]
    with np.errstate(all="ignore"):
        v = v * g
        v = v + b
        d = noise_unit(seed, v.shape[1], v.shape[2]) - F32(0.5)
        v = v + d * a
        assert v.dtype == F32
        out = np.where(v > 0, v, F32(0.0))            # NaN and -0 become +0
        out = np.where(out < 1, out, F32(1.0))
    return out.astype(F32), v


def box_of(gt_row, valid):
    x, y, w, h = (int(v) for v in gt_row[7:11])
    if not valid or x < 0 or y < 0 or w <= 0 or h <= 0:
        return EMPTY_BOX
    return (float(x), float(y), float(x + w - 1), float(y + h - 1), 1.0)


def _hex(bits):
    return float(np.array([bits], dtype=np.uint64).view(np.float64)[0])


LOG2E, LN2_HI, LN2_LO = _hex(0x3FF71547652B82FE), _hex(0xBFE62E42FEFA39EF), _hex(0xBC7ABC9E3B39803F)      # the last two negative
EXP_POLY = [_hex(b) for b in (0x3E5ADE156A5DCB37, 0x3E928AF3FCA7AB0C, 0x3EC71DEE623FDE64, 0x3EFA01997C89E6B0, 0x3F2A01A014761F6E,
                              0x3F56C16C1852B7B0, 0x3F81111111122322, 0x3FA55555555502A1, 0x3FC5555555555511, 0x3FE000000000000B)]


def _fma(a, b, c):
    """a * b + c rounded once: exact in rationals, then the nearest double (int / int division rounds correctly)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def device_exp(x):
    """15.2's exponential for finite arguments in (-1075, 0], elementwise: n = rint(x log2 e), t = x - n ln 2 by two fused
    steps on a two-part ln 2, a degree-11 polynomial in t by Horner's rule with a fused multiply-add per step, and the
    result scaled by 2^n. One rounding per written operation."""
    out = np.empty(np.shape(x), np.float64)
    flat = out.reshape(-1)
    for k, v in enumerate(np.asarray(x, dtype=np.float64).reshape(-1).tolist()):
        assert -1075.0 < v <= 0.0
        n = float(np.rint(v * LOG2E))
        t = _fma(LN2_LO, n, _fma(LN2_HI, n, v))
        p = EXP_POLY[0]
        for c in EXP_POLY[1:] + [1.0, 1.0]:
            p = _fma(t, p, c)
        flat[k] = math.ldexp(p, int(n))
    return out


def heatmap(box, hh, hw, scale, sigma=SIGMA):
    if box[4] <= 0:
        return np.zeros((hh, hw))
    cx, cy = (box[0] + box[2]) / 2.0 * scale, (box[1] + box[3]) / 2.0 * scale
    y, x = np.indices((hh, hw)).astype(np.float64)
    dx, dy = x - cx, y - cy
    d = np.sqrt(dx * dx + dy * dy)
    return device_exp(-(d * d / (2.0 * sigma * sigma)))


def scene_dtoid_batch(color, instance, gt_info, targets, hh, hw, jitter=None):
    """color u8 [S,H,W,3], instance int32 [S,H,W], gt_info int32 [I,12], targets [T,2], jitter f32 [T,8] or None ->
    img f32 [T,3,H,W], mask f32 [T,1,H,W], bbox_gt f32 [T,1,5], heatmap f64 [T,1,hh,hw], and `raw`, the jittered values
    before the clamp (None without jitter)."""
    S, H, W, _ = color.shape
    I, T = len(gt_info), len(targets)
    img = np.zeros((T, 3, H, W), F32)
    raw = None if jitter is None else np.zeros((T, 3, H, W), F32)
    mask = np.zeros((T, 1, H, W), F32)
    bbox = np.zeros((T, 1, 5), F32)
    heat = np.zeros((T, 1, hh, hw), np.float64)
    for t, (s, i) in enumerate(np.asarray(targets).tolist()):
        valid = 0 <= s < S and 0 <= i < I
        box = box_of(gt_info[i] if valid else None, valid) if valid else EMPTY_BOX
        bbox[t, 0] = np.asarray(box, dtype=np.float64).astype(F32)
        heat[t, 0] = heatmap(box, hh, hw, float(hh) / float(H))
        if not valid:
            continue
        v = unit_image(color[s])
        if jitter is not None:
            v, raw[t] = jitter_image(v, jitter[t])
        img[t] = v
        mask[t, 0] = (instance[s] == i).astype(F32)
    return {"img": img, "mask": mask, "bbox_gt": bbox, "heatmap": heat, "raw": raw}
