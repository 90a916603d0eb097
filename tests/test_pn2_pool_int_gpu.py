"""The SA1 and SA2 kernels pool max(0, max over samples) on the values' bit patterns as signed integers (csrc/pn2.hip,
pool_acc; SA3 pools the same values as floats). The corner cases, forced at every level (the last layer of SA1, SA2 and SA3)
by editing weights:
  a channel that is negative for every sample (a large negative bias): pooled value +0.0, bit pattern 0x00000000;
  a channel with weights -0.0 and bias -0.0, whose every sample is -0.0 (INT_MIN as an integer): +0.0 as well;
  a channel with a large positive bias.
Everything is compared with the CPU oracle byte for byte; the -0.0 channel in value, and as +0.0 in bits."""
import numpy as np
import pytest
import torch

from test_oracle import _model, _oracle_features, small_inputs

pytestmark = pytest.mark.gpu

NEG, NEGZERO, BIG = 5, 37, 70          # channels (one per corner case) in each level's last layer
NEG_BIAS = (-1e3, -1e6, -1e9)          # below anything the level's inputs can reach (they grow with BIG from level to level)
BIG_BIAS = 1e3


def _edit(model):
    with torch.no_grad():
        for level, sa in enumerate(model.SA_modules):
            conv, bn = sa.mlps[0][6], sa.mlps[0][7]
            for ch in (NEG, NEGZERO, BIG):                 # folded scale 1 / sqrt(1 + eps) > 0, folded bias = bn.bias
                bn.weight[ch], bn.running_var[ch], bn.running_mean[ch] = 1.0, 1.0, 0.0
            bn.bias[NEG] = NEG_BIAS[level]
            bn.bias[BIG] = BIG_BIAS
            conv.weight[NEGZERO] = -0.0
            bn.bias[NEGZERO] = -0.0
    return model


def test_pool_corner_cases_bit_exact(hiplib, ozr):
    from ossid_code_amd.zephyr.pointnet2 import fold_pn2
    B = 2
    d = small_inputs(N=B, M=512)
    _, _, _, px, _, _ = _oracle_features(ozr, d)
    model = _edit(_model(11))
    folded = fold_pn2(model)
    for li in (2, 5, 8):                                   # the edits arrive in the folded layers as intended
        W, b = folded[li]
        assert np.signbit(W[NEGZERO]).all() and not W[NEGZERO].any() and np.signbit(b[NEGZERO]) and b[NEGZERO] == 0
    want, wdbg = ozr.pn2_score(px, folded, debug=True)
    got, dbg = model.cuda().score(torch.from_numpy(px).cuda(), debug=True)
    for k in ("feat1", "feat2", "feat3"):
        w, g = wdbg[k], dbg[k].cpu().numpy()
        assert g.shape == w.shape, k
        # the cases occur: the oracle's own output has the all-negative channel at zero and the large one large
        assert not w[..., NEG].any() and not w[..., NEGZERO].any() and (w[..., BIG] > 0).all(), k
        assert not g[..., NEG].view(np.uint32).any(), k               # +0.0 in bits
        assert not g[..., NEGZERO].view(np.uint32).any(), k           # the -0.0 channel: +0.0 in bits,
        assert np.array_equal(g[..., NEGZERO], w[..., NEGZERO]), k    # equal in value to the oracle
        rest = np.ones(w.shape[-1], bool)
        rest[NEGZERO] = False
        assert g[..., rest].tobytes() == w[..., rest].tobytes(), k
    assert np.isfinite(want).all()
    assert got.cpu().numpy().tobytes() == want.tobytes()
