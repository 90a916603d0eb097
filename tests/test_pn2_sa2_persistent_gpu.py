"""GPU parity of the persistent SA2 kernel (csrc/pn2.hip: the middle layer's weights in registers, the last layer's in LDS, one
wave per SIMD, a grid of 4 waves x CU count, every wave walking a contiguous slice of the B * 128 centres, two 32-sample tiles
per centre): every feature stage and the scores bit-identical to the CPU oracle for batch sizes on each side of the
partition's edges -- fewer centres than waves, slices of unequal length, many centres per wave -- and for a small ball radius,
where centres have fewer than 32 distinct neighbours and a tile is all padding (the first hit repeated)."""
import numpy as np
import pytest
import torch

from test_oracle import _model, _oracle_features, small_inputs

pytestmark = pytest.mark.gpu

NP2 = 128        # SA2 centres per hypothesis


# 1, 2, 3, 5: at most 640 centres; 33: 4 224, not a multiple of any wave count in reach; 65: 8 320, eight and more per wave
BATCHES = [1, 2, 3, 5, 33, 65]


def test_cases_straddle_the_wave_count(hiplib):
    """The batch sizes cover each side of the partition's edges on THIS device (CU count read from it, not assumed)."""
    waves = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    totals = [b * NP2 for b in BATCHES]
    assert any(t < waves for t in totals), (waves, totals)                  # fewer centres than waves: some waves idle
    assert any(t > waves and t % waves for t in totals), (waves, totals)    # slices of unequal length
    assert any(t >= 8 * waves for t in totals), (waves, totals)             # many centres per wave


def _compare(ozr, B, M, cfg=None):
    from ossid_code_amd.zephyr.pointnet2 import fold_pn2
    d = small_inputs(N=B, M=M)
    _, _, _, px_o, _, _ = _oracle_features(ozr, d)
    m = _model(B)
    if cfg:
        m.SA_modules[0].radius, m.SA_modules[1].radius = cfg["radius1"], cfg["radius2"]
    want, wdbg = ozr.pn2_score(px_o, fold_pn2(m), cfg=cfg, debug=True)
    m = m.cuda()
    got, dbg = m.score(torch.from_numpy(px_o).cuda(), debug=True)
    for k in ("ball1", "ball2", "feat1", "feat2", "feat3"):
        g = dbg[k].cpu().numpy()
        assert g.shape == wdbg[k].shape and g.tobytes() == wdbg[k].tobytes(), k
    g = got.cpu().numpy()
    assert g.tobytes() == want.tobytes()
    return wdbg


@pytest.mark.parametrize("M", [512, 777])
@pytest.mark.parametrize("B", BATCHES)
def test_persistent_partition_bit_exact(hiplib, ozr, B, M):
    _compare(ozr, B, M)


def _distinct(ball):
    s = np.sort(ball, axis=-1)
    return 1 + (s[..., 1:] != s[..., :-1]).sum(-1)


@pytest.mark.parametrize("M", [512, 777])
def test_padded_tiles_bit_exact(hiplib, ozr, M):
    """Small radii: centres whose ball holds fewer than 32 distinct points, so the whole second tile (and part of the
    first) repeats the first hit -- in SA1 and in SA2."""
    wdbg = _compare(ozr, 5, M, cfg=dict(radius1=0.15, radius2=0.3))
    n1, n2 = _distinct(wdbg["ball1"]), _distinct(wdbg["ball2"])
    print("distinct samples per centre: sa1 min %d mean %.1f, sa2 min %d mean %.1f; centres under 32: sa1 %d of %d, sa2 %d of %d"
          % (n1.min(), n1.mean(), n2.min(), n2.mean(), (n1 < 32).sum(), n1.size, (n2 < 32).sum(), n2.size))
    assert (n2 < 32).any() and (n2 >= 32).any(), "the radius must leave SA2 centres on both sides of one tile"
    assert (n1 < 32).any()
