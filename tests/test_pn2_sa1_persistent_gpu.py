"""GPU parity of the persistent SA1 kernel (csrc/pn2.hip: weights in registers, one wave per SIMD, a grid of 4 waves x CU count,
every wave walking a contiguous slice of the B * 512 centres): every feature stage and the scores bit-identical to the CPU
oracle for batch sizes on each side of the partition's edges -- fewer centres than waves, exactly one per wave, not a
multiple of the wave count, and many per wave."""
import numpy as np
import pytest
import torch

from test_oracle import _model, _oracle_features, small_inputs

pytestmark = pytest.mark.gpu

NP1 = 512        # SA1 centres per hypothesis


BATCHES = [1, 2, 3, 5, 33]


def test_cases_straddle_the_wave_count(hiplib):
    """The batch sizes cover each side of the partition's edges on THIS device (CU count read from it, not assumed)."""
    waves = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    totals = [b * NP1 for b in BATCHES]
    assert any(t <= waves for t in totals), (waves, totals)                 # at most one centre per wave, some waves idle
    assert any(t > waves and t % waves for t in totals), (waves, totals)    # slices of unequal length
    assert any(t >= 8 * waves for t in totals), (waves, totals)             # many centres per wave


@pytest.mark.parametrize("M", [512, 777])
@pytest.mark.parametrize("B", BATCHES)
def test_persistent_partition_bit_exact(hiplib, ozr, B, M):
    from ossid_code_amd.zephyr.pointnet2 import fold_pn2
    d = small_inputs(N=B, M=M)
    _, _, _, px_o, _, _ = _oracle_features(ozr, d)
    m = _model(B)
    want, wdbg = ozr.pn2_score(px_o, fold_pn2(m), debug=True)
    m = m.cuda()
    got, dbg = m.score(torch.from_numpy(px_o).cuda(), debug=True)
    for k in ("feat1", "feat2", "feat3"):
        g = dbg[k].cpu().numpy()
        assert g.shape == wdbg[k].shape and g.tobytes() == wdbg[k].tobytes(), k
    g = got.cpu().numpy()
    assert g.tobytes() == want.tobytes()
