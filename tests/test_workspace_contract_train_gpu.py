"""The workspace contract of the detector's training and post-processing entries on the GPU (tests/guarded.py,
tests/workspace_cases.py): every consumer runs on a workspace of exactly the queried size between guard words, filled with
0xFF and with 0x7F, and must give the bytes of a run on a generous zeroed one, leave every guard intact, refuse a
workspace one byte short, and meet its own existing test's bound against that test's reference. The allocation floors of
the Python wrappers hide all of this at every shape the rest of the suite runs."""
import pytest
import torch

import workspace_cases as wc
from guarded import EINVAL, GUARD_BYTE, Contract, Guarded, ready, run_contract

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(case, shape, id="%s-%s" % (case.name, wc.sid(shape))) for case in wc.TRAIN_CASES for shape in case.shapes]


def test_the_helper_notices_what_it_is_there_for(hiplib):
    """Guarded's layout as stated, and run_contract on four stand-in entries written with torch on the test's own memory: one
    that copies its workspace into its output before writing it, one that writes one byte past its workspace, one that takes
    a workspace one byte short, and a clean one."""
    g = Guarded(1000, 0x7F)
    assert g.ptr % 256 == 0 and g.nbytes == 1000 and g.off >= 4096 and g.whole.numel() - g.off - 1000 >= 64 << 10
    assert bool((g.payload == 0x7F).all()) and bool((g.whole[:g.off] == GUARD_BYTE).all()) and g.intact()
    assert g.view(torch.float32).numel() == 250 and g.view(torch.float32).data_ptr() == g.ptr
    big = Guarded(100001, 0x00, align=16)
    assert big.ptr % 16 == 0 and big.whole.numel() - big.off - 100001 >= 100001
    for where in (g.off - 1, g.off + 1000, 0, g.whole.numel() - 1):
        g.whole[where] = 0
        assert not g.intact(), where
        g.whole[where] = GUARD_BYTE
        assert g.intact()

    def reads_first(ws, out):
        out["out"].payload.copy_(ws["ws"].payload[:64])
        return 0

    def overruns(ws, out):
        out["out"].payload.fill_(1)
        ws["ws"].whole[ws["ws"].off + ws["ws"].nbytes] = 1
        return 0

    def clean(ws, out):
        if ws["ws"].nbytes < 1000 or ws["ws"].ptr % 16:
            return EINVAL
        ws["ws"].payload.fill_(9)
        out["out"].payload[:32].copy_(ws["ws"].payload[:32])          # the rest of the output is left as it was
        return 0
    probe = lambda run, **kw: Contract("probe", {"ws": 1000}, {"out": 64}, run, **kw)      # noqa: E731
    with pytest.raises(AssertionError, match="differs from run A in 64 of 64 bytes"):
        run_contract(probe(reads_first))
    with pytest.raises(AssertionError, match="guard words around `ws`"):
        run_contract(probe(overruns))
    with pytest.raises(AssertionError, match="not OSSID_EINVAL"):
        run_contract(probe(lambda ws, out: 0, short=("ws",)))
    with pytest.raises(AssertionError, match="not OSSID_EINVAL"):
        run_contract(probe(lambda ws, out: EINVAL if ws["ws"].nbytes < 1000 else 0, short=("ws",), misalign=("ws",)))
    assert run_contract(probe(clean, short=("ws",), misalign=("ws",))) == {"ws": 1000}


@pytest.mark.parametrize("case,shape", PARAMS)
def test_workspace_contract(hiplib, case, shape):
    ready()
    for contract in case.build(hiplib, shape):
        sizes = run_contract(contract)
        print("CONTRACT %-44s %s" % (contract.name, " ".join("%s=%d%s" % (k, n, "" if n % 512 else " (x512)") for k, n in sizes.items())))
