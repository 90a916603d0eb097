"""The workspace contract of the pose, rendering and evaluation entries on the GPU (tests/guarded.py,
tests/workspace_cases.py): the scorer and its training path, the dense PPF refinement, the rasterisers, the scene renderer,
the model cloud's face weights, detection matching and the keypoint features. Every consumer runs on a workspace of exactly
the queried size between guard words, filled with 0xFF and with 0x7F, and must give the bytes of a run on a generous zeroed
one, leave every guard intact, refuse a workspace one byte short or off its stated alignment, and equal its own
restatement or oracle as its existing test demands."""
import pytest

import workspace_cases as wc
from guarded import ready, run_contract

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(case, shape, id="%s-%s" % (case.name, wc.sid(shape))) for case in wc.POSE_CASES for shape in case.shapes]


@pytest.mark.parametrize("case,shape", PARAMS)
def test_workspace_contract(hiplib, case, shape):
    ready()
    for contract in case.build(hiplib, shape):
        sizes = run_contract(contract)
        print("CONTRACT %-44s %s" % (contract.name, " ".join("%s=%d%s" % (k, n, "" if n % 512 else " (x512)") for k, n in sizes.items())))
