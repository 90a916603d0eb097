"""train_ops.dptr / _side_operands_of: how the weight-gradient stream's record_stream set is collected (host code only: CPU
tensors, the library is never loaded)."""
import pytest
import torch

from ossid_code_amd.dtoid import train_ops as T


def test_outside_a_side_issue_dptr_is_the_address_and_notes_nothing():
    t = torch.zeros(6)
    assert T._SIDE_OPERANDS is None
    assert T.dptr(t) == t.data_ptr() and T.dptr(t[2:]) == t.data_ptr() + 8
    assert T.dptr(None) is None
    assert T._SIDE_OPERANDS is None


def test_inside_a_side_issue_every_tensor_is_noted_once_slices_included():
    a, b = torch.zeros(8), torch.zeros(3)
    part = a[4:]
    got = []

    def launch():
        got.extend([T.dptr(a), T.dptr(part), T.dptr(None), T.dptr(b), T.dptr(a)])
    noted = T._side_operands_of(launch)
    assert got == [a.data_ptr(), a.data_ptr() + 16, None, b.data_ptr(), a.data_ptr()]
    assert len(noted) == 3 and noted[0] is a and noted[1] is part and noted[2] is b      # `a` twice: one entry; None: none
    assert T._SIDE_OPERANDS is None


def test_the_collector_is_restored_when_the_launch_raises_and_the_next_region_starts_empty():
    a, b = torch.zeros(2), torch.zeros(2)

    def failing():
        T.dptr(a)
        raise RuntimeError("launch failed")
    with pytest.raises(RuntimeError, match="launch failed"):
        T._side_operands_of(failing)
    assert T._SIDE_OPERANDS is None
    T.dptr(a)                                       # outside again: noted nowhere
    noted = T._side_operands_of(lambda: T.dptr(b))
    assert len(noted) == 1 and noted[0] is b
