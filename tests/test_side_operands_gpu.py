"""GPU test (pytest -m gpu) of the property train_ops._wgrad_async exists for: every device address handed to a launch on the
weight-gradient stream lies in memory the caching allocator has been told to keep for that stream -- the storage of a tensor
record_stream()ed on it during the same _wgrad_async call -- or in scratch allocated on that stream. The launches are
watched from outside (the C-ABI calls, Tensor.record_stream, the scratch allocator), not through train_ops.dptr."""
import ctypes

import pytest
import torch

from ossid_code_amd import _lib
from ossid_code_amd.dtoid import backbones
from ossid_code_amd.dtoid import train_ops as T

pytestmark = pytest.mark.gpu


def cl(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def _struct_addresses(s):
    """Non-null values of the c_void_p fields of a descriptor struct, as its _fields_ declare them."""
    return [getattr(s, name) for name, ftype in s._fields_ if ftype is ctypes.c_void_p and getattr(s, name)]


def _addresses(name, args, stream_handle):
    """Every non-null device address a C-ABI call receives: its pointer arguments (the stream handle apart) and the pointer
    fields of descriptors passed by reference or as an array."""
    out = []
    for a, t in zip(args, _lib._PROTOS[name][1]):
        if t is not ctypes.c_void_p or a is None:
            continue
        a = getattr(a, "_obj", a)                        # ctypes.byref(d) -> d
        if isinstance(a, ctypes.Structure):
            out += _struct_addresses(a)
        elif isinstance(a, ctypes.Array):
            for s in a:
                out += _struct_addresses(s)
        elif a and a != stream_handle:
            out.append(int(a))
    return out


def unrecorded(launches, ranges):
    """(entry point, address) of every address in `launches` [(name, [address])] outside all of `ranges` [(first, bytes)]."""
    return [(name, hex(p)) for name, ps in launches for p in ps if not any(lo <= p < lo + n for lo, n in ranges)]


class Watch:
    """While installed: per _wgrad_async call, the launches issued with the weight-gradient stream current and the storages
    record_stream()ed on it; over all calls, the scratch handed out with that stream current. `missing` collects what
    `unrecorded` finds after each call."""

    def __init__(self, monkeypatch):
        self.side = T.side_streams(torch.device("cuda"))["wgrad"]
        self.launches, self.n_launches, self.recorded, self.scratch, self.missing = [], 0, [], [], []
        self.last = ([], [])                             # (launches, ranges) of the latest _wgrad_async call
        real_fn, real_scratch, real_async = _lib.fn, T._scratch, T._wgrad_async
        real_record = torch.Tensor.record_stream

        def on_side():
            return torch.cuda.current_stream() == self.side

        def fn(name):
            f = real_fn(name)

            def call(*args):
                if on_side():
                    self.launches.append((name, _addresses(name, args, self.side.cuda_stream)))
                    self.n_launches += bool(args) and args[-1] == self.side.cuda_stream   # (size queries take no stream)
                return f(*args)
            return call

        def scratch(*a):
            t = real_scratch(*a)
            if on_side():
                self.scratch.append((t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()))
            return t

        def record_stream(t, s):
            if s == self.side:
                self.recorded.append((t.untyped_storage().data_ptr(), t.untyped_storage().nbytes()))
            return real_record(t, s)

        def wgrad_async(*a, **k):
            self.launches, self.recorded = [], []
            real_async(*a, **k)
            self.missing += unrecorded(self.launches, self.recorded + self.scratch)
            self.last = (self.launches, self.recorded + self.scratch)

        monkeypatch.setattr(_lib, "fn", fn)
        monkeypatch.setattr(T, "_scratch", scratch)
        monkeypatch.setattr(torch.Tensor, "record_stream", record_stream)
        monkeypatch.setattr(T, "_wgrad_async", wgrad_async)

    def check(self):
        T.join_wgrad_stream()
        torch.cuda.synchronize()
        assert self.n_launches >= 1, "nothing was launched on the weight-gradient stream: the case ran in line"
        assert not self.missing, self.missing
        # the checker itself: an address outside every logged range is reported (host code; nothing is launched with it)
        launches, ranges = self.last
        beyond = max(lo + n for lo, n in ranges) + 4096
        assert unrecorded(launches + [("fabricated", [beyond])], ranges) == [("fabricated", hex(beyond))]


@pytest.fixture
def watch(hiplib, monkeypatch):
    monkeypatch.setattr(T, "WGRAD_SIDE", True)
    torch.manual_seed(3)
    return Watch(monkeypatch)


def test_fused_conv_weight_gradient_operands_are_recorded(watch):
    """3x3 with a (scale, shift) + ReLU prologue and nearest up-sampling 3x4 -> 10x9, B=2, 16 -> 32; a leaf weight without a
    gradient, so the launch goes to the side stream."""
    x = cl(torch.randn(2, 16, 3, 4)).requires_grad_(True)
    w = torch.nn.Parameter(torch.randn(32, 16, 3, 3, device="cuda") * 0.1)
    ps, pt = torch.rand(16, device="cuda") + 0.5, torch.randn(16, device="cuda")
    assert w.is_leaf and w.grad is None
    y = T.FusedConv.apply(x, w, None, ps, pt, True, 0, (10, 9), False)
    y.backward(cl(torch.randn(2, 32, 10, 9)))
    watch.check()


def test_one_output_channel_conv3x3_weight_gradient_operands_are_recorded(watch):
    conv = torch.nn.Conv2d(8, 1, 3, padding=1).cuda()
    x = cl(torch.randn(3, 8, 5, 7)).requires_grad_(True)
    T.conv3x3_c1(x, conv).backward(torch.randn(3, 1, 5, 7, device="cuda"))
    watch.check()


def test_stem_conv_weight_gradient_operands_are_recorded(watch):
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda()
    y = T.stem_conv(torch.rand(1, 3, 16, 40, device="cuda"), conv)
    y.backward(cl(torch.randn(y.shape)))
    watch.check()


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("L,C0,B,H,W", [(3, 64, 2, 12, 16), (4, 256, 1, 7, 9)])
def test_dense_block_grouped_weight_gradient_operands_are_recorded(watch, monkeypatch, L, C0, B, H, W, replay):
    """The grouped launch of a dense block's 2 L weight gradients, eager and in the recording pass (the first call with
    SEQ_REPLAY): with the fused backward its 1x1 items read three more tensors each (dy_add)."""
    monkeypatch.setattr(T, "SEQ_REPLAY", replay)
    blk = backbones.DenseBlock(L, C0).cuda().train()
    x = torch.randn(B, C0, H, W, device="cuda").requires_grad_(True)
    T.dense_block_train(x, blk).backward(torch.randn(B, C0 + 32 * L, H, W, device="cuda"))
    watch.check()


def test_template_encoder_weight_gradient_operands_are_recorded(watch, monkeypatch):
    """One SqueezeNet encoder node, eager, at the smallest batch of its own test: the grouped launch (the stem's `key="stem"`
    buffer among its items) and stem_relayout behind it."""
    from ossid_code_amd.dtoid import network
    from ossid_code_amd.dtoid import train_encoders as TE
    monkeypatch.setattr(T, "SEQ_REPLAY", False)
    mod = network.TemplateFeatExtract().cuda().train()
    y = TE.template_encoder_train(mod, torch.rand(3, 4, 124, 124, device="cuda"))
    y.backward(torch.randn(y.shape, device="cuda"))
    assert any(name == "ossid_stem_weight_relayout" for name, _ in watch.last[0])
    watch.check()
