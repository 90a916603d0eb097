"""The case table of the workspace contract (tests/guarded.py): one entry per size query of include/ossid_hip.h -- the
query, the entries that consume the memory it sizes, one or two small ragged shapes, and a host-side predicate saying why
each shape is one where the layout can go wrong. Defined once: tests/test_workspace_contract.py evaluates the queries, the
refusals and the predicates on the host, the two *_gpu.py files build the Contracts and run them.

Nothing here touches the GPU at import; `build` functions do (they are called by the GPU tests only)."""
import ctypes
import math

import numpy as np
import torch

import pn2_train_cases
from guarded import EINVAL, Contract

SUFFIXES = ("_workspace_bytes", "_workspace_floats", "_partials", "_grid_bytes", "_pyramid_bytes")

# Queries outside the table, each with its reason. Nothing else may be exempt: a query added later fails the coverage lock
# of tests/test_workspace_contract.py until it is in the table.
EXEMPT = {
    "ossid_ppf_sample_workspace_bytes": "behind guard words in tests/test_ppf_edges_gpu.py",
    "ossid_ppf_vote_workspace_bytes": "behind guard words in tests/test_ppf_edges_gpu.py",
    "ossid_mesh_vertex_normals_workspace_bytes": "behind guard words in tests/test_scene_light_gpu.py",
    "ossid_pn2_train_bn_stats_workspace_bytes": "a constant",
    "ossid_conv3x3_c1_wgrad_workspace_bytes": "a constant",
    "ossid_seg_bce_iou_workspace_bytes": "a one-term size (B * 64 * 3 doubles)",
    "ossid_conv3x3_wgrad_workspace_bytes": "belongs to ossid_conv3x3_wgrad, an exported entry with no Python caller",
}


class Case:
    """name; queries: the size queries this entry covers; shapes: tuples; need(lib, shape) -> {query: value as returned};
    predicate(lib, shape): asserts that the shape exercises the layout (host only); build(lib, shape) -> [Contract] (GPU);
    refusals: [(query, call)] (see R) that must return 0 (<= 0 for the int ones); ragged: False where NO valid shape gives a size
    that is not a multiple of 512 bytes, or where the size depends on the device (the reason stands at the case)."""

    def __init__(self, name, queries, shapes, need, predicate, build, refusals, nbytes=None, ragged=True):
        self.name, self.queries, self.shapes, self.need, self.predicate = name, tuple(queries), list(shapes), need, predicate
        self.build, self.refusals, self.ragged = build, list(refusals), ragged
        self.nbytes = nbytes or (lambda lib, shape: list(need(lib, shape).values()))   # buffer sizes in bytes, for the 512 rule


def R(query, *args):
    """A refusal: (query, call) -- call(lib) evaluates the query on bad arguments and must return 0 (<= 0 for an int one)."""
    return query, (lambda lib: lib.fn(query)(*args))


def sid(shape):
    return "-".join("%dof" % len(v) if isinstance(v, tuple) else str(v) for v in shape)


# ---- small helpers -------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def f32(g, *shape):
    """An output's payload as a float32 tensor of `shape` (a copy on the CPU)."""
    return g.view(torch.float32).view(*shape).cpu()


def nhwc(t):
    """[B, C, H, W] -> a contiguous [B, H, W, C] CUDA tensor."""
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def split_bf16(lib):
    return bool(lib.fn("ossid_conv_split_bf16")())


def stream(lib):
    return lib.stream()


def packed(w, kind):
    """A private copy of train_ops._pack's operand layout of the host weight `w`. _pack keeps ONE buffer per (weight address,
    shape, kind) and re-fills it: two weights of one shape whose device copies are handed the same address in turn (the first
    freed before the second is made) share it, and the later pack overwrites the earlier one's operands."""
    from ossid_code_amd.dtoid import train_ops as T
    wd = w.cuda()
    return T._pack(wd, kind).clone()


# ---- D16 ossid_conv_wgrad ------------------------------------------------------------------------------------------------------
# shape: (B, Cin, Cout, H, W, taps). The dispatch of ossid_conv_wgrad (csrc/train.hip), restated: the decoder's few-channel 3x3
# layers go to csrc/wgrad_fc.hip, 3x3 layers with input channels in 128s (<= 256) to csrc/wgrad_t9.hip (split-bf16 builds), the
# rest stays on train.hip's split-K kernels.
def wgrad_path(lib, Cin, Cout, taps):
    if taps == 9 and (Cout, Cin) in ((16, 32), (32, 64)):
        return "fewch"
    if taps == 9 and Cin <= 256 and Cin % 128 == 0 and Cout >= 32 and Cout % 4 == 0 and bool(lib.fn("ossid_conv_wgrad_split_bf16")()):
        return "t9"
    return "generic"


def wgrad_variant(Cin, Cout, taps):
    """(tiling variant, slabs per split) of train.hip's wgrad_plan."""
    if taps == 1:
        return (4, 1) if Cout <= 64 else (3, 1)
    if Cout <= 32 and Cin <= 32:
        return 5, 4
    if Cout <= 32 and Cin <= 64:
        return 6, 2
    if Cout <= 32:
        return 2, 1
    return (1, 1) if (Cout <= 64 or Cout == 96) else (0, 1)


WGRAD_SHAPES = [(2, 32, 16, 13, 37, 9),       # few-channel (the slab is 16 * 32 * 9 floats = 36 * 512 bytes: never ragged)
                (2, 128, 32, 9, 13, 9),       # t9 (the slab is 9 * 32 * 128 floats: never ragged)
                (3, 12, 20, 11, 70, 9)]       # generic, two K-splits or more; 20 * 12 * 9 floats per slab


def wgrad_need(lib, s):
    B, Cin, Cout, H, W, taps = s
    return {"ossid_conv_wgrad_workspace_bytes": int(lib.fn("ossid_conv_wgrad_workspace_bytes")(B, H, W, Cin, Cout, taps))}


def wgrad_pred(lib, s):
    B, Cin, Cout, H, W, taps = s
    want = {WGRAD_SHAPES[0]: "fewch", WGRAD_SHAPES[1]: "t9", WGRAD_SHAPES[2]: "generic"}[s]
    path = wgrad_path(lib, Cin, Cout, taps)
    if want == "t9" and not lib.fn("ossid_conv_wgrad_split_bf16")():
        want = "generic"                                       # an all-f32 build has no t9 kernel
    assert path == want, (s, path)
    need = wgrad_need(lib, s)["ossid_conv_wgrad_workspace_bytes"]
    assert need > 0
    if path == "generic":
        wk = wgrad_variant(Cin, Cout, taps)[1]
        slab = wk * taps * Cout * Cin * 4
        assert need % slab == 0 and need // slab >= 2, (s, need, slab)          # nsplit >= 2
        assert need % 512 != 0


def _wgrad_inputs(B, Cin, Cout, H, W, taps, seed):
    g = gen(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    k = 3 if taps == 9 else 1
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.double(), w, padding=k // 2).backward(dy.double())
    return nhwc(x), nhwc(dy), w.grad, k


def wgrad_build(lib, s):
    B, Cin, Cout, H, W, taps = s
    xd, dyd, want, k = _wgrad_inputs(B, Cin, Cout, H, W, taps, Cin + Cout + H)
    need = wgrad_need(lib, s)["ossid_conv_wgrad_workspace_bytes"]

    def run(ws, out):
        d = lib.WgradDesc()
        d.x, d.dy, d.dw, d.workspace, d.workspace_bytes = xd.data_ptr(), dyd.data_ptr(), out["dw"].ptr, ws["ws"].ptr, ws["ws"].nbytes
        d.batch, d.height, d.width, d.cin, d.cout, d.taps = B, H, W, Cin, Cout, taps
        return lib.fn("ossid_conv_wgrad")(ctypes.byref(d), stream(lib))

    def anchor(out):                                           # the bound of test_train_ops_gpu.py::test_wgrad_matches_torch
        assert rel(f32(out["dw"], Cout, Cin, k, k), want) < 5e-5
    return [Contract("conv_wgrad " + sid(s), {"ws": need}, {"dw": Cout * Cin * taps * 4}, run, anchor, short=("ws",))]


# ---- D16 ossid_conv_wgrad_group ------------------------------------------------------------------------------------------------
# shape: (B, H, W, ((Cin, Cout, taps) or (Cin, Cout, taps, H, W), ...)); a problem may carry a height and width of its own.
# Row 0: the 3x3 (128 -> 32) and 1x1 (c -> 128) problems of a dense block, which csrc/wgrad_t9.hip takes as two tiling variants
# of their own, and two problems that stay on train.hip's kernels (two more variants): the group's one workspace is carved
# four ways. Row 1: two geometries and both t9 classes (cout 32 / cout >= 64) in one group: csrc/wgrad_t9.hip takes one
# geometry and one class per call, so the group goes there in rounds -- {0, 7}, {1}, {2} to t9, {3}, {4} to t1 -- and the two
# problems left over ({5, 6}) share train.hip's grouped launches.
GROUP_SHAPES = [(1, 7, 9, ((128, 32, 9), (64, 128, 1), (128, 32, 9), (96, 128, 1), (16, 16, 9), (24, 40, 9))),
                (1, 7, 9, ((128, 32, 9), (128, 64, 9), (128, 32, 9, 5, 6), (64, 128, 1), (96, 128, 1, 5, 6), (24, 40, 9, 5, 6),
                           (16, 16, 9), (128, 32, 9)))]
MIXED_PARTS = ((0, 7), (1,), (2,), (3,), (4,), (5, 6))         # row 1 as the calls its rounds amount to (split-bf16 builds)


def group_probs(s):
    """The problems of a row as (Cin, Cout, taps, B, H, W)."""
    B, H, W, probs = s
    return [(p[0], p[1], p[2], B) + (tuple(p[3:5]) if len(p) > 3 else (H, W)) for p in probs]


def group_sub(s, idx):
    """The row holding the problems `idx` of row `s`, in that order."""
    return s[:3] + (tuple(s[3][i] for i in idx),)


def _group_descs(lib, s, ptrs=None):
    probs = group_probs(s)
    arr = (lib.WgradDesc * len(probs))()
    for i, (d, (cin, cout, taps, B, H, W)) in enumerate(zip(arr, probs)):
        d.batch, d.height, d.width, d.cin, d.cout, d.taps = B, H, W, cin, cout, taps
        if ptrs is not None:
            d.x, d.dy, d.dw = ptrs[i]
    return arr


def group_need(lib, s):
    arr = _group_descs(lib, s) if len(s[3]) else None
    return {"ossid_conv_wgrad_group_workspace_bytes": int(lib.fn("ossid_conv_wgrad_group_workspace_bytes")(arr, len(s[3])))}


def group_pred(lib, s):
    probs = group_probs(s)
    sb = bool(lib.fn("ossid_conv_wgrad_split_bf16")())
    kinds = set()
    for cin, cout, taps, _, _, _ in probs:
        if sb and taps == 9 and cin % 128 == 0 and cout >= 32:
            kinds.add("t9")
        elif sb and taps == 1 and cout == 128 and cin % 32 == 0:
            kinds.add("t1")
        else:
            kinds.add(wgrad_variant(cin, cout, taps)[0])
    assert len(probs) >= 3 and len(kinds) >= 2, kinds
    whole = group_need(lib, s)["ossid_conv_wgrad_group_workspace_bytes"]
    assert whole > 0
    if s == GROUP_SHAPES[1] and sb:
        # the group's size is the sum of its parts queried separately, whatever the order of the problems
        parts = [group_need(lib, group_sub(s, idx))["ossid_conv_wgrad_group_workspace_bytes"] for idx in MIXED_PARTS]
        assert all(p > 0 for p in parts) and whole == sum(parts), (whole, parts)
        turned = group_need(lib, group_sub(s, (6, 4, 7, 2, 5, 1, 3, 0)))["ossid_conv_wgrad_group_workspace_bytes"]
        assert turned == whole, (turned, whole)


def group_build(lib, s):
    probs = group_probs(s)
    ins = [_wgrad_inputs(B, cin, cout, H, W, taps, 11 * i + cin) for i, (cin, cout, taps, B, H, W) in enumerate(probs)]
    need = group_need(lib, s)["ossid_conv_wgrad_group_workspace_bytes"]

    def run(ws, out):
        arr = _group_descs(lib, s, [(x.data_ptr(), dy.data_ptr(), out["dw%d" % i].ptr) for i, (x, dy, _, _) in enumerate(ins)])
        return lib.fn("ossid_conv_wgrad_group")(arr, len(probs), ws["ws"].ptr, ws["ws"].nbytes, stream(lib))

    def anchor(out):          # the bound of test_train_ops_gpu.py::test_grouped_weight_gradients_of_a_dense_block_match_torch
        for i, ((cin, cout, taps, _, _, _), (_, _, want, k)) in enumerate(zip(probs, ins)):
            assert rel(f32(out["dw%d" % i], cout, cin, k, k), want) < 5e-5, (i, cin, cout)
    outs = {"dw%d" % i: cout * cin * taps * 4 for i, (cin, cout, taps, _, _, _) in enumerate(probs)}
    # every share of the workspace is rounded to 256 bytes and the tiled kernels' slabs are multiples of 512
    return [Contract("conv_wgrad_group " + sid(s), {"ws": need}, outs, run, anchor, short=("ws",))]


# ---- D4 ossid_stem_conv_wgrad --------------------------------------------------------------------------------------------------
STEM_SHAPES = [(3, 53, 77)]


def stem_need(lib, s):
    return {"ossid_stem_conv_wgrad_workspace_bytes": int(lib.fn("ossid_stem_conv_wgrad_workspace_bytes")(*s))}


def stem_pred(lib, s):
    B, H, W = s
    assert B == 3 and H % 2 == 1 and W % 2 == 1
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert Ho % 4 and Wo % 32                                  # ragged against the 4 x 32 output tiles
    assert stem_need(lib, s)["ossid_stem_conv_wgrad_workspace_bytes"] > 0


def stem_build(lib, s):
    B, H, W = s
    g = gen(B * 1000 + H + W)
    img = torch.rand(B, 3, H, W, generator=g)
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(img.double(), w, stride=2, padding=3)
    go = torch.randn(y.shape, generator=g)
    y.backward(go.double())
    imgd, god = img.cuda(), nhwc(go)
    need = stem_need(lib, s)["ossid_stem_conv_wgrad_workspace_bytes"]

    def run(ws, out):
        return lib.fn("ossid_stem_conv_wgrad")(imgd.data_ptr(), god.data_ptr(), B, 3, H, W, 64, 7, 2, 3, None, None, ws["ws"].ptr,
                                               ws["ws"].nbytes, out["dw"].ptr, 0, stream(lib))

    def anchor(out):  # the bound of test_train_ops_gpu.py::test_stem_conv7x7s2_implicit_im2col_forward_and_weight_gradient
        assert rel(f32(out["dw"], 64, 3, 7, 7), w.grad) < 2e-5
    return [Contract("stem_conv_wgrad " + sid(s), {"ws": need}, {"dw": 64 * 147 * 4}, run, anchor, short=("ws",), misalign=("ws",))]


# ---- D16 ossid_dw_bwd_k_nhwc ---------------------------------------------------------------------------------------------------
# shape (B, H, W, C): chunks of 4 image rows x (256 / (C / 4)) * 4 columns
DWK_SHAPES = [(1, 9, 129, 64)]


def dwk_need(lib, s):
    return {"ossid_dw_bwd_k_workspace_floats": int(lib.fn("ossid_dw_bwd_k_workspace_floats")(*s))}


def dwk_pred(lib, s):
    B, H, W, C = s
    cols = (256 // (C // 4)) * 4
    assert math.ceil(H / 4) >= 3 and W % cols != 0 and W > cols
    n = dwk_need(lib, s)["ossid_dw_bwd_k_workspace_floats"]
    assert n == math.ceil(H / 4) * math.ceil(W / cols) * B * C * 9 and (4 * n) % 512 != 0


def _dw_ref(x, k):
    """x + per-sample depthwise 3x3 cross-correlation, float64: x [B,C,H,W], k [B,C,3,3]."""
    B, C, H, W = x.shape
    y = torch.nn.functional.conv2d(x.reshape(1, B * C, H, W), k.reshape(B * C, 1, 3, 3), padding=1, groups=B * C)
    return x + y.view(B, C, H, W)


def dwk_build(lib, s):
    B, H, W, C = s
    g = gen(H + W + C)
    x, go = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    k = torch.zeros(B, C, 3, 3, dtype=torch.float64, requires_grad=True)
    _dw_ref(x.double(), k).backward(go.double())
    xd, gd = nhwc(x), nhwc(go)
    need = 4 * dwk_need(lib, s)["ossid_dw_bwd_k_workspace_floats"]

    def run(ws, out):
        return lib.fn("ossid_dw_bwd_k_nhwc")(xd.data_ptr(), gd.data_ptr(), B, H, W, C, ws["ws"].ptr, out["dk"].ptr, stream(lib))

    def anchor(out):          # the kernel gradient's bound of test_train_ops_gpu.py::test_stem_training_pieces_match_torch_autograd
        assert rel(f32(out["dk"], B, C, 3, 3), k.grad) < 1e-4
    return [Contract("dw_bwd_k " + sid(s), {"ws": need}, {"dk": B * C * 9 * 4}, run, anchor)]


# ---- D6 ossid_conv1x1_c1_bwd ---------------------------------------------------------------------------------------------------
# shape (rows, C): 64 rows per partial row up to 65 536 rows, 256 above
C1_SHAPES = [(199, 8), (65800, 4)]


def c1_need(lib, s):
    return {"ossid_conv1x1_c1_bwd_workspace_floats": int(lib.fn("ossid_conv1x1_c1_bwd_workspace_floats")(*s))}


def c1_pred(lib, s):
    rows, C = s
    rpb = 256 if rows > 65536 else 64
    n = c1_need(lib, s)["ossid_conv1x1_c1_bwd_workspace_floats"]
    assert rows % 256 != 0 and rows % rpb != 0 and math.ceil(rows / rpb) >= 3 and n == math.ceil(rows / rpb) * (C + 1)
    assert (4 * n) % 512 != 0


def c1_build(lib, s):
    rows, C = s
    g = gen(rows + C)
    x, go, w = torch.randn(rows, C, generator=g), torch.randn(rows, generator=g), torch.randn(C, generator=g)
    xd, gd, wd = x.cuda(), go.cuda(), w.cuda()
    need = 4 * c1_need(lib, s)["ossid_conv1x1_c1_bwd_workspace_floats"]

    def run(ws, out):
        return lib.fn("ossid_conv1x1_c1_bwd")(xd.data_ptr(), gd.data_ptr(), rows, C, wd.data_ptr(), ws["ws"].ptr, out["dx"].ptr,
                                              out["dw_db"].ptr, stream(lib))

    def anchor(out):      # the bound of test_head_train_gpu.py::test_one_output_channel_convs_at_the_head_shapes_against_float64
        assert rel(f32(out["dx"], rows, C), go.double()[:, None] * w.double()[None]) < 7e-7
        assert rel(f32(out["dw_db"], C + 1), torch.cat([(go.double()[:, None] * x.double()).sum(0), go.double().sum()[None]])) < 7e-7
    return [Contract("conv1x1_c1_bwd " + sid(s), {"ws": need}, {"dx": rows * C * 4, "dw_db": (C + 1) * 4}, run, anchor)]


# ---- D15 ossid_focal_smoothl1_loss_fwd / _bwd ----------------------------------------------------------------------------------
LOSS_SHAPES = [(3, 300)]


def loss_need(lib, s):
    return {"ossid_focal_smoothl1_loss_workspace_floats": int(lib.fn("ossid_focal_smoothl1_loss_workspace_floats")(*s))}


def loss_pred(lib, s):
    B, A = s
    n = loss_need(lib, s)["ossid_focal_smoothl1_loss_workspace_floats"]
    assert B == 3 and A % 256 != 0 and A > 256 and n == B * math.ceil(A / 256) * 3 and (4 * n) % 512 != 0


def loss_build(lib, s):
    from ossid_code_amd import dtoid
    B, A = s
    C, G = 2, 2
    g = gen(A)
    ctr = torch.rand(A, 2, generator=g) * torch.tensor([600.0, 440.0]) + 20
    wh = torch.rand(A, 2, generator=g) * 80 + 40
    anchors = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    cls = torch.rand(B, A, C, generator=g)
    reg = torch.randn(B, A, 4, generator=g) * 0.3
    ann = torch.full((B, G, 5), -1.0)
    for b in range(B - 1):                                     # the last image has no box
        for j in range(1 + b):
            ann[b, j, :4] = anchors[17 * b + 5 * j + 3] + torch.tensor([3.0, -2.0, 4.0, 1.0])
            ann[b, j, 4] = float(j % 2)
    cd, rd, ad, nd = cls.cuda(), reg.cuda(), anchors.cuda(), ann.cuda()
    up = torch.tensor([1.7, 0.6]).cuda()
    need = 4 * loss_need(lib, s)["ossid_focal_smoothl1_loss_workspace_floats"]
    outs = {"dcls_raw": B * A * C * 4, "dreg_raw": B * A * 16, "losses2": 8, "scales2B": 8 * B, "dcls": B * A * C * 4, "dreg": B * A * 16}

    def run(ws, out):
        rc = lib.fn("ossid_focal_smoothl1_loss_fwd")(cd.data_ptr(), rd.data_ptr(), ad.data_ptr(), nd.data_ptr(), B, A, C, G, 0.25, 2.0,
                                                     out["dcls_raw"].ptr, out["dreg_raw"].ptr, ws["ws"].ptr, out["losses2"].ptr,
                                                     out["scales2B"].ptr, stream(lib))
        if rc:
            return rc
        return lib.fn("ossid_focal_smoothl1_loss_bwd")(out["dcls_raw"].ptr, out["dreg_raw"].ptr, out["scales2B"].ptr, up.data_ptr(), B,
                                                       A, C, out["dcls"].ptr, out["dreg"].ptr, stream(lib))

    def anchor(out):      # reference and bound of test_dtoid_gpu.py::test_fused_detection_loss_matches_tensor_expressions
        c, r = cd.clone().requires_grad_(True), rd.clone().requires_grad_(True)
        lossf = dtoid.DetectionLoss()
        lossf.use_fused = False
        lc, lr = lossf(c, r, ad[None], nd)
        (1.7 * lc + 0.6 * lr).sum().backward()
        got = (f32(out["losses2"], 2)[0:1], f32(out["losses2"], 2)[1:2], f32(out["dcls"], B, A, C), f32(out["dreg"], B, A, 4))
        for a, b, name in zip(got, (lc.detach().cpu(), lr.detach().cpu(), c.grad.cpu(), r.grad.cpu()), ("loss_cls", "loss_reg", "dcls", "dreg")):
            scale = float(b.abs().max().clamp(min=1e-12))
            assert float((a - b.reshape(a.shape)).abs().max()) <= 2e-5 * scale + 1e-9, name
        assert float(c.grad.abs().max()) > 0 and float(r.grad.abs().max()) > 0
    return [Contract("focal_smoothl1_loss " + sid(s), {"ws": need}, outs, run, anchor)]


# ---- D6-D8 ossid_conv3x3_wino_fwd / _fwd_pair ----------------------------------------------------------------------------------
# shape (B, Cin, Cout, H, W). The scratch is optional by the header (without it the launch runs whole workgroups and rounds
# differently), so one byte short is no refusal here: the three runs all pass at least the queried size. A slice's raw sums
# are a power-of-two count of floats: no valid shape gives a size that is not a multiple of 512 bytes.
WINO_SHAPES = [(3, 128, 32, 5, 7)]


def _wino_desc(lib, s, ptrs=(1, 1, 1, 1)):
    B, Cin, Cout, H, W = s
    d = lib.ConvDesc()
    d.x, d.wpk, d.bias, d.out = ptrs
    d.in_batch_stride, d.batch, d.height, d.width, d.cin, d.cout, d.taps, d.act = -1, B, H, W, Cin, Cout, 9, 1
    return d


def wino_need(lib, s):
    d0, d1 = _wino_desc(lib, s), _wino_desc(lib, s)
    return {"ossid_conv3x3_wino_workspace_bytes": int(lib.fn("ossid_conv3x3_wino_workspace_bytes")(ctypes.byref(d0))),
            "ossid_conv3x3_wino_pair_workspace_bytes": int(lib.fn("ossid_conv3x3_wino_pair_workspace_bytes")(ctypes.byref(d0), ctypes.byref(d1)))}


def wino_pred(lib, s):
    B, Cin, Cout, H, W = s
    th, tw = (H + 1) // 2, (W + 1) // 2
    assert th % 2 == 1 and (B * th * tw) % 32 != 0 and Cin >= 128          # odd tile counts; a reduction long enough to cut
    n = wino_need(lib, s)
    assert n["ossid_conv3x3_wino_workspace_bytes"] > 0 and n["ossid_conv3x3_wino_pair_workspace_bytes"] > 0    # the tail split is taken


def wino_build(lib, s):
    B, Cin, Cout, H, W = s
    g = gen(B * 1000 + Cin + H)
    layers = []
    for _ in range(2):
        x = torch.randn(B, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
        bias = torch.randn(Cout, generator=g)
        ref = torch.nn.functional.elu(torch.nn.functional.conv2d(x.double(), w.double(), bias.double(), padding=1))
        layers.append((nhwc(x), packed(w, "wino_fwd"), bias.cuda(), ref.permute(0, 2, 3, 1)))
    need = wino_need(lib, s)
    nout = B * H * W * Cout * 4

    def desc(i, out, ws=None):
        x, wpk, bias, _ = layers[i]
        d = _wino_desc(lib, s, (x.data_ptr(), wpk.data_ptr(), bias.data_ptr(), out.ptr))
        if ws is not None:
            d.scratch, d.scratch_bytes = ws.ptr, ws.nbytes
        return d

    def run1(ws, out):
        return lib.fn("ossid_conv3x3_wino_fwd")(ctypes.byref(desc(0, out["out"], ws["ws"])), stream(lib))

    def run2(ws, out):
        return lib.fn("ossid_conv3x3_wino_fwd_pair")(ctypes.byref(desc(0, out["out0"], ws["ws"])), ctypes.byref(desc(1, out["out1"])),
                                                     stream(lib))

    def anchor1(out):                                          # the bound of test_wino_gpu.py::test_wino_forward_matches_conv2d
        assert rel(f32(out["out"], B, H, W, Cout), layers[0][3]) < 2e-5

    def anchor2(out):                                          # the bound of test_wino_gpu.py::test_wino_pair_launch_at_128_channel_workgroups
        assert rel(f32(out["out0"], B, H, W, Cout), layers[0][3]) < 2e-5 and rel(f32(out["out1"], B, H, W, Cout), layers[1][3]) < 2e-5
    return [Contract("wino_fwd " + sid(s), {"ws": need["ossid_conv3x3_wino_workspace_bytes"]}, {"out": nout}, run1, anchor1),
            Contract("wino_fwd_pair " + sid(s), {"ws": need["ossid_conv3x3_wino_pair_workspace_bytes"]}, {"out0": nout, "out1": nout},
                     run2, anchor2)]


# ---- D12 ossid_topk / ossid_nms / ossid_detect_post ----------------------------------------------------------------------------
# shape (n, k, A): n in {1, 65, 1025}, k in {1, n}
POST_SHAPES = [(1, 1, 1), (65, 1, 13), (65, 65, 13), (1025, 1, 41), (1025, 1025, 41)]


def post_need(lib, s):
    n, k, A = s
    return {"ossid_topk_workspace_bytes": int(lib.fn("ossid_topk_workspace_bytes")(n, k)),
            "ossid_nms_workspace_bytes": int(lib.fn("ossid_nms_workspace_bytes")(n)),
            "ossid_detect_post_workspace_bytes": int(lib.fn("ossid_detect_post_workspace_bytes")(n, k))}


def post_pred(lib, s):
    n, k, A = s
    assert n in (1, 65, 1025) and k in (1, n) and n % A == 0
    need = post_need(lib, s)
    words = (n + 63) // 64
    assert need["ossid_nms_workspace_bytes"] == n * words * 8 + 256
    assert need["ossid_detect_post_workspace_bytes"] == -(-need["ossid_topk_workspace_bytes"] // 256) * 256 + (k * ((k + 63) // 64) * 8 + 256)
    assert need["ossid_topk_workspace_bytes"] % 512 != 0 or k != 1


def post_build(lib, s):
    from ossid_code_amd.dtoid import ops
    n, k, A = s
    g = gen(n + k)
    scores = torch.rand(n, generator=g)
    if n > 10:
        scores[7] = scores[3]                                  # tied scores: the index decides
    ctr = torch.rand(n, 2, generator=g) * 200
    wh = torch.rand(n, 2, generator=g) * 60 + 2
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)         # as test_nms_matches_greedy_oracle draws them
    if n > 10:
        boxes[5] = boxes[2]
    anchors = boxes[:A].contiguous()
    deltas = torch.randn(n, 4, generator=g) * 0.3
    sd, bd, ad, dd = scores.cuda(), boxes.cuda(), anchors.cuda(), deltas.cuda()
    cls2 = torch.stack([1 - sd, sd], 1).contiguous()           # the object column, stride 2
    need = post_need(lib, s)

    def run_topk(ws, out):
        return lib.fn("ossid_topk")(sd.data_ptr(), n, k, ws["ws"].ptr, ws["ws"].nbytes, out["values"].ptr, out["indices"].ptr, stream(lib))

    def anchor_topk(out):                                      # the checks of test_dtoid_gpu.py::test_topk_radix_select_matches_torch
        rv, _ = torch.topk(scores, k)
        assert torch.equal(out["values"].view(torch.float32).cpu(), rv)
        assert torch.equal(out["indices"].view(torch.int64).cpu(), torch.sort(-scores, stable=True).indices[:k])

    def run_nms(ws, out):
        return lib.fn("ossid_nms")(bd.data_ptr(), n, 0.5, ws["ws"].ptr, ws["ws"].nbytes, out["keep"].ptr, out["num_keep"].ptr, stream(lib))

    def anchor_nms(out):                                       # the oracle of test_dtoid_gpu.py::test_nms_matches_greedy_oracle
        from oracle import dtoid_oracle
        want = dtoid_oracle.nms(boxes, torch.arange(n, 0, -1).float(), 0.5)        # (the boxes are taken as already sorted)
        cnt = int(out["num_keep"].view(torch.int32).item())
        assert out["keep"].view(torch.int32)[:cnt].cpu().tolist() == want.tolist()

    def run_post(ws, out):
        return lib.fn("ossid_detect_post")(cls2.data_ptr() + 4, n, 2, k, ad.data_ptr(), dd.data_ptr(), A, 640.0, 480.0, 0.5, ws["ws"].ptr,
                                           ws["ws"].nbytes, out["scores"].ptr, out["indices"].ptr, out["boxes"].ptr, out["keep"].ptr,
                                           out["num_keep"].ptr, stream(lib))

    def anchor_post(out):     # the step-by-step path of test_dtoid_gpu.py::test_fused_post_processing_equals_the_step_by_step_one
        vals, idx = ops.topk_scores(sd, k)
        allb = ops.decode_clip_boxes(ad[None], dd.view(n // A, A, 4), 640.0, 480.0).reshape(n, 4)
        cand = allb[idx].contiguous()
        kept = ops.nms(cand, vals, 0.5, sorted_desc=True)
        assert torch.equal(out["scores"].view(torch.float32), vals) and torch.equal(out["indices"].view(torch.int64), idx)
        assert torch.equal(out["boxes"].view(torch.float32).view(k, 4), cand)
        cnt = int(out["num_keep"].view(torch.int32).item())
        assert out["keep"].view(torch.int32)[:cnt].tolist() == kept.tolist()
    cs = [Contract("topk " + sid(s), {"ws": need["ossid_topk_workspace_bytes"]}, {"values": 4 * k, "indices": 8 * k}, run_topk,
                   anchor_topk, short=("ws",)),
          Contract("detect_post " + sid(s), {"ws": need["ossid_detect_post_workspace_bytes"]},
                   {"scores": 4 * k, "indices": 8 * k, "boxes": 16 * k, "keep": 4 * k, "num_keep": 4}, run_post, anchor_post, short=("ws",))]
    if k == n:                                                 # (ossid_nms takes n alone: once per n)
        cs.append(Contract("nms " + sid(s), {"ws": need["ossid_nms_workspace_bytes"]}, {"keep": 4 * n, "num_keep": 4}, run_nms,
                           anchor_nms, short=("ws",)))
    return cs


# ---- D16 ossid_chan_op ---------------------------------------------------------------------------------------------------------
# shape (n_rows, C): partials [P][2][C] floats as the header states
CHAN_SHAPES = [(301, 8), (77, 96)]


def chan_need(lib, s):
    return {"ossid_chan_op_partials": int(lib.fn("ossid_chan_op_partials")(*s))}


def chan_nbytes(lib, s):
    return [chan_need(lib, s)["ossid_chan_op_partials"] * 2 * s[1] * 4]


def chan_pred(lib, s):
    n, C = s
    P = chan_need(lib, s)["ossid_chan_op_partials"]
    assert P >= 3 and n % math.ceil(n / P) != 0 and C in (8, 96) and (P * 2 * C * 4) % 512 != 0


def chan_build(lib, s):
    n, C = s
    g = gen(n + C)
    G = torch.randn(n, C, generator=g) + 3.0
    X = torch.randn(n, C, generator=g)
    Gd, Xd = G.cuda(), X.cuda()
    P = chan_need(lib, s)["ossid_chan_op_partials"]
    cs = []
    for sum_mode in (1, 3):
        for defer in (0, 1):
            def run(ws, out, sum_mode=sum_mode, defer=defer):
                d = lib.ChanOpDesc()
                d.g, d.x, d.out = Gd.data_ptr(), Xd.data_ptr(), out["out"].ptr
                d.n_rows, d.channels, d.sum_mode, d.partials = n, C, sum_mode, ws["partials"].ptr
                d.pivot = Gd.data_ptr() if sum_mode == 3 else None
                d.defer_finalize, d.sums = defer, (None if defer else out["sums"].ptr)
                rc = lib.fn("ossid_chan_op")(ctypes.byref(d), stream(lib))
                if rc or not defer:
                    return rc
                return lib.fn("ossid_colsum_finalize")(ws["partials"].ptr, P, C, out["sums"].ptr, 0, stream(lib))

            def anchor(out, sum_mode=sum_mode, defer=defer):       # the bounds of test_train_ops_gpu.py::test_chan_op_all_modes
                rows = 3 if (sum_mode == 3 and not defer) else 2
                sums = f32(out["sums"], rows, C)
                assert rel(f32(out["out"], n, C), G) < 1e-5
                gs, xs = G.double(), X.double()
                if sum_mode == 1:
                    assert rel(sums[0], gs.sum(0)) < 2e-5 and rel(sums[1], (gs * xs).sum(0)) < 2e-5
                else:
                    dd = gs - gs[0]
                    assert rel(sums[0], dd.sum(0)) < 3e-7 and rel(sums[1], (dd * dd).sum(0)) < 3e-7
                    if not defer:
                        assert torch.equal(sums[2], G[0])
            rows = 3 if (sum_mode == 3 and not defer) else 2
            cs.append(Contract("chan_op %s sum_mode %d%s" % (sid(s), sum_mode, " deferred" if defer else ""), {"partials": P * 2 * C * 4},
                               {"out": n * C * 4, "sums": rows * C * 4}, run, anchor))
    return cs


# ---- D16 the fused dense-block kernels (csrc/dense_bwd.hip) ----------------------------------------------------------------------
# shape (B, H, W, c, Ct): "B3-5x9" of tests/test_dense_train_gpu.py, which pins these very shapes against float64; the inputs
# are drawn as there (away from the ReLU kink). In a -DOSSID_CONV_F32 build the three entries return OSSID_EINVAL, as the
# header documents, and the contract asserts that.
DENSE_SHAPES = [(3, 5, 9, 224, 256)]
MID = 128


def _away(n, c, g, lo=0.02):
    s = (0.5 + torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    t = 0.5 * torch.randn(c, generator=g)
    z = (lo + torch.randn(n, c, generator=g).abs()) * torch.where(torch.rand(n, c, generator=g) < 0.5, -1.0, 1.0)
    return (z - t) / s, s, t


def fwd1_need(lib, s):
    return {"ossid_dense_fwd1_stats_partials": int(lib.fn("ossid_dense_fwd1_stats_partials")(s[0] * s[1] * s[2]))}


def fwd1_nbytes(lib, s):
    P = fwd1_need(lib, s)["ossid_dense_fwd1_stats_partials"]
    return [P * 4]      # counts [P] floats; the rows [P][3][128] floats are P * 1536 bytes, a multiple of 512 whatever P


def fwd1_pred(lib, s):
    N = s[0] * s[1] * s[2]
    P = fwd1_need(lib, s)["ossid_dense_fwd1_stats_partials"]
    assert 3 <= P <= math.ceil(N / 32) and N % 32 != 0 and (P * 4) % 512 != 0


def fwd1_build(lib, s):
    B, H, W, c, Ct = s
    N = B * H * W
    g = gen(N + 7 * c + Ct)
    x, ps, pt = _away(N, c, g)
    w1 = torch.randn(MID, c, 1, 1, generator=g) / c ** 0.5
    xfull = torch.full((N, Ct), float("nan"))
    xfull[:, :c] = x
    xd, psd, ptd = xfull.cuda(), ps.cuda(), pt.cuda()
    sb = split_bf16(lib)
    wpk = packed(w1, "fwd_x6") if sb else xd
    P = fwd1_need(lib, s)["ossid_dense_fwd1_stats_partials"]

    def run(ws, out):      # partial rows [P][3][128] and counts [P]: two buffers, sized from the header's words
        return lib.fn("ossid_dense_fwd1_stats")(xd.data_ptr(), Ct, c, psd.data_ptr(), ptd.data_ptr(), wpk.data_ptr(), N, out["y1"].ptr,
                                                ws["partials"].ptr, ws["counts"].ptr, stream(lib))

    def anchor(out):       # the bound of test_dense_train_gpu.py::test_dense_fwd1_stats_and_fold_against_float64 on y1
        y64 = torch.relu(x.double() * ps.double() + pt.double()) @ w1.view(MID, c).double().t()
        assert rel(f32(out["y1"], N, MID), y64) < 5e-6
    return [Contract("dense_fwd1_stats " + sid(s), {"partials": P * 3 * MID * 4, "counts": P * 4}, {"y1": N * MID * 4}, run, anchor,
                     expect=0 if sb else EINVAL)]


# the rows of ossid_dense_fwd1_stats are results (ossid_bn_fold_fwd_rows reads them): the contract above runs the fold on them
# as well, so that a row or count the kernel leaves unwritten shows in the fold's outputs
def fwd1_build_with_fold(lib, s):
    (c0,) = fwd1_build(lib, s)
    B, H, W, c, Ct = s
    N = B * H * W
    P = fwd1_need(lib, s)["ossid_dense_fwd1_stats_partials"]
    g = gen(c + 1)
    gamma, beta = (1 + 0.2 * torch.randn(MID, generator=g)).cuda(), (0.2 * torch.randn(MID, generator=g)).cuda()
    inner = c0.run

    def run(ws, out):
        rc = inner(ws, out)
        if rc:
            return rc
        f = out["fold"].ptr
        return lib.fn("ossid_bn_fold_fwd_rows")(ws["partials"].ptr, ws["counts"].ptr, P, MID, float(N), gamma.data_ptr(), beta.data_ptr(),
                                                1e-5, 0.1, None, None, f, f + MID * 4, f + 2 * MID * 4, f + 3 * MID * 4, stream(lib))
    inner_anchor = c0.anchor

    def anchor(out):       # ... and its 1e-6 on the fold against float64 statistics of the kernel's own y1
        inner_anchor(out)
        y = f32(out["y1"], N, MID).double()
        mean, var = y.mean(0), y.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        scale = gamma.cpu().double() * rstd
        own = torch.stack([scale, beta.cpu().double() - mean * scale, mean, rstd])
        got = f32(out["fold"], 4, MID)
        for i in range(4):
            assert rel(got[i], own[i]) < 1e-6, i
    c0.run, c0.anchor = run, anchor
    c0.outputs["fold"] = 4 * MID * 4
    return [c0]


def dgrad1_need(lib, s):
    return {"ossid_dense_dgrad1_acc_partials": int(lib.fn("ossid_dense_dgrad1_acc_partials")(s[0] * s[1] * s[2]))}


def dgrad1_nbytes(lib, s):
    return [dgrad1_need(lib, s)["ossid_dense_dgrad1_acc_partials"] * 2 * s[3] * 4]


def dgrad1_pred(lib, s):
    N = s[0] * s[1] * s[2]
    P = dgrad1_need(lib, s)["ossid_dense_dgrad1_acc_partials"]
    assert P >= 3 and N % 64 != 0 and (P * 2 * s[3] * 4) % 512 != 0


def _colsum(lib, ws_ptr, P, C, out, name):
    return lib.fn("ossid_colsum_finalize")(ws_ptr, P, C, out[name].ptr, 0, stream(lib))


def dgrad1_build(lib, s):
    B, H, W, c, Ct = s
    N = B * H * W
    g = gen(N + 3 * c + Ct)
    x, ms, mt = _away(N, c, g)
    xfull = torch.full((N, Ct), float("nan"))
    xfull[:, :c] = x
    G0 = torch.randn(N, Ct, generator=g)
    dz = torch.randn(N, MID, generator=g)
    w1 = torch.randn(MID, c, 1, 1, generator=g) / MID ** 0.5
    alpha = torch.randn(c, generator=g)
    xd, dzd, al, msd, mtd, G0d = xfull.cuda(), dz.cuda(), alpha.cuda(), ms.cuda(), mt.cuda(), G0.cuda()
    sb = split_bf16(lib)
    wpk = packed(w1, "dgrad") if sb else xd
    P = dgrad1_need(lib, s)["ossid_dense_dgrad1_acc_partials"]

    def run(ws, out):      # partial rows [P][2][c], then their fixed-order sum (what ossid_bn_fold_bwd starts from)
        rc = lib.fn("ossid_dense_dgrad1_acc")(dzd.data_ptr(), wpk.data_ptr(), xd.data_ptr(), out["G"].ptr, N, c, Ct, al.data_ptr(),
                                              msd.data_ptr(), mtd.data_ptr(), ws["partials"].ptr, None, None, None, stream(lib))
        return rc or _colsum(lib, ws["partials"].ptr, P, c, out, "sums")

    def anchor(out):       # the bounds of test_dense_train_gpu.py::test_dense_dgrad1_acc_and_fold_against_float64
        Gn = f32(out["G"], N, Ct)
        prod = dz.double() @ w1.view(MID, c).double()
        m = (x.double() * ms.double() + mt.double() > 0).double()
        assert torch.equal(Gn[:, c:], G0[:, c:])
        assert rel(Gn[:, :c].double() - G0[:, :c].double(), alpha.double() * m * prod) < 2e-5
        sums = f32(out["sums"], 2, c)
        assert rel(sums[0], (prod * m).sum(0)) < 5e-5 and rel(sums[1], (prod * m * x.double()).sum(0)) < 5e-5
    return [Contract("dense_dgrad1_acc " + sid(s), {"partials": P * 2 * c * 4}, {"G": N * Ct * 4, "sums": 2 * c * 4}, run, anchor,
                     init={"G": G0d}, expect=0 if sb else EINVAL)]


# shape (B, H, W, Ct, coff): "B3-5x9" of test_dense_dgrad3_mask_and_fold_against_float64. Partial rows [P][2][128] floats are
# P * 1024 bytes: no shape gives a size that is not a multiple of 512.
DGRAD3_SHAPES = [(3, 5, 9, 96, 64)]


def dgrad3_need(lib, s):
    return {"ossid_dense_dgrad3_mask_partials": int(lib.fn("ossid_dense_dgrad3_mask_partials")(*s[:3]))}


def dgrad3_pred(lib, s):
    B, H, W = s[:3]
    P = dgrad3_need(lib, s)["ossid_dense_dgrad3_mask_partials"]
    assert P >= 3 and H % 4 and W % 8 and P <= B * math.ceil(H / 4) * math.ceil(W / 8)


def dgrad3_build(lib, s):
    B, H, W, Ct, coff = s
    N = B * H * W
    g = gen(N + Ct + coff)
    gs = torch.randn(N, 32, generator=g)
    Gfull = torch.full((N, Ct), float("nan"))
    Gfull[:, coff:coff + 32] = gs
    y1, ms, mt = _away(N, MID, g)
    alpha = torch.randn(MID, generator=g)
    w2 = torch.randn(32, MID, 3, 3, generator=g) / (MID * 9) ** 0.5
    Gd, y1d, al, msd, mtd = Gfull.cuda(), y1.cuda(), alpha.cuda(), ms.cuda(), mt.cuda()
    sb = split_bf16(lib)
    wpk = packed(w2, "dgrad") if sb else y1d
    P = dgrad3_need(lib, s)["ossid_dense_dgrad3_mask_partials"]

    def run(ws, out):
        rc = lib.fn("ossid_dense_dgrad3_mask")(Gd.view(-1)[coff:].data_ptr(), Ct, wpk.data_ptr(), y1d.data_ptr(), out["db"].ptr, B, H, W,
                                               al.data_ptr(), msd.data_ptr(), mtd.data_ptr(), ws["partials"].ptr, stream(lib))
        return rc or _colsum(lib, ws["partials"].ptr, P, MID, out, "sums")

    def anchor(out):       # the bounds of test_dense_train_gpu.py::test_dense_dgrad3_mask_and_fold_against_float64
        gimg = gs.double().view(B, H, W, 32).permute(0, 3, 1, 2)
        conv = torch.nn.functional.conv_transpose2d(gimg, w2.double(), padding=1).permute(0, 2, 3, 1).reshape(N, MID)
        m = (y1.double() * ms.double() + mt.double() > 0).double()
        assert rel(f32(out["db"], N, MID), alpha.double() * m * conv) < 2e-5
        sums = f32(out["sums"], 2, MID)
        assert rel(sums[0], (conv * m).sum(0)) < 5e-5 and rel(sums[1], (conv * m * y1.double()).sum(0)) < 5e-5
    return [Contract("dense_dgrad3_mask " + sid(s), {"partials": P * 2 * MID * 4}, {"db": N * MID * 4, "sums": 2 * MID * 4}, run, anchor,
                     expect=0 if sb else EINVAL)]


# ---- D4 / D16 the training stem: ossid_dw_add_stats_nhwc, ossid_stem_pool_bwd -----------------------------------------------------
# shape (B, H, W, C) = a case of test_train_ops_gpu.py::test_stem_tail_fused_modulation_batchnorm_relu_pool_matches_torch_autograd,
# which pins both entries at this very shape through train_ops.StemTail; partial rows are [P][2][C] floats.
STEMEL_SHAPES = [(3, 21, 27, 16)]


def dwadd_need(lib, s):
    return {"ossid_dw_add_stats_partials": int(lib.fn("ossid_dw_add_stats_partials")(*s))}


def poolbwd_need(lib, s):
    return {"ossid_stem_pool_bwd_partials": int(lib.fn("ossid_stem_pool_bwd_partials")(*s))}


def dwadd_pred(lib, s):
    B, H, W, C = s
    P = dwadd_need(lib, s)["ossid_dw_add_stats_partials"]
    assert P >= 3 and H % 2 == 1 and W % 2 == 1 and P == B * math.ceil(H / 2) * math.ceil(W / ((256 // (C // 4)) * 4))
    assert (P * 2 * C * 4) % 512 != 0


def poolbwd_pred(lib, s):
    B, H, W, C = s
    P = poolbwd_need(lib, s)["ossid_stem_pool_bwd_partials"]
    assert P >= 3 and H % 2 == 1 and W % 2 == 1 and (P * 2 * C * 4) % 512 != 0


def dwadd_build(lib, s):
    B, H, W, C = s
    g = gen(B * 100 + C + H)
    x = torch.randn(B, C, H, W, generator=g)
    k = torch.randn(1, C, 3, 3, generator=g) * 0.3
    xd, kd = nhwc(x), k.cuda()
    P = dwadd_need(lib, s)["ossid_dw_add_stats_partials"]

    def run(ws, out):      # the partial rows are what ossid_bn_fold_fwd combines: summed here in the same fixed order
        rc = lib.fn("ossid_dw_add_stats_nhwc")(xd.data_ptr(), kd.data_ptr(), 0, B, H, W, C, 0, out["y"].ptr, ws["partials"].ptr,
                                               out["pivot"].ptr, stream(lib))
        return rc or _colsum(lib, ws["partials"].ptr, P, C, out, "sums")

    def anchor(out):       # that test's bound on the output (1e-5) and on the batch statistics (running mean / variance: 1e-5)
        y64 = _dw_ref(x.double(), k.double().expand(B, -1, -1, -1)).permute(0, 2, 3, 1)
        y = f32(out["y"], B, H, W, C)
        assert rel(y, y64) < 1e-5
        assert torch.equal(f32(out["pivot"], C), y[0, 0, 0])
        d = (y.double() - y[0, 0, 0].double()).reshape(-1, C)
        sums = f32(out["sums"], 2, C)
        assert rel(sums[0], d.sum(0)) < 1e-5 and rel(sums[1], (d * d).sum(0)) < 1e-5
    return [Contract("dw_add_stats " + sid(s), {"partials": P * 2 * C * 4}, {"y": B * H * W * C * 4, "pivot": C * 4, "sums": 2 * C * 4},
                     run, anchor)]


def poolbwd_build(lib, s):
    B, H, W, C = s
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = gen(B * 100 + C + W)
    m = torch.randn(B, C, H, W, generator=g)
    scale = 1 + 0.3 * torch.randn(C, generator=g)
    scale[0] = -0.7
    shift = 0.3 * torch.randn(C, generator=g)
    dp = torch.randn(B, C, Ho, Wo, generator=g)
    md, sd, td, dpd = nhwc(m), scale.cuda(), shift.cuda(), nhwc(dp)
    pooled = torch.empty(B * Ho * Wo * C, device="cuda")
    argmax = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device="cuda")
    rc = lib.fn("ossid_stem_pool_fwd")(md.data_ptr(), sd.data_ptr(), td.data_ptr(), B, H, W, C, pooled.data_ptr(), argmax.data_ptr(),
                                       stream(lib))
    assert rc == 0
    P = poolbwd_need(lib, s)["ossid_stem_pool_bwd_partials"]

    def run(ws, out):
        rc = lib.fn("ossid_stem_pool_bwd")(md.data_ptr(), argmax.data_ptr(), dpd.data_ptr(), sd.data_ptr(), td.data_ptr(), None, None,
                                           B, H, W, C, ws["partials"].ptr, None, stream(lib))
        return rc or _colsum(lib, ws["partials"].ptr, P, C, out, "sums")

    def anchor(out):       # (sum gm, sum gm m) by float64 autograd; that test's 1e-4 on the BatchNorm gradients they become
        a = (m.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).requires_grad_(True)
        torch.nn.functional.max_pool2d(torch.relu(a), 3, 2, 1).backward(dp.double())
        gm = a.grad
        sums = f32(out["sums"], 2, C).double()
        want = torch.stack([gm.sum((0, 2, 3)), (gm * m.double()).sum((0, 2, 3))])
        for i in range(2):
            assert float((sums[i] - want[i]).norm() / want[i].norm()) < 1e-4, i
    return [Contract("stem_pool_bwd " + sid(s), {"partials": P * 2 * C * 4}, {"sums": 2 * C * 4}, run, anchor)]


# ---- the detector side's table ---------------------------------------------------------------------------------------------------
TRAIN_CASES = [
    Case("conv_wgrad", ["ossid_conv_wgrad_workspace_bytes"], WGRAD_SHAPES, wgrad_need, wgrad_pred, wgrad_build,
         [R("ossid_conv_wgrad_workspace_bytes", 0, 5, 7, 16, 16, 9), R("ossid_conv_wgrad_workspace_bytes", 1, 5, 7, 16, 16, 4),
          R("ossid_conv_wgrad_workspace_bytes", 1, 5, 7, 0, 16, 9), R("ossid_conv_wgrad_workspace_bytes", 1, 1 << 15, 1 << 15, 16, 16, 9)]),
    # (every share is rounded to 256 bytes and the device decides the tiled kernels' slab counts)
    Case("conv_wgrad_group", ["ossid_conv_wgrad_group_workspace_bytes"], GROUP_SHAPES, group_need, group_pred, group_build,
         [R("ossid_conv_wgrad_group_workspace_bytes", None, 3),
          ("ossid_conv_wgrad_group_workspace_bytes", lambda lib: group_need(lib, GROUP_SHAPES[0][:3] + (GROUP_SHAPES[0][3][:0],))),
          ("ossid_conv_wgrad_group_workspace_bytes", lambda lib: group_need(lib, GROUP_SHAPES[0][:3] + (((16, 16, 9),) * 49,))),
          ("ossid_conv_wgrad_group_workspace_bytes", lambda lib: group_need(lib, GROUP_SHAPES[0][:3] + (((16, 16, 5),) * 3,)))], ragged=False),
    # (64 * 147 floats per resident workgroup: the device decides how many)
    Case("stem_conv_wgrad", ["ossid_stem_conv_wgrad_workspace_bytes"], STEM_SHAPES, stem_need, stem_pred, stem_build,
         [R("ossid_stem_conv_wgrad_workspace_bytes", 0, 53, 77), R("ossid_stem_conv_wgrad_workspace_bytes", 3, 0, 77),
          R("ossid_stem_conv_wgrad_workspace_bytes", 3, 53, -1)], ragged=False),
    Case("dw_bwd_k", ["ossid_dw_bwd_k_workspace_floats"], DWK_SHAPES, dwk_need, dwk_pred, dwk_build,
         [R("ossid_dw_bwd_k_workspace_floats", 0, 9, 129, 64), R("ossid_dw_bwd_k_workspace_floats", 1, 9, 129, 6),
          R("ossid_dw_bwd_k_workspace_floats", 1, 9, 129, 48), R("ossid_dw_bwd_k_workspace_floats", 1, 9, 129, 512)],
         nbytes=lambda lib, s: [4 * dwk_need(lib, s)["ossid_dw_bwd_k_workspace_floats"]]),
    Case("conv1x1_c1_bwd", ["ossid_conv1x1_c1_bwd_workspace_floats"], C1_SHAPES, c1_need, c1_pred, c1_build,
         [R("ossid_conv1x1_c1_bwd_workspace_floats", 0, 8), R("ossid_conv1x1_c1_bwd_workspace_floats", 199, 0)],
         nbytes=lambda lib, s: [4 * c1_need(lib, s)["ossid_conv1x1_c1_bwd_workspace_floats"]]),
    Case("focal_smoothl1_loss", ["ossid_focal_smoothl1_loss_workspace_floats"], LOSS_SHAPES, loss_need, loss_pred, loss_build,
         [R("ossid_focal_smoothl1_loss_workspace_floats", 0, 300), R("ossid_focal_smoothl1_loss_workspace_floats", 3, 0)],
         nbytes=lambda lib, s: [4 * loss_need(lib, s)["ossid_focal_smoothl1_loss_workspace_floats"]]),
    Case("conv3x3_wino", ["ossid_conv3x3_wino_workspace_bytes", "ossid_conv3x3_wino_pair_workspace_bytes"], WINO_SHAPES, wino_need,
         wino_pred, wino_build, [("ossid_conv3x3_wino_workspace_bytes", lambda lib: wino_need(lib, (3, 120, 32, 5, 7))),     # Cin % 16
          ("ossid_conv3x3_wino_workspace_bytes", lambda lib: wino_need(lib, (0, 128, 32, 5, 7))),
          ("ossid_conv3x3_wino_pair_workspace_bytes", lambda lib: wino_need(lib, (3, 128, 32, 0, 7)))],
         ragged=False),
    Case("detect_post", ["ossid_topk_workspace_bytes", "ossid_nms_workspace_bytes", "ossid_detect_post_workspace_bytes"], POST_SHAPES,
         post_need, post_pred, post_build, []),           # (the header names no bad arguments for these three)
    Case("chan_op", ["ossid_chan_op_partials"], CHAN_SHAPES, chan_need, chan_pred, chan_build, [], nbytes=chan_nbytes),
    Case("dense_fwd1_stats", ["ossid_dense_fwd1_stats_partials"], DENSE_SHAPES, fwd1_need, fwd1_pred, fwd1_build_with_fold, [],
         nbytes=fwd1_nbytes),
    Case("dense_dgrad1_acc", ["ossid_dense_dgrad1_acc_partials"], DENSE_SHAPES, dgrad1_need, dgrad1_pred, dgrad1_build, [],
         nbytes=dgrad1_nbytes),
    Case("dense_dgrad3_mask", ["ossid_dense_dgrad3_mask_partials"], DGRAD3_SHAPES, dgrad3_need, dgrad3_pred, dgrad3_build, [],
         nbytes=lambda lib, s: [dgrad3_need(lib, s)["ossid_dense_dgrad3_mask_partials"] * 2 * MID * 4], ragged=False),
    Case("dw_add_stats", ["ossid_dw_add_stats_partials"], STEMEL_SHAPES, dwadd_need, dwadd_pred, dwadd_build,
         [R("ossid_dw_add_stats_partials", 0, 21, 27, 16), R("ossid_dw_add_stats_partials", 3, 21, 27, 6),
          R("ossid_dw_add_stats_partials", 3, 21, 27, 48)],
         nbytes=lambda lib, s: [dwadd_need(lib, s)["ossid_dw_add_stats_partials"] * 2 * s[3] * 4]),
    Case("stem_pool_bwd", ["ossid_stem_pool_bwd_partials"], STEMEL_SHAPES, poolbwd_need, poolbwd_pred, poolbwd_build,
         [R("ossid_stem_pool_bwd_partials", 3, 0, 27, 16), R("ossid_stem_pool_bwd_partials", 3, 21, 27, 12)],
         nbytes=lambda lib, s: [poolbwd_need(lib, s)["ossid_stem_pool_bwd_partials"] * 2 * s[3] * 4]),
]


# =================================================================================================================================
# Pose, rendering and evaluation side
# =================================================================================================================================
def i32(g, *shape):
    return g.view(torch.int32).view(*shape).cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


def up(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.from_numpy(a).cuda()


# ---- Z3 ossid_pn2_score ----------------------------------------------------------------------------------------------------------
# shape (B, M) with the product's npoint 512 / 128: B odd and more than the eight hypotheses one persistent slice of the SA
# kernels takes, M no multiple of 64. Debug outputs on: every stage is an output.
PN2_SHAPES = [(5, 640), (13, 777)]
NP1, NP2 = 512, 128


def pn2_need(lib, s):
    return {"ossid_pn2_workspace_bytes": int(lib.fn("ossid_pn2_workspace_bytes")(s[0], s[1], NP1, NP2))}


def pn2_pred(lib, s):
    B, M = s
    assert B % 2 == 1 and B > 1 and M >= NP1 and (M % 64 or s == PN2_SHAPES[0])
    assert pn2_need(lib, s)["ossid_pn2_workspace_bytes"] > 0


def _pn2_inputs(s):
    B, M = s
    rng = np.random.default_rng(100 * B + M)
    px = np.zeros((B, M, 8), np.float32)
    px[..., :2] = rng.uniform(-1, 1, (B, M, 2)).astype(np.float32)
    px[..., 3:] = rng.uniform(-1, 1, (B, M, 5)).astype(np.float32)
    return px


def pn2_build(lib, s):
    from oracle import zephyr_oracle
    from ossid_code_amd.zephyr.pointnet2 import fold_pn2
    from test_oracle import _model
    B, M = s
    zephyr_oracle.build()
    px = _pn2_inputs(s)
    m = _model(B)
    want, wdbg = zephyr_oracle.pn2_score(px, fold_pn2(m), debug=True)
    m = m.cuda()
    w = m.packed_weights(torch.device("cuda", torch.cuda.current_device()))
    pxd = up(px)
    need = pn2_need(lib, s)["ossid_pn2_workspace_bytes"]
    stages = (("fps1", (B, NP1), np.int32), ("ball1", (B, NP1, 64), np.int32), ("feat1", (B, NP1, 128), np.float32),
              ("fps2", (B, NP2), np.int32), ("ball2", (B, NP2, 64), np.int32), ("feat2", (B, NP2, 256), np.float32),
              ("feat3", (B, 1024), np.float32))
    outs = {"scores": 4 * B}
    outs.update((k, 4 * int(np.prod(sh))) for k, sh, _ in stages)

    def run(ws, out):
        return lib.fn("ossid_pn2_score")(pxd.data_ptr(), B, M, ctypes.byref(w), ws["ws"].ptr, ws["ws"].nbytes, out["scores"].ptr,
                                         *[out[k].ptr for k, _, _ in stages], None, stream(lib))

    def anchor(out):       # the oracle, bit for bit, as tests/test_pn2_granules_gpu.py::test_every_stage_bit_exact
        for k, sh, dt in stages:
            got = out[k].payload.cpu().numpy().view(dt).reshape(sh)
            assert got.shape == wdbg[k].shape and np.array_equal(got, wdbg[k]), k
        assert np.array_equal(out["scores"].payload.cpu().numpy().view(np.float32), want)
    c = Contract("pn2_score " + sid(s), {"ws": need}, outs, run, anchor, short=("ws",), misalign=("ws",))
    c.keep = m
    return [c]


# ---- Z3t ossid_pn2_train_forward + _backward ---------------------------------------------------------------------------------------
# shape (B, M, npoint1, npoint2) = S1 of tests/test_pn2_train_gpu.py, which pins scores and every gradient of this shape to
# float64; forward and backward run as one unit on one workspace. Every piece of the workspace is rounded to 256 bytes and S1's
# sum is a multiple of 512: the same step at B = 3 is the shape whose size is not.
PN2T_SHAPES = [(4, 96, 32, 32), (3, 96, 32, 32)]


def pn2t_need(lib, s):
    return {"ossid_pn2_train_workspace_bytes": int(lib.fn("ossid_pn2_train_workspace_bytes")(*s))}


def pn2t_pred(lib, s):
    B, M, np1, np2 = s
    assert B >= 2 and M >= np1 >= np2 and np1 % 32 == 0 and np2 % 32 == 0 and M < 64 * 2      # every ball padded
    assert pn2t_need(lib, s)["ossid_pn2_train_workspace_bytes"] > 0


def pn2t_build(lib, s):
    import copy
    import ref_pn2_train as rt
    from ossid_code_amd import zephyr
    B, M, np1, np2 = s
    g = gen(11)
    cpu = rt.init_model(zephyr.PointNet2SSG(8, None, 1), 7)
    cpu.SA_modules[0].npoint, cpu.SA_modules[1].npoint = np1, np2
    x = rt.make_inputs(B, M, 3)
    keep = (torch.rand(B, 256, generator=g) >= 0.5).to(torch.uint8)
    dsc = torch.randn(B, 1, generator=g)
    gpu = copy.deepcopy(cpu).cuda().train()
    lin, bns = gpu.train_layers()
    params = [m.weight for m in lin] + [b.weight for b in bns] + [b.bias for b in bns] + [lin[11].bias]
    tensors = [p.detach().reshape(p.shape[0], -1).contiguous().float() if p.dim() > 1 else p.detach().contiguous().float()
               for p in params]
    st = lib.PN2TrainParams()
    for i in range(12):
        st.w[i] = tensors[i].data_ptr()
    for i in range(11):
        st.gamma[i], st.beta[i] = tensors[12 + i].data_ptr(), tensors[23 + i].data_ptr()
    st.bias = tensors[34].data_ptr()
    st.npoint1, st.npoint2 = np1, np2
    st.radius1, st.radius2 = gpu.SA_modules[0].radius, gpu.SA_modules[1].radius
    xd, kd, dd = x.cuda(), keep.cuda(), dsc.reshape(B).contiguous().cuda()
    need = pn2t_need(lib, s)["ossid_pn2_train_workspace_bytes"]
    outs = {"scores": 4 * B}
    outs.update(("g%d" % i, 4 * t.numel()) for i, t in enumerate(tensors))

    def run(ws, out):
        rc = lib.fn("ossid_pn2_train_forward")(xd.data_ptr(), B, M, ctypes.byref(st), kd.data_ptr(), 0.5, ws["ws"].ptr, ws["ws"].nbytes,
                                               out["scores"].ptr, None, stream(lib))
        if rc:
            return rc
        gr = lib.PN2TrainGrads()
        for i in range(12):
            gr.w[i] = out["g%d" % i].ptr
        for i in range(11):
            gr.gamma[i], gr.beta[i] = out["g%d" % (12 + i)].ptr, out["g%d" % (23 + i)].ptr
        gr.bias = out["g34"].ptr
        return lib.fn("ossid_pn2_train_backward")(dd.data_ptr(), B, M, ctypes.byref(st), 0.5, ws["ws"].ptr, ws["ws"].nbytes,
                                                  ctypes.byref(gr), stream(lib))

    def anchor(out):       # the module's own step, which test_pn2_train_gpu.py holds to float64 at this shape: the same bits
        res = gpu({"point_x": xd}, keep_mask=keep)
        res.backward(dsc.cuda())
        torch.cuda.synchronize()
        assert torch.equal(out["scores"].view(torch.float32), res.detach().reshape(B))
        for i, p in enumerate(params):
            assert torch.equal(out["g%d" % i].view(torch.float32), p.grad.reshape(-1)), i
    return [Contract("pn2_train " + sid(s), {"ws": need}, outs, run, anchor, short=("ws",), misalign=("ws",))]


# ---- Z3t ossid_pn2_train_linear_wgrad ----------------------------------------------------------------------------------------------
# shape (R, K, C) of tests/test_pn2_train_gpu.py::test_linear_kernels_alone: K the padded width, the weight has the real one;
# then two row counts of tests/pn2_train_cases.py: a second split of one row, and a chunk grown past 512 with a ragged tail
PN2W_SHAPES = [(160, 264, 256), (5, 256, 1), (513, 8, 64), (131073, 8, 64)]


def _kr(K):
    return {136: 131, 264: 259}.get(K, K)


def pn2w_need(lib, s):
    R, K, C = s
    return {"ossid_pn2_train_wgrad_workspace_bytes": int(lib.fn("ossid_pn2_train_wgrad_workspace_bytes")(R, C, _kr(K)))}


def pn2w_pred(lib, s):
    R, K, C = s
    chunk, splits, tail = pn2_train_cases.wgrad_split(R)
    assert (s == PN2W_SHAPES[0] and _kr(K) != K and R % 64) or (s == PN2W_SHAPES[1] and C == 1 and R < 8) or \
        (s == PN2W_SHAPES[2] and (chunk, splits, tail) == (512, 2, 1)) or \
        (s == PN2W_SHAPES[3] and chunk > 512 and splits > 2 and tail % 16 != 0)
    need = pn2w_need(lib, s)["ossid_pn2_train_wgrad_workspace_bytes"]
    assert need == (splits * C * _kr(K) * 4 if splits > 1 else 0) + 256


def pn2w_build(lib, s):
    R, K, C = s
    Kr = _kr(K)
    g = gen(R + K + C)
    X = torch.zeros(R, K)
    X[:, :Kr] = torch.randn(R, Kr, generator=g)
    torch.randn(C, Kr, generator=g)
    dZ = torch.randn(R, C, generator=g)
    Xd, dZd = X.cuda(), dZ.cuda()
    need = pn2w_need(lib, s)["ossid_pn2_train_wgrad_workspace_bytes"]

    def run(ws, out):
        return lib.fn("ossid_pn2_train_linear_wgrad")(dZd.data_ptr(), R, C, Xd.data_ptr(), K, Kr, out["dW"].ptr, ws["ws"].ptr,
                                                      ws["ws"].nbytes, stream(lib))

    def anchor(out):       # that test's bound: 4 x the error of the same product in float32 torch
        want64, ref32 = dZ.double().t() @ X[:, :Kr].double(), dZ.t() @ X[:, :Kr]
        ref = float(want64.abs().max())
        e32 = float((ref32.double() - want64).abs().max()) / ref
        err = float((f32(out["dW"], C, Kr).double() - want64).abs().max()) / ref
        assert err <= 4 * e32, (err, e32)
    return [Contract("pn2_train_linear_wgrad " + sid(s), {"ws": need}, {"dW": 4 * C * Kr}, run, anchor, short=("ws",))]


# ---- SPEC 6.9 ossid_ppf_refine_model_grid / ossid_ppf_refine / ossid_ppf_refine_match ----------------------------------------------
# shape (scene index of tests/ref_ppf.py, num_poses, slack): the object and frame 0 of tests/test_ppf_refine_gpu.py, the
# scene sample taken by the restatement (the device's is pinned equal to it there), cap = its count + slack
PPFR_SHAPES = [(0, 3, 37)]


def _ppfr_host(s):
    import functools
    import ref_ppf as rp
    import ref_ppf_refine as rr

    @functools.lru_cache(maxsize=None)
    def make(scene, n_poses, slack):
        import ref_icp as ri
        P, N = rp.object_model()
        rm = rr.RefineModel(P, N)
        depth, K, mask, T = rp.scene(scene)
        _idx, S = rr.scene_points(rp.depth2cloud(depth, mask, K), rm.D)
        poses = [T, ri.perturb(T, [1.0, 0.2, 0.1], 6.0, [0.004, 0.0, -0.003]), ri.perturb(T, [0.1, 1.0, -0.3], 4.0, [-0.002, 0.003, 0.002])]
        return rm, S, np.stack(poses[:n_poses]), len(S) + slack
    if not hasattr(_ppfr_host, "make"):
        _ppfr_host.make = make
    return _ppfr_host.make(*s)


def ppfr_need(lib, s):
    import ref_ppf_refine as rr
    rm, S, poses, cap = _ppfr_host(s)
    return {"ossid_ppf_refine_grid_bytes": int(lib.fn("ossid_ppf_refine_grid_bytes")(len(rm.idx), rr.REFINE_STEPS, float(rm.D), float(rm.h))),
            "ossid_ppf_refine_workspace_bytes": int(lib.fn("ossid_ppf_refine_workspace_bytes")(cap, len(poses)))}


def ppfr_pred(lib, s):
    rm, S, poses, cap = _ppfr_host(s)
    assert len(poses) % 2 == 1 and len(poses) >= 3 and len(S) > 256 and cap > len(S) and cap % 64 != 0
    assert all(v > 0 for v in ppfr_need(lib, s).values())


def ppfr_build(lib, s):
    import ref_ppf_refine as rr
    rm, S, poses, cap = _ppfr_host(s)
    NR, Mr, steps, D, h = len(poses), len(rm.idx), rr.REFINE_STEPS, float(rm.D), float(rm.h)
    need = ppfr_need(lib, s)
    wsz = {"grid": need["ossid_ppf_refine_grid_bytes"], "ws": need["ossid_ppf_refine_workspace_bytes"]}
    pts, nrm = up(rm.P, np.float32), up(rm.N, np.float32)
    Sd = torch.zeros(cap, 3, dtype=torch.float32, device="cuda")
    Sd[:len(S)] = up(S, np.float32)
    cnt = torch.tensor([len(S)], dtype=torch.int32, device="cuda")
    Td = up(poses, np.float64)
    nh = torch.tensor([NR], dtype=torch.int32, device="cuda")
    thr = rr.thresholds(rm.D, rm.h)

    def grid(ws):
        return lib.fn("ossid_ppf_refine_model_grid")(pts.data_ptr(), nrm.data_ptr(), Mr, steps, D, h, ws["grid"].ptr, ws["grid"].nbytes, None)

    def run_match(ws, out):
        rc = grid(ws)
        for step in (0, steps - 1):
            rc = rc or lib.fn("ossid_ppf_refine_match")(Sd.data_ptr(), cnt.data_ptr(), cap, ws["grid"].ptr, ws["grid"].nbytes, Mr,
                                                        Td.data_ptr(), NR, steps, step, D, h, ws["ws"].ptr, ws["ws"].nbytes,
                                                        out["match%d" % step].ptr, None)
        return rc

    def anchor_match(out):     # the brute force of test_ppf_refine_gpu.py::test_correspondences_equal_the_brute_force
        for step in (0, steps - 1):
            got = i32(out["match%d" % step], NR, cap)[:, :len(S)]
            for i, Tp in enumerate(poses):
                si, mi, _d2, _X = rr.correspondences(Tp, S, rm.P, thr[step])
                want = np.full(len(S), -1, dtype=np.int32)
                want[si] = mi
                assert np.array_equal(got[i], want), (step, i)

    def run_refine(ws, out):
        return grid(ws) or lib.fn("ossid_ppf_refine")(Sd.data_ptr(), cnt.data_ptr(), cap, ws["grid"].ptr, ws["grid"].nbytes, Mr, Td.data_ptr(),
                                                      nh.data_ptr(), NR, steps, D, h, ws["ws"].ptr, ws["ws"].nbytes, out["poses"].ptr,
                                                      out["scores"].ptr, out["pairs"].ptr, out["steps_done"].ptr, out["status"].ptr, None)

    def anchor_refine(out):    # the bounds of test_ppf_refine_gpu.py::test_one_step_and_full_run_equal_the_restatement
        one = [rr.refine_one(Tp, S, rm) for Tp in poses]
        order = sorted(range(NR), key=lambda i: (-one[i][1], i))
        P = out["poses"].view(torch.float64).view(NR, 4, 4).cpu().numpy()
        sc = out["scores"].view(torch.float64).cpu().numpy()
        pr, sd, status = i32(out["pairs"], NR), i32(out["steps_done"], NR), i32(out["status"], 4)
        for row, i in enumerate(order):
            T5, n5, d5 = one[i]
            assert np.abs(P[row] - T5).max() <= 1e-6 and pr[row] == n5 and sd[row] == d5 and sc[row] == n5 / float(Mr), (row, i)
        assert list(status) == [0, len(S), NR, 0]
    return [Contract("ppf_refine_match " + sid(s), wsz, {"match0": 4 * NR * cap, "match%d" % (steps - 1): 4 * NR * cap}, run_match,
                     anchor_match, short=("grid", "ws")),
            Contract("ppf_refine " + sid(s), wsz, {"poses": 128 * NR, "scores": 8 * NR, "pairs": 4 * NR, "steps_done": 4 * NR, "status": 16},
                     run_refine, anchor_refine, short=("grid", "ws"))]


# ---- SPEC 7 ossid_raster_depth / ossid_raster_color / ossid_raster_textured --------------------------------------------------------
# shape (mesh name, N poses, H, W): the icosphere(2) and the 12-face cube of tests/ref_scene.py under its camera
RASTER_SHAPES = [("sphere", 3, 40, 56), ("cube", 3, 40, 56)]


def _raster_mesh(name):
    import ref_raster as rr
    import ref_scene as rs
    if name == "cube":
        return rs.cube(0.05)
    sv, sf = rr.icosphere(2)
    return 0.06 * sv, sf


def raster_need(lib, s):
    V, F = _raster_mesh(s[0])
    return {"ossid_raster_workspace_bytes": int(lib.fn("ossid_raster_workspace_bytes")(len(V), len(F), s[1])),
            "ossid_raster_color_workspace_bytes": int(lib.fn("ossid_raster_color_workspace_bytes")(len(V), len(F), s[1], s[2], s[3]))}


def raster_pred(lib, s):
    V, F = _raster_mesh(s[0])
    name, N, H, W = s
    assert N == 3 and (H, W) == (40, 56) and len(F) == (12 if name == "cube" else 320)
    n = raster_need(lib, s)
    assert n["ossid_raster_workspace_bytes"] == 16 * N * len(V) and n["ossid_raster_color_workspace_bytes"] == 16 * N * len(V) + 8 * N * H * W
    assert all(v % 512 for v in n.values())


def raster_build(lib, s):
    import ref_raster as rr
    import ref_raster_color as rc
    import ref_raster_textured as rt
    import ref_scene as rs
    name, N, H, W = s
    V, F = _raster_mesh(name)
    rng = np.random.default_rng(len(F))
    C = rng.integers(0, 256, (len(V), 3)).astype(np.uint8)
    k = 0.7 / np.abs(V[:, 0]).max()
    UV = (0.5 + k * np.asarray(V)[:, :2]).astype(np.float32)          # past the texture's edge on both sides
    tex = rng.integers(0, 256, (12, 20, 3)).astype(np.uint8)
    levels = rt.mip_chain(tex)
    poses = np.stack([rr.pose_at((-0.10, 0.0, 0.60)), rr.pose_at((0.02, 0.0, 0.50)), rr.pose_at((0.25, 0.0, 0.62))])   # the last: cut by the edge
    cam = [float(v) for v in rs.CAM]
    Kc = rc.cam_matrix(*cam)
    v, f, c, uv = up(V, np.float32), up(F, np.int32).reshape(-1, 3), up(C), up(UV)
    T = up(poses.astype(np.float32))
    cams = up(np.tile(np.array(cam, np.float32), (N, 1)))
    mb = int(lib.fn("ossid_texture_mip_bytes")(12, 20))
    mips = torch.empty(mb, dtype=torch.uint8, device="cuda")
    texd = up(tex)
    assert lib.fn("ossid_texture_mips")(texd.data_ptr(), 12, 20, mips.data_ptr(), mb, stream(lib)) == 0
    need = raster_need(lib, s)
    px = N * H * W

    def run_depth(ws, out):
        return lib.fn("ossid_raster_depth")(v.data_ptr(), len(V), f.data_ptr(), len(F), T.data_ptr(), N, *cam, H, W, 0.0, 0.05,
                                            ws["ws"].ptr, ws["ws"].nbytes, out["depth"].ptr, out["stats"].ptr, stream(lib))

    def run_color(ws, out):
        return lib.fn("ossid_raster_color")(v.data_ptr(), len(V), f.data_ptr(), len(F), c.data_ptr(), T.data_ptr(), N, cams.data_ptr(),
                                            H, W, 0.0, 0.05, ws["ws"].ptr, ws["ws"].nbytes, out["color"].ptr, out["depth"].ptr,
                                            out["face"].ptr, out["stats"].ptr, stream(lib))

    def run_tex(ws, out):
        return lib.fn("ossid_raster_textured")(v.data_ptr(), len(V), f.data_ptr(), len(F), uv.data_ptr(), mips.data_ptr(), mb, 12, 20,
                                               T.data_ptr(), N, cams.data_ptr(), H, W, 0.0, 0.05, ws["ws"].ptr, ws["ws"].nbytes,
                                               out["color"].ptr, out["depth"].ptr, out["face"].ptr, out["lod"].ptr, out["stats"].ptr,
                                               stream(lib))

    def anchor_depth(out):     # tests/ref_raster.py, bit for bit, as tests/test_raster_gpu.py
        d, st = out["depth"].view(torch.float32).view(N, H, W).cpu().numpy(), i32(out["stats"], N, 4)
        for i in range(N):
            want, _count, wstats = rr.render(V, F, poses[i], Kc, (H, W), pixel_offset=0.0)
            assert np.array_equal(d[i], want) and st[i, :3].tolist() == wstats.tolist(), i
        assert d.any()

    def anchor_color(out):     # tests/ref_raster_color.py, bit for bit, as tests/test_raster_color_gpu.py
        col = out["color"].payload.view(N, H, W, 3).cpu().numpy()
        d, fc, st = out["depth"].view(torch.float32).view(N, H, W).cpu().numpy(), i32(out["face"], N, H, W), i32(out["stats"], N, 4)
        for i in range(N):
            wc, wd, wf, ws_ = rc.render(V, F, C, poses[i], Kc, (H, W), pixel_offset=0.0)
            assert np.array_equal(d[i], wd) and np.array_equal(fc[i], wf) and np.array_equal(col[i], wc) and st[i, :3].tolist() == ws_.tolist(), i

    def anchor_tex(out):       # tests/ref_raster_textured.py, bit for bit, as tests/test_raster_textured_gpu.py
        col = out["color"].payload.view(N, H, W, 3).cpu().numpy()
        d, fc, st = out["depth"].view(torch.float32).view(N, H, W).cpu().numpy(), i32(out["face"], N, H, W), i32(out["stats"], N, 4)
        lod = i32(out["lod"], N, H, W)
        for i in range(N):
            wc, wd, wf, wl, ws_ = rt.render(V, F, UV, levels, poses[i], Kc, (H, W), pixel_offset=0.0)
            assert np.array_equal(d[i], wd) and np.array_equal(fc[i], wf) and np.array_equal(lod[i], wl) and np.array_equal(col[i], wc), i
            assert st[i, :3].tolist() == ws_.tolist(), i
    img = {"color": 3 * px, "depth": 4 * px, "face": 4 * px, "stats": 16 * N}
    return [Contract("raster_depth " + sid(s), {"ws": need["ossid_raster_workspace_bytes"]}, {"depth": 4 * px, "stats": 16 * N}, run_depth,
                     anchor_depth, short=("ws",), misalign=("ws",)),
            Contract("raster_color " + sid(s), {"ws": need["ossid_raster_color_workspace_bytes"]}, img, run_color, anchor_color,
                     short=("ws",), misalign=("ws",)),
            Contract("raster_textured " + sid(s), {"ws": need["ossid_raster_color_workspace_bytes"]}, dict(img, lod=4 * px), run_tex,
                     anchor_tex, short=("ws",), misalign=("ws",))]


# ---- SPEC 13 ossid_scene_render / ossid_scene_render_textured ------------------------------------------------------------------------
# shape (textured atlas?): the layout of tests/ref_scene.fixture() -- 40 x 56, nine instances in three scenes, one of them empty
SCENE_SHAPES = [(False,), (True,)]


def _scene_host(textured):
    import ref_scene as rs
    import ref_scene_textured as rst
    fx = rst.fixture() if textured else rs.fixture()
    counts = {}
    for o, m in fx["meshes"].items():
        counts[int(o)] = len(m[0])
    records = int(sum(counts[int(o)] for o in fx["instance_obj"]))
    return fx, records


def scene_need(lib, s):
    import ref_scene as rs
    fx, records = _scene_host(s[0])
    S = len(fx["scene_first"]) - 1
    return {"ossid_scene_workspace_bytes": int(lib.fn("ossid_scene_workspace_bytes")(records, S, rs.HW[0], rs.HW[1]))}


def scene_pred(lib, s):
    import ref_scene as rs
    fx, records = _scene_host(s[0])
    first = fx["scene_first"]
    assert rs.HW == (40, 56) and len(fx["instance_obj"]) == 9 and any(first[i] == first[i + 1] for i in range(len(first) - 1))
    assert scene_need(lib, s)["ossid_scene_workspace_bytes"] > 0


def scene_build(lib, s):
    import ref_scene as rs
    import ref_scene_textured as rst
    from ossid_code_amd import render, scenes
    textured = s[0]
    H, W = rs.HW
    if textured:
        fx, ref = rst.fixture(), rst.reference(True)
        meshes = {o: render.Mesh(V, F, colors=C, uvs=U, texture=I) for o, (V, F, C, U, I) in fx["meshes"].items()}
        atlas = scenes.MeshAtlas(meshes, use_texture=(1, 2))
    else:
        fx, ref = rs.fixture(), rs.reference()
        meshes = {o: render.Mesh(V, F, colors=C) for o, (V, F, C) in fx["meshes"].items()}
        atlas = scenes.MeshAtlas(meshes)
    layout = scenes.Layout([atlas.index_of[int(o)] for o in fx["instance_obj"]], fx["transforms"], fx["scene_first"], fx["cams"])
    S, I = layout.n_scenes, layout.n_instances
    offsets = scenes.work_offsets(atlas, layout)
    d_mesh, d_T, d_first = up(layout.instance_mesh), up(layout.transforms.astype(np.float32)), up(layout.scene_first)
    d_cams, d_off = up(layout.cams), up(offsets)
    records, items = int(offsets[-1, 1]), int(offsets[-1, 0])
    need = int(lib.fn("ossid_scene_workspace_bytes")(records, S, H, W))
    assert need == scene_need(lib, s)["ossid_scene_workspace_bytes"]
    Wd = (W + 31) // 32
    px = S * H * W
    outs = {"color": 3 * px, "depth": 4 * px, "instance": 4 * px, "face": 4 * px, "facing": 4 * px, "amodal": 4 * I * H * Wd}
    if textured:
        outs["lod"] = 4 * px

    def run(ws, out):
        desc = lib.SceneDesc(
            vertices=atlas.vertices.data_ptr(), colors=atlas.colors.data_ptr(), faces=atlas.faces.data_ptr(), meshes=atlas.table.data_ptr(),
            instance_mesh=d_mesh.data_ptr(), transforms=d_T.data_ptr(), scene_first=d_first.data_ptr(), cams=d_cams.data_ptr(),
            offsets=d_off.data_ptr(), background=None, color_out=out["color"].ptr, depth_out=out["depth"].ptr,
            instance_out=out["instance"].ptr, face_out=out["face"].ptr, facing_out=out["facing"].ptr, amodal_out=out["amodal"].ptr,
            Vt=len(atlas.vertices_host), Ft=len(atlas.faces_host), K=atlas.n_meshes, I=I, S=S, H=H, W=W, Sb=0, work_items=items,
            records=records, pixel_offset=0.0, z_near=0.05)
        if not textured:
            return lib.fn("ossid_scene_render")(ctypes.byref(desc), ws["ws"].ptr, ws["ws"].nbytes, stream(lib))
        tex = lib.SceneTex(uvs=atlas.uvs.data_ptr(), mips=atlas.mips.data_ptr(), tex_table=atlas.tex_table.data_ptr(),
                           lod_out=out["lod"].ptr, mip_texels=atlas.mips.numel() // 4)
        return lib.fn("ossid_scene_render_textured")(ctypes.byref(desc), ctypes.byref(tex), ws["ws"].ptr, ws["ws"].nbytes, stream(lib))

    def anchor(out):           # the restatement, bit for bit, as tests/test_scene_gpu.py / tests/test_scene_textured_gpu.py
        got = {"depth": out["depth"].view(torch.float32).view(S, H, W).cpu().numpy(), "instance": i32(out["instance"], S, H, W),
               "face": i32(out["face"], S, H, W), "color": out["color"].payload.view(S, H, W, 3).cpu().numpy(),
               "facing": out["facing"].view(torch.float32).view(S, H, W).cpu().numpy()}
        if textured:
            got["lod"] = i32(out["lod"], S, H, W)
        for name, g in got.items():
            assert same(g, ref[name]), name
        assert np.array_equal(i32(out["amodal"], I, H, Wd).view(np.uint32), rs.pack_amodal(ref["amodal"]))
    c = Contract("scene_render%s" % ("_textured" if textured else ""), {"ws": need}, outs, run, anchor, short=("ws",), misalign=("ws",))
    c.keep = (atlas, meshes)
    return [c]


# ---- SPEC 9 ossid_cloud_weights ------------------------------------------------------------------------------------------------------
# shape (F,): the one entry that takes the query's workspace
CLOUD_SHAPES = [(1,), (320,)]


def cloud_need(lib, s):
    return {"ossid_cloud_workspace_bytes": int(lib.fn("ossid_cloud_workspace_bytes")(s[0]))}


def cloud_pred(lib, s):
    assert s[0] in (1, 320) and cloud_need(lib, s)["ossid_cloud_workspace_bytes"] > 0


def cloud_build(lib, s):
    import ref_model_cloud as rm
    import ref_raster as rr
    Fn = s[0]
    if Fn == 1:
        V, F = np.array([[0.0, 0.0, 0.0], [0.3, 0.0, 0.1], [0.0, 0.2, 0.05]]), np.array([[0, 1, 2]], np.int32)
    else:
        sv, F = rr.icosphere(2)
        V = 0.06 * sv
    V32 = rm.f32_vertices(V)
    rng = np.random.default_rng(Fn)
    votes = rng.integers(0, 50, (Fn, 2)).astype(np.int32)
    votes[rng.random(Fn) < 0.2] = 0                                 # faces nothing saw
    if Fn == 1:
        votes[0] = (3, 7)
    v, f, vt = up(V32), up(F, np.int32).reshape(-1, 3), up(votes)
    need = cloud_need(lib, s)["ossid_cloud_workspace_bytes"]

    def run(ws, out):
        return lib.fn("ossid_cloud_weights")(v.data_ptr(), len(V32), f.data_ptr(), Fn, vt.data_ptr(), ws["ws"].ptr, ws["ws"].nbytes,
                                             out["weights"].ptr, out["prefix"].ptr, out["normals"].ptr, stream(lib))

    def anchor(out):   # as tests/test_model_cloud_gpu.py::test_weights_prefix_and_normals_equal_the_restatement
        w, P, nrm, _usable = rm.weights(V32, F, votes)
        assert np.array_equal(out["weights"].view(torch.int64).cpu().numpy().view(np.uint64), w.astype(np.uint64))
        assert np.array_equal(out["prefix"].view(torch.int64).cpu().numpy().view(np.uint64), P.astype(np.uint64))
        assert same(out["normals"].view(torch.float32).view(Fn, 3).cpu().numpy(), nrm)
    return [Contract("cloud_weights " + sid(s), {"ws": need}, {"weights": 8 * Fn, "prefix": 8 * Fn, "normals": 12 * Fn}, run, anchor,
                     short=("ws",), misalign=("ws",))]


# ---- SPEC 10 ossid_det_match ---------------------------------------------------------------------------------------------------------
# shape (N, C, T). (3000, 1500, 1), every class populated: more than 1024 tiles (a class owns at least one), which drives the
# second step of both second-level scans and the 256-stride class loop of the final kernel without the million detections
# tests/test_det_eval_gpu.py::test_second_level_of_the_scans needs.
DET_SHAPES = [(1025, 3, 2), (3000, 1500, 1)]
DET_TILE = 1024


def _det_case(s):
    from test_det_eval_gpu import make
    N, C, T = s
    if C == 3:
        return make(N, 7 + N)
    c = make(N, 5, classes=np.arange(C), C=C)
    c["det_cls"] = c["det_cls"].copy()
    c["det_cls"][:C] = np.arange(C, dtype=np.int32)                 # every class has a detection
    return c


def det_need(lib, s):
    N, C, T = s
    G = len(_det_case(s)["gt_cls"])
    return {"ossid_det_eval_workspace_bytes": int(lib.fn("ossid_det_eval_workspace_bytes")(N, G, C, T))}


def det_pred(lib, s):
    N, C, T = s
    c = _det_case(s)
    counts = np.bincount(c["det_cls"], minlength=C)
    tiles = int(np.sum((counts + DET_TILE - 1) // DET_TILE))
    if C == 1500:
        assert (counts > 0).all() and tiles > 1024 and C > 256
    else:
        assert N % DET_TILE == 1 and counts.max() < N
    assert det_need(lib, s)["ossid_det_eval_workspace_bytes"] > 0


def det_build(lib, s):
    import ref_det_eval as rde
    from ossid_code_amd import det_eval
    from test_det_eval_gpu import same_f32
    N, C, T = s
    c = _det_case(s)
    thr = (0.5, 0.75)[:T]
    r = rde.evaluate(c["det_box"], c["det_score"], c["det_cls"], c["det_image"], c["gt_box"], c["gt_cls"], c["gt_offset"],
                     c["gt_difficult"], C, thr)
    G, I = len(c["gt_cls"]), c["n_images"]
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)   # noqa: E731
    db, ds, dc, di = t(c["det_box"], torch.float32), t(c["det_score"], torch.float32), t(c["det_cls"], torch.int32), t(c["det_image"], torch.int32)
    gb, gc, go, gd = t(c["gt_box"], torch.float32), t(c["gt_cls"], torch.int32), t(c["gt_offset"], torch.int32), t(c["gt_difficult"], torch.uint8)
    best_gt = torch.empty(N, dtype=torch.int32, device="cuda")
    best_iou = torch.empty(N, dtype=torch.float32, device="cuda")
    key = torch.empty(N, dtype=torch.int64, device="cuda")
    assert lib.fn("ossid_det_claim")(db.data_ptr(), ds.data_ptr(), dc.data_ptr(), di.data_ptr(), N, gb.data_ptr(), gc.data_ptr(),
                                     go.data_ptr(), G, I, C, best_gt.data_ptr(), best_iou.data_ptr(), key.data_ptr(), stream(lib)) == 0
    order = torch.sort(key, stable=True)[1].to(torch.int32)
    class_offset = det_eval.class_offsets(dc, C)
    thr_host = np.asarray(thr, dtype=np.float32)
    need = det_need(lib, s)["ossid_det_eval_workspace_bytes"]
    names = (("status", 1, (T, N)), ("n_easy", 4, (C,)), ("p11", 4, (T, C, 11)), ("ap11", 4, (T, C)), ("apa", 8, (T, C)), ("map11", 4, (T,)),
             ("mapa", 8, (T,)), ("ctp", 4, (T, N)), ("cfp", 4, (T, N)), ("prec", 4, (T, N)), ("rec", 4, (T, N)), ("env", 4, (T, N)))
    outs = {k: b * int(np.prod(sh)) for k, b, sh in names}

    def run(ws, out):
        return lib.fn("ossid_det_match")(best_gt.data_ptr(), best_iou.data_ptr(), order.data_ptr(), class_offset.data_ptr(), N,
                                         gc.data_ptr(), gd.data_ptr(), G, C, thr_host.ctypes.data, T, ws["ws"].ptr, ws["ws"].nbytes,
                                         *[out[k].ptr for k, _, _ in names], stream(lib))

    def anchor(out):           # tests/ref_det_eval.evaluate, as tests/test_det_eval_gpu.py::assert_matches
        h = {}
        for k, b, sh in names:
            dt = {"status": np.uint8, "n_easy": np.int32, "ctp": np.int32, "cfp": np.int32, "apa": np.float64, "mapa": np.float64}.get(k, np.float32)
            h[k] = out[k].payload.cpu().numpy().view(dt).reshape(sh)
        for k in ("status", "n_easy", "ctp", "cfp"):
            assert np.array_equal(h[k], r[k]), k
        for k in ("prec", "rec", "env", "p11", "ap11", "map11"):
            assert same_f32(h[k], r[k]), k
        assert np.abs(h["apa"] - r["apa"]).max(initial=0.0) <= 1e-12 and np.abs(h["mapa"] - r["mapa"]).max() <= 1e-12
        assert np.array_equal(best_gt.cpu().numpy(), r["best_gt"]) and np.array_equal(order.cpu().numpy(), r["order"])
    return [Contract("det_match " + sid(s), {"ws": need}, outs, run, anchor, short=("ws",), misalign=("ws",))]


# ---- SPEC 11 ossid_feat_pyramid / ossid_feat_detect / ossid_feat_match -----------------------------------------------------------------
# shape (H, W): three octaves and two (a third would have a side below 8)
FEAT_SHAPES = [(65, 97), (20, 33)]
FEAT_CAP, FEAT_NM, FEAT_KP = 40, 33, 256


def feat_need(lib, s):
    H, W = s
    return {"ossid_feat_pyramid_bytes": int(lib.fn("ossid_feat_pyramid_bytes")(H, W, 3)),
            "ossid_feat_detect_workspace_bytes": int(lib.fn("ossid_feat_detect_workspace_bytes")(H, W, 3)),
            "ossid_feat_match_workspace_bytes": int(lib.fn("ossid_feat_match_workspace_bytes")(FEAT_CAP))}


def feat_pred(lib, s):
    import ref_features as rf
    H, W = s
    assert H % 2 == 1 or W % 2 == 1
    assert len(rf.octave_sizes(H, W)) == (2 if s == (20, 33) else 3)
    n = feat_need(lib, s)
    assert all(v > 0 for v in n.values())
    assert n["ossid_feat_pyramid_bytes"] >= 4 * sum(5 * h * w for h, w in rf.octave_sizes(H, W))


def feat_build(lib, s):
    import ref_features as rf
    from ossid_code_amd import features
    from test_features_gpu import _depth_plane, _smooth
    H, W = s
    img = _smooth(H, W, 2)
    depth, mask = _depth_plane(H, W, 2)
    imgd, dd, md = up(img), up(depth), up(mask.astype(np.uint8))
    need = feat_need(lib, s)
    ref_pyr = rf.pyramid(img)
    ref_kp = rf.detect(ref_pyr, depth, mask)
    levels = sum(5 * h * w for h, w in rf.octave_sizes(H, W))

    def run(ws, out):
        rc = lib.fn("ossid_feat_pyramid")(imgd.data_ptr(), H, W, 3, ws["pyramid"].ptr, ws["pyramid"].nbytes, stream(lib))
        rc = rc or lib.fn("ossid_feat_detect")(ws["pyramid"].ptr, H, W, 3, dd.data_ptr(), md.data_ptr(), features.CONTRAST, FEAT_KP,
                                               ws["ws"].ptr, ws["ws"].nbytes, out["keypoints"].ptr, out["count"].ptr, stream(lib))
        if rc == 0:            # the levels are a result too: copied out from where the header says they are
            out["levels"].payload.copy_(ws["pyramid"].payload[:4 * levels])
        return rc

    def anchor(out):           # tests/ref_features.py, as tests/test_features_gpu.py::_check_frame
        lv, off = i32(out["levels"], levels), 0
        for (h, w), want in zip(rf.octave_sizes(H, W), ref_pyr):
            assert np.array_equal(lv[off:off + 5 * h * w].reshape(5, h, w), want)
            off += 5 * h * w
        n = len(ref_kp)
        assert n <= FEAT_KP and i32(out["count"], 2).tolist() == [n, 0]
        assert np.array_equal(i32(out["keypoints"], FEAT_KP, 4)[:n], ref_kp)
    cs = [Contract("feat_pyramid+detect " + sid(s), {"pyramid": need["ossid_feat_pyramid_bytes"], "ws": need["ossid_feat_detect_workspace_bytes"]},
                   {"keypoints": 16 * FEAT_KP, "count": 8, "levels": 4 * levels}, run, anchor, short=("pyramid", "ws"))]
    if s == FEAT_SHAPES[0]:    # the matcher takes no frame: once
        rng = np.random.default_rng(FEAT_NM)
        Bm = rng.integers(0, 128, (FEAT_NM, 128)).astype(np.int8)
        Ns = 37
        A = rng.integers(0, 128, (Ns, 128)).astype(np.int8)
        take = rng.integers(0, FEAT_NM, Ns // 2)
        A[:len(take)] = np.clip(Bm[take].astype(int) + rng.integers(-3, 4, (len(take), 128)), 0, 127).astype(np.int8)
        ok = rng.random(Ns) < 0.85
        ds = torch.zeros(FEAT_CAP, 128, dtype=torch.uint8, device="cuda")
        ds[:Ns] = up(A.view(np.uint8))
        oks = torch.zeros(FEAT_CAP, dtype=torch.uint8, device="cuda")
        oks[:Ns] = up(ok.astype(np.uint8))
        cnt = torch.tensor([Ns, 0], dtype=torch.int32, device="cuda")
        dm = up(Bm.view(np.uint8))

        def run_m(ws, out):
            return lib.fn("ossid_feat_match")(ds.data_ptr(), oks.data_ptr(), cnt.data_ptr(), FEAT_CAP, dm.data_ptr(), FEAT_NM, ws["ws"].ptr,
                                              ws["ws"].nbytes, out["match"].ptr, stream(lib))

        def anchor_m(out):     # exact integers, as tests/test_features_gpu.py::test_matcher_equals_integer_arithmetic
            best, d2, w = rf.match(A, ok, Bm)
            assert np.array_equal(i32(out["match"], FEAT_CAP, 3)[:Ns], np.stack([best, d2, w], 1).astype(np.int32))
        cs.append(Contract("feat_match cap %d Nm %d" % (FEAT_CAP, FEAT_NM), {"ws": need["ossid_feat_match_workspace_bytes"]},
                           {"match": 12 * FEAT_CAP}, run_m, anchor_m, short=("ws",), misalign=("ws",)))
    return cs


POSE_CASES = [
    Case("pn2_score", ["ossid_pn2_workspace_bytes"], PN2_SHAPES, pn2_need, pn2_pred, pn2_build, []),
    Case("pn2_train", ["ossid_pn2_train_workspace_bytes"], PN2T_SHAPES, pn2t_need, pn2t_pred, pn2t_build,
         [R("ossid_pn2_train_workspace_bytes", 1, 96, 32, 32), R("ossid_pn2_train_workspace_bytes", 4, 31, 32, 32),
          R("ossid_pn2_train_workspace_bytes", 4, 96, 48, 32), R("ossid_pn2_train_workspace_bytes", 4, 96, 32, 64)]),
    Case("pn2_train_linear_wgrad", ["ossid_pn2_train_wgrad_workspace_bytes"], PN2W_SHAPES, pn2w_need, pn2w_pred, pn2w_build, []),
    Case("ppf_refine", ["ossid_ppf_refine_grid_bytes", "ossid_ppf_refine_workspace_bytes"], PPFR_SHAPES, ppfr_need, ppfr_pred, ppfr_build,
         [R("ossid_ppf_refine_grid_bytes", 0, 5, 0.2, 0.004), R("ossid_ppf_refine_grid_bytes", 20000, 5, 0.2, 0.004),
          R("ossid_ppf_refine_grid_bytes", 100, 0, 0.2, 0.004), R("ossid_ppf_refine_workspace_bytes", 70000, 10),
          R("ossid_ppf_refine_workspace_bytes", 1000, 0)]),
    Case("raster", ["ossid_raster_workspace_bytes", "ossid_raster_color_workspace_bytes"], RASTER_SHAPES, raster_need, raster_pred,
         raster_build, [R("ossid_raster_workspace_bytes", 0, 1, 1), R("ossid_raster_workspace_bytes", 1, -1, 1),
                        R("ossid_raster_workspace_bytes", 1, 1, 0), R("ossid_raster_workspace_bytes", 1, 1, 257),
                        R("ossid_raster_color_workspace_bytes", 0, 1, 1, 4, 4), R("ossid_raster_color_workspace_bytes", 8, 12, 3, 0, 56),
                        R("ossid_raster_color_workspace_bytes", 8, 12, 257, 40, 56)]),
    Case("scene", ["ossid_scene_workspace_bytes"], SCENE_SHAPES, scene_need, scene_pred, scene_build,
         [R("ossid_scene_workspace_bytes", -1, 3, 40, 56), R("ossid_scene_workspace_bytes", 100, 0, 40, 56),
          R("ossid_scene_workspace_bytes", 100, 3, 0, 56)]),
    Case("cloud_weights", ["ossid_cloud_workspace_bytes"], CLOUD_SHAPES, cloud_need, cloud_pred, cloud_build,
         [R("ossid_cloud_workspace_bytes", 0), R("ossid_cloud_workspace_bytes", (1 << 22) + 1)]),
    Case("det_match", ["ossid_det_eval_workspace_bytes"], DET_SHAPES, det_need, det_pred, det_build,
         [R("ossid_det_eval_workspace_bytes", (1 << 22) + 1, 10, 3, 1), R("ossid_det_eval_workspace_bytes", 10, (1 << 20) + 1, 3, 1),
          R("ossid_det_eval_workspace_bytes", 10, 10, 0, 1), R("ossid_det_eval_workspace_bytes", 10, 10, 4097, 1),
          R("ossid_det_eval_workspace_bytes", 10, 10, 3, 17), R("ossid_det_eval_workspace_bytes", 10, 10, 3, 0)]),
    Case("features", ["ossid_feat_pyramid_bytes", "ossid_feat_detect_workspace_bytes", "ossid_feat_match_workspace_bytes"], FEAT_SHAPES,
         feat_need, feat_pred, feat_build,
         [R("ossid_feat_pyramid_bytes", 7, 97, 3), R("ossid_feat_pyramid_bytes", 65, 97, 0), R("ossid_feat_pyramid_bytes", 65, 97, 4),
          R("ossid_feat_match_workspace_bytes", 0), R("ossid_feat_match_workspace_bytes", 4097)]),
]

# Queried sizes at the shapes above, in bytes, as an MI355X build answered them when the table was written (a + marks a size
# that is not a multiple of 512; the few-channel, t9, group, stem and dense sizes depend on the device's resident workgroups):
#   conv_wgrad 958464 / 2654208 / 1140480+   conv_wgrad_group 1351936+   stem_conv_wgrad 1580544   dw_bwd_k 20736+
#   conv1x1_c1_bwd 144+ / 5160+   focal_smoothl1_loss 72+   wino 524288, pair 1048576   topk 28744+ / 29256+ / 36936+
#   nms 264+ / 1296+ / 139656+   detect_post 29192+ / 30736+ / 176776+   chan_op 192+ / 2304+   dense_fwd1_stats rows 7680,
#   counts 20+   dense_dgrad1_acc 5376+   dense_dgrad3_mask 12288   dw_add_stats 4224+   stem_pool_bwd 1152+
#   pn2_score 4171520+ / 10844928+   pn2_train 50977792 / 39291136+   pn2_train_linear_wgrad 256+ / 256+ / 4352+ / 510208+
#   ppf_refine grid 1025312+, workspace 2576+   raster 7776+ / 384+, colour 61536+ / 54144+   scene 62240+
#   cloud_weights 8208+ / 10760+   det_match 13544+ / 61696+   feat pyramid 217380+ / 21880+, detect 16958+ / 1688+, match 320+
