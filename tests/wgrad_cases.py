"""The cases of tests/test_wgrad_routes.py (host) and tests/test_wgrad_routes_gpu.py: every form ossid_conv_wgrad and
ossid_conv_wgrad_group can send a weight gradient to -- csrc/wgrad_fc.hip, csrc/wgrad_t9.hip (t9 and t1), the seven tilings
of csrc/train.hip and its three slab reductions -- at the sizes where a form changes or a tile ends, with the two kinds of
data both files use and the float64 reference.

A case names the form it was chosen for (`family`, `variant`). The route itself is not restated here: expect_route asks
workspace_cases.wgrad_path / wgrad_variant, and the number of slabs comes from the library's own size query.

Data. "int": every tensor holds integers in [-3, 3] (scales nonzero). Each operand of a product is then an integer below
256 -- exact in bf16, the low parts of the split are zero -- and every partial sum stays below 2^24 (the host test asserts
it on the reference), so whatever the K-split and the order of the reduction, the float64 reference cast to f32 must come
out bit for bit. "normal": standard normal data, held element by element to

    |dw - ref| <= (2^-14 + N 2^-23) sum_p |x_p| |dy_p|        N = the summed pixels, batch * height * width

(the sum: the same convolution on absolute values, in float64). 2^-14 covers the three-product split -- each operand kept
to 2^-16 relative, the lo * lo product dropped -- and N 2^-23 the f32 accumulation. One dropped or doubled pixel is 1 / N of
the sum: orders of magnitude above the bound at every size here.

Nothing here touches the GPU at import."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

import workspace_cases as wc

_FIELDS = ("name", "B", "H", "W", "cin", "cout", "taps", "family", "variant", "pre", "in_extra", "dy_off", "dy_extra", "up",
           "misalign", "sweep", "dy_add")
Case = collections.namedtuple("Case", _FIELDS)
PRE = ("none", "relu", "affine")                               # the prologue: identity, BatchNorm affine + ReLU, affine only


def case(name, B, H, W, cin, cout, taps, family, variant, k=0, up=None, misalign=False, sweep=None, dy_add=False, strided=None):
    """k picks the prologue (k % 3) and, unless `strided` says, whether x is a channel prefix of a wider buffer and dy a
    channel slice at a nonzero offset (k % 2 == 0); both offsets keep 16-byte alignment."""
    strided = (k % 2 == 0) if strided is None else strided
    return Case(name, B, H, W, cin, cout, taps, family, variant, PRE[k % 3], 8 if strided else 0, 4 + 4 * (k % 3) if strided else 0,
                4 if strided else 0, up, misalign, sweep, dy_add)


def cid(c):
    return c.name


# ---- single problems (ossid_conv_wgrad) ----------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, taps, variant[, k of case()]): the tiled kernels' table. The variant is what wgrad_plan must say; the slab count is queried.
_TABLE = [
    (2, 9, 50, 260, 132, 9, 0),       # three 128-wide blocks of input channels, the last one 4 wide
    (1, 40, 60, 132, 132, 9, 0),      # enough work for a ragged slab count of the middle reduce class
    (2, 9, 50, 32, 100, 9, 0),
    (2, 9, 50, 32, 64, 9, 1),
    (2, 9, 50, 36, 96, 9, 1),         # Cout == 96: two 64-wide blocks, the second half empty
    (2, 9, 50, 68, 36, 9, 1),
    (2, 9, 50, 96, 32, 9, 2),
    (2, 9, 50, 160, 16, 9, 2),
    (1, 2, 3, 132, 12, 9, 2),
    (2, 9, 13, 260, 68, 1, 3, 8),
    (1, 1, 31, 68, 132, 1, 3),        # one ragged chunk of the flattened pixel row
    (2, 9, 13, 132, 60, 1, 4),
    (1, 1, 33, 36, 64, 1, 4),
    (1, 1, 1, 4, 4, 1, 4),
    (8, 30, 40, 64, 16, 1, 4),        # many slabs: the widest reduce class
    (1, 1, 1, 4, 4, 9, 5),            # all halo
    (2, 9, 70, 32, 32, 9, 5),
    (2, 20, 130, 16, 16, 9, 5),       # KT is raised to 64 after the chunks per row were counted: 3 chunks over 130
    (1, 3, 5, 64, 16, 9, 6),
    (2, 9, 35, 48, 32, 9, 6),
    (2, 9, 70, 64, 16, 9, 6),
    (4, 40, 70, 48, 16, 9, 6),
]
def _kname(taps):
    return "3x3" if taps == 9 else "1x1"


TABLE_CASES = [case("tab-%dx%dx%d-%dto%d-%s" % (s[:5] + (_kname(s[5]),)), *s[:6], "generic", s[6], k=s[7] if len(s) > 7 else i)
               for i, s in enumerate(_TABLE)]

# one 3x3 shape per swept variant, run over W = the variant's chunk length - 1, + 0, + 1 and H = 1, 2 (the top and bottom taps
# all halo / half halo). W is filled in by resolve(): the chunk length depends on the build.
SWEEP_SHAPES = {0: (36, 132), 5: (16, 16), 6: (48, 32)}
SWEEP_CASES = [case("sweep-v%d-W%+d-H%d" % (v, dw, H), 2, H, None, ci, co, 9, "generic", v, k=3 * v + dw + H, sweep=dw)
               for v, (ci, co) in sorted(SWEEP_SHAPES.items()) for dw in (-1, 0, 1) for H in (1, 2)]


def chunk_len(variant, sb):
    """The most pixels of a row a chunk of the 3x3 variants holds (train.hip wgrad_plan: ktmax), by build."""
    return {5: 64 if sb else 48, 6: 32 if sb else 40}.get(variant, 48)


# the tiled kernels' nearest-neighbour up-sampling prologue: integer and non-integer ratios
UP_CASES = [case("up-%dto%d-%dx%d" % (ci, co, H, W), 2, H, W, ci, co, 9, "generic", v, k=i + j, up=(7, 9))
            for i, (ci, co, v) in enumerate(((16, 16, 5), (48, 32, 6), (96, 32, 2), (32, 64, 1), (32, 128, 0)))
            for j, (H, W) in enumerate(((14, 18), (15, 20)))]

# a workspace 4 bytes past a 16-byte boundary sends any problem to the tiled kernels: the few-channel and t9 shapes too
MISALIGNED_CASES = [case("misaligned-%dto%d" % (ci, co), 2, 9, 50, ci, co, 9, "generic", v, k=i + 1, misalign=True)
                    for i, (ci, co, v) in enumerate(((32, 16, 5), (64, 32, 6), (128, 32, 2)))]

# csrc/wgrad_t9.hip through the single entry: its 4 x 16 pixel tiles at their edges, ragged last channel blocks, both classes;
# and one problem of 50 jobs (above a launch's 48), cut over two launches
T9_CASES = [case("t9-%dto%d-%dx%dx%d" % (ci, co, 1 + (H + W) % 2, H, W), 1 + (H + W) % 2, H, W, ci, co, 9, "t9", 2 if co <= 32 else 1 if
                 (co <= 64 or co == 96) else 0, k=i + 3 * j + l)
            for i, (ci, co) in enumerate(((128, 32), (128, 36), (256, 60), (128, 64), (256, 68), (256, 100)))
            for j, H in enumerate((1, 3, 4, 5)) for l, W in enumerate((15, 16, 17))]
T9_CASES.append(case("t9-256to1600-1x4x16", 1, 4, 16, 256, 1600, 9, "t9", 0, k=1))

# csrc/wgrad_fc.hip: plain and behind an integer and a non-integer up-sampling
FEWCH_CASES = [case("fewch-%dto%d-%dx%dx%d" % (ci, co, B, H, W), B, H, W, ci, co, 9, "fewch", 5 if ci == 32 else 6, k=i + j)
               for i, (ci, co) in enumerate(((32, 16), (64, 32))) for j, (B, H, W) in enumerate(((1, 1, 1), (1, 4, 32), (1, 5, 33), (2, 3, 31)))]
FEWCH_CASES += [case("fewch-up-%dto%d-%dx%d" % (ci, co, H, W), 2, H, W, ci, co, 9, "fewch", 5 if ci == 32 else 6, k=i + j + 1, up=(2, 16))
                for i, (ci, co) in enumerate(((32, 16), (64, 32))) for j, (H, W) in enumerate(((4, 32), (5, 33)))]

SINGLE_CASES = TABLE_CASES + SWEEP_CASES + UP_CASES + MISALIGNED_CASES + T9_CASES + FEWCH_CASES
TILED_CASES = [c for c in SINGLE_CASES if c.family == "generic"]


def split_bf16(lib):
    return bool(lib.fn("ossid_conv_wgrad_split_bf16")())


def resolve(lib, c):
    """The case with the row length of a sweep filled in for this build."""
    return c if c.sweep is None else c._replace(W=chunk_len(c.variant, split_bf16(lib)) + c.sweep)


def expect_route(lib, c):
    """(family, variant or None) the entry must take for the single problem `c`: workspace_cases' restatement, and the rule
    that a misaligned workspace leaves only the tiled kernels. An all-f32 build has no t9: those cases stay tiled."""
    path = "generic" if c.misalign else wc.wgrad_path(lib, c.cin, c.cout, c.taps)
    return path, (wc.wgrad_variant(c.cin, c.cout, c.taps)[0] if path == "generic" else None)


def slab_count(lib, c):
    """How many slabs the tiled kernels write for `c`, from the library's size query. Only where the query is the tiled
    kernels' own need (a few-channel or t9 shape answers the larger of two needs)."""
    assert wc.wgrad_path(lib, c.cin, c.cout, c.taps) == "generic", c
    need = int(lib.fn("ossid_conv_wgrad_workspace_bytes")(c.B, c.H, c.W, c.cin, c.cout, c.taps))
    unit = c.taps * c.cout * c.cin * 4
    assert need > 0 and need % unit == 0, (c, need)
    return need // unit


def reduce_class(slabs):
    """PARTS of the wgrad_reduce2_kernel that sums `slabs` slabs."""
    return 1 if slabs <= 16 else 4 if slabs <= 128 else 32


# ---- data and reference ----------------------------------------------------------------------------------------------------------
def _seed(c, kind):
    return zlib.crc32(("%s %s %s" % (c.name, c.W, kind)).encode())


def _draw(g, kind, *shape, nonzero=False):
    if kind == "normal":
        return torch.randn(*shape, generator=g)
    if nonzero:
        return (torch.randint(1, 4, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()
    return torch.randint(-3, 4, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def inputs(c, kind):
    """CPU tensors of the (resolved) case: x [B, cin + in_extra, Hs, Ws] (the problem reads the first cin channels), dy
    [B, dy_off + cout + dy_extra, H, W] (channels dy_off .. dy_off + cout), the prologue rows ps, pt (None: no prologue), dw0
    (integers: what `accumulate` adds to) and, for dy_add cases, add (like dy), add_scale, add_shift [cout]."""
    g = torch.Generator().manual_seed(_seed(c, kind))
    Hs, Ws = c.up or (c.H, c.W)
    k = 3 if c.taps == 9 else 1
    d = {"x": _draw(g, kind, c.B, c.cin + c.in_extra, Hs, Ws), "dy": _draw(g, kind, c.B, c.dy_off + c.cout + c.dy_extra, c.H, c.W),
         "ps": None, "pt": None, "add": None}
    if c.pre != "none":
        d["ps"], d["pt"] = _draw(g, kind, c.cin, nonzero=True), _draw(g, kind, c.cin)
    d["dw0"] = _draw(g, "int", c.cout, c.cin, k, k)
    if c.dy_add:
        d["add"] = _draw(g, kind, c.B, c.dy_off + c.cout + c.dy_extra, c.H, c.W)
        d["add_scale"], d["add_shift"] = _draw(g, kind, c.cout, nonzero=True), _draw(g, kind, c.cout)
    return d


def operands(c, d):
    """The two float64 operands of the gradient: P(x) [B, cin, H, W] after the prologue and the up-sampling, and the output
    gradient [B, cout, H, W] (with dy_add's term)."""
    xin = d["x"][:, :c.cin].double()
    if c.pre != "none":
        xin = xin * d["ps"].double().view(1, -1, 1, 1) + d["pt"].double().view(1, -1, 1, 1)
        if c.pre == "relu":
            xin = F.relu(xin)
    if c.up is not None:
        xin = F.interpolate(xin, size=(c.H, c.W), mode="nearest")
    sl = slice(c.dy_off, c.dy_off + c.cout)
    dy = d["dy"][:, sl].double()
    if c.dy_add:
        dy = dy + d["add_scale"].double().view(1, -1, 1, 1) * d["add"][:, sl].double() + d["add_shift"].double().view(1, -1, 1, 1)
    return xin, dy


def _grad(xin, dy, taps):
    k = 3 if taps == 9 else 1
    w = torch.zeros(dy.shape[1], xin.shape[1], k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, w, padding=k // 2).backward(dy)
    return w.grad


@functools.lru_cache(maxsize=None)
def reference(c, kind):
    """(ref, mag): the float64 weight gradient of the case and the same sum over absolute values (the bound's sum term)."""
    xin, dy = operands(c, inputs(c, kind))
    return _grad(xin, dy, c.taps), _grad(xin.abs(), dy.abs(), c.taps)


def pixels(c):
    return c.B * c.H * c.W


def bound(c, mag):
    return (2.0 ** -14 + pixels(c) * 2.0 ** -23) * mag


# ---- groups (ossid_conv_wgrad_group) -------------------------------------------------------------------------------------------
def _gcase(tag, i, B, H, W, cin, cout, taps, family, variant, dy_add=False):
    return case("%s-%d-%dto%d-%s-%dx%dx%d" % (tag, i, cin, cout, _kname(taps), B, H, W), B, H, W, cin, cout, taps, family, variant, k=i, dy_add=dy_add)


# all seven tilings at two geometries; none takeable by t9 or t1 (64 -> 32, the few-channel form's shape, stays tiled here:
# the group entry has no few-channel route)
_SEVEN = ((260, 132, 9, 0), (32, 100, 9, 0), (32, 64, 9, 1), (36, 96, 9, 1), (96, 32, 9, 2), (132, 12, 9, 2), (260, 68, 1, 3),
          (68, 132, 1, 3), (132, 60, 1, 4), (36, 64, 1, 4), (32, 32, 9, 5), (16, 16, 9, 5), (64, 32, 9, 6), (48, 16, 9, 6))
GROUP_SEVEN = [_gcase("seven", i, *((1, 5, 9) if i % 2 == 0 else (2, 3, 17)), ci, co, t, "generic", v)
               for i, (ci, co, t, v) in enumerate(_SEVEN)]
# 25 problems of variant 5 (a launch takes 24: the piece splits in two) and 2 of variant 4
GROUP_CUT = [_gcase("cut", i, 1, 3, 5, 4 + 4 * (i % 4), 4 + 4 * ((i // 4) % 4), 9, "generic", 5) for i in range(25)] + \
            [_gcase("cut", 25, 1, 3, 5, 36, 64, 1, "generic", 4), _gcase("cut", 26, 1, 3, 5, 132, 60, 1, "generic", 4)]
# one t9 problem of 50 jobs (a launch takes 48), then one of the other class, which runs in another round
GROUP_T9 = [_gcase("t9", 0, 1, 4, 16, 640, 640, 9, "t9", 0), _gcase("t9", 1, 1, 4, 16, 128, 32, 9, "t9", 2)]
# t1 jobs 32, 256, 32 (of 288) and 32 (of 544) channels wide, at a pixel count that is no multiple of its 64-pixel stage
GROUP_T1 = [_gcase("t1", i, 1, 5, 13, ci, 128, 1, "t1", 3, dy_add=(i == 2)) for i, ci in enumerate((32, 256, 288, 544))]
GROUPS = {"seven": GROUP_SEVEN, "cut": GROUP_CUT, "t9": GROUP_T9, "t1": GROUP_T1}
GROUP_MAX, T9_MAX, T1_PXS = 24, 48, 64                          # train.hip OSSID_WGRAD_GROUP_MAX; wgrad_t9.hip


def expect_group_route(lib, c):
    """The family a problem of a group goes to. The group entry knows no few-channel form and no limit on t9's input
    channels; t1 (1x1, c -> 128, c in 32s) is reached through it alone. Both exist on split-bf16 builds only."""
    if split_bf16(lib) and c.taps == 9 and c.cin % 128 == 0 and wc.wgrad_path(lib, 128, c.cout, 9) == "t9":
        return "t9"
    if split_bf16(lib) and c.taps == 1 and c.cout == 128 and c.cin % 32 == 0:
        return "t1"
    return "generic"


def group_bytes(lib, cases):
    arr = (lib.WgradDesc * len(cases))()
    for d, c in zip(arr, cases):
        d.batch, d.height, d.width, d.cin, d.cout, d.taps = c.B, c.H, c.W, c.cin, c.cout, c.taps
    return int(lib.fn("ossid_conv_wgrad_group_workspace_bytes")(arr, len(cases)))
