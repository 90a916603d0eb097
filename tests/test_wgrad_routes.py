"""The host side of tests/test_wgrad_routes_gpu.py (no device needed: the size queries of the tiled kernels are host functions):
every case of tests/wgrad_cases.py reaches the form it was chosen for, the table as a whole covers the seven tilings and
the three slab reductions with their ragged tails, the integer data keeps every partial sum exact in f32, and the float64
reference is the sum the header states."""
import pytest
import torch

import wgrad_cases as wg
import workspace_cases as wc


def _tiled_slabs(lib):
    out = []
    for c in wg.TILED_CASES:
        c = wg.resolve(lib, c)
        if wc.wgrad_path(lib, c.cin, c.cout, c.taps) == "generic":      # (the misaligned cases' shapes answer for two families)
            out.append((c, wg.slab_count(lib, c)))
    return out


@pytest.mark.parametrize("c", wg.SINGLE_CASES, ids=wg.cid)
def test_every_single_case_reaches_the_form_it_was_chosen_for(hiplib, c):
    c = wg.resolve(hiplib, c)
    family, variant = wg.expect_route(hiplib, c)
    want = "generic" if (c.family == "t9" and not wg.split_bf16(hiplib)) else c.family
    assert family == want, (c.name, family)
    if family == "generic":
        assert variant == c.variant, (c.name, variant)
    need = int(hiplib.fn("ossid_conv_wgrad_workspace_bytes")(c.B, c.H, c.W, c.cin, c.cout, c.taps))
    assert need > 0
    if wc.wgrad_path(hiplib, c.cin, c.cout, c.taps) == "generic":
        slabs = wg.slab_count(hiplib, c)
        assert slabs >= 1 and slabs % wc.wgrad_variant(c.cin, c.cout, c.taps)[1] == 0, (c.name, slabs)
        print(c.name, "variant", variant, "slabs", slabs, "reduce class", wg.reduce_class(slabs))
    assert c.in_extra % 4 == 0 and c.dy_off % 4 == 0 and c.dy_extra % 4 == 0                 # 16-byte alignment of x and dy kept


def test_the_table_covers_every_tiling_and_every_reduction_with_ragged_tails(hiplib):
    """A failure here means "pick another shape" (the K-split comes from a cost model that may be retuned), not "the kernel is
    wrong"."""
    seen = _tiled_slabs(hiplib)
    assert {c.variant for c, _ in seen} == set(range(7))
    classes = {wg.reduce_class(s) for _, s in seen}
    assert classes == {1, 4, 32}, classes
    assert any(wg.reduce_class(s) == 4 and s % 4 for _, s in seen), "no ragged slab count in the 4-part reduction"
    assert any(wg.reduce_class(s) == 32 and s % 256 for _, s in seen), "no ragged slab count in the 32-part reduction"
    # the up-sampling prologue and the misaligned-workspace fallback run on the tiled kernels
    assert {c.variant for c in wg.UP_CASES} == {0, 1, 2, 5, 6} and all(wg.expect_route(hiplib, c)[0] == "generic" for c in wg.UP_CASES)
    assert [wc.wgrad_path(hiplib, c.cin, c.cout, c.taps) for c in wg.MISALIGNED_CASES] == \
        ["fewch", "fewch", "t9" if wg.split_bf16(hiplib) else "generic"]
    assert all(wg.expect_route(hiplib, c)[0] == "generic" for c in wg.MISALIGNED_CASES)
    # per tiling: x as a channel prefix and dy as a channel slice at a nonzero offset; a ReLU and an affine-only prologue
    for v in range(7):
        mine = [c for c in wg.TILED_CASES if c.variant == v]
        assert any(c.in_extra and c.dy_off for c in mine), v
        assert {"relu", "affine"} <= {c.pre for c in mine}, v
    # the row-length sweep stands at the build's chunk lengths
    sb = wg.split_bf16(hiplib)
    for v in (0, 5, 6):
        ws = sorted({wg.resolve(hiplib, c).W for c in wg.SWEEP_CASES if c.variant == v})
        assert ws == [wg.chunk_len(v, sb) + d for d in (-1, 0, 1)], (v, ws)
        assert {c.H for c in wg.SWEEP_CASES if c.variant == v} == {1, 2}


def test_the_groups_hold_the_cuts_they_were_built_for(hiplib):
    sb = wg.split_bf16(hiplib)
    for name, cases in wg.GROUPS.items():
        assert wg.group_bytes(hiplib, cases) > 0, name
        assert len({c.name for c in cases}) == len(cases) <= 2 * wg.GROUP_MAX
    seven = wg.GROUP_SEVEN
    assert all(wg.expect_group_route(hiplib, c) == "generic" and wc.wgrad_path(hiplib, c.cin, c.cout, c.taps) != "t9" for c in seven)
    assert any(wc.wgrad_path(hiplib, c.cin, c.cout, c.taps) == "fewch" for c in seven)        # tiled here all the same
    for geo in ((1, 5, 9), (2, 3, 17)):
        assert {c.variant for c in seven if (c.B, c.H, c.W) == geo} == set(range(7)), geo
    assert all(wc.wgrad_variant(c.cin, c.cout, c.taps)[0] == c.variant for c in seven + wg.GROUP_CUT)
    assert sum(c.variant == 5 for c in wg.GROUP_CUT) == wg.GROUP_MAX + 1 and sum(c.variant == 4 for c in wg.GROUP_CUT) == 2
    if not sb:
        return
    big, small = wg.GROUP_T9
    assert [wg.expect_group_route(hiplib, c) for c in wg.GROUP_T9] == ["t9", "t9"]
    assert (big.cout // 64) * (big.cin // 128) > wg.T9_MAX and (big.cout >= 64) != (small.cout >= 64)
    assert (big.B, big.H, big.W) == (small.B, small.H, small.W)
    assert all(wg.expect_group_route(hiplib, c) == "t1" for c in wg.GROUP_T1)
    assert wg.pixels(wg.GROUP_T1[0]) % wg.T1_PXS != 0 and sum(c.dy_add for c in wg.GROUP_T1) == 1
    assert {c.cin % 256 for c in wg.GROUP_T1} == {32, 0}


def _direct(c, xin, dy):
    """dw[co][ci][ky][kx] = sum_{b,y,x} dy[b][co][y][x] P(x)[b][ci][y+ky-1][x+kx-1], written out."""
    k = 3 if c.taps == 9 else 1
    xp = torch.nn.functional.pad(xin, (k // 2,) * 4)
    out = torch.zeros(c.cout, c.cin, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            out[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", dy, xp[:, :, ky:ky + c.H, kx:kx + c.W])
    return out


@pytest.mark.parametrize("c", wg.SINGLE_CASES + [c for cases in wg.GROUPS.values() for c in cases], ids=wg.cid)
def test_integer_data_is_exact_in_f32_and_the_reference_is_the_stated_sum(hiplib, c):
    c = wg.resolve(hiplib, c)
    d = wg.inputs(c, "int")
    for key in ("x", "dy", "ps", "pt", "dw0", "add"):
        if d[key] is not None:
            assert float(d[key].abs().max()) <= 3 and torch.equal(d[key], d[key].round())
    assert d["ps"] is None or float(d["ps"].abs().min()) >= 1
    xin, dy = wg.operands(c, d)
    assert float(xin.abs().max()) < 256 and float(dy.abs().max()) < 256          # exact in bf16: the low parts are zero
    ref, mag = wg.reference(c, "int")
    # every partial sum, in any order, is bounded by the sum of the absolute products (+ what `accumulate` adds to)
    assert float(mag.max()) + 3 < 2 ** 24
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
    assert (ref.abs() <= mag).all()
    if wg.pixels(c) * c.cin * c.cout <= 1 << 24:                                  # the reference against the sum written out
        assert torch.equal(_direct(c, xin, dy), ref)
        xn, dyn = wg.operands(c, wg.inputs(c, "normal"))
        want = _direct(c, xn, dyn)
        got, magn = wg.reference(c, "normal")
        assert float((got - want).abs().max()) <= 1e-12 * float(magn.max())
