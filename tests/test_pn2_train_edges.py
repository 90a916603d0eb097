"""CPU side of the scorer's training-kernel edge tests (SPEC.md 12): every case of tests/pn2_train_cases.py lands on the
edge it is named for, by the restated chunk arithmetic of csrc/pn2_train.hip (wgrad_split, stat_chunks) and, for the
whole-model shapes, on the restatement's own ball lists. A later change to the chunking that moves a case off its edge fails
here. Prints the premise figures."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import pn2_train_cases as pc
import ref_pn2_train as rt
import test_pn2_train_gpu as tg

SRC = Path(__file__).resolve().parent.parent / "ossid_code_amd" / "csrc" / "pn2_train.hip"


def test_the_restated_chunk_arithmetic_is_the_sources():
    """The constants the restatement copies, read off the source: a change there has to come by here."""
    text = SRC.read_text()
    body = text[text.index("void wgrad_split("):text.index("size_t wgrad_ws_bytes(")]
    assert "(R + 255) / 256" in body and "ch < 512" in body and "(ch + 15) / 16 * 16" in body
    body = text[text.index("void stat_chunks("):text.index("int bn_stats(")]
    assert "(R + 255) / 256" in body and "n > STAT_MAX_CHUNKS" in body and "(R + n - 1) / n" in body
    assert int(re.search(r"STAT_MAX_CHUNKS = (\d+);", text).group(1)) == pc.STAT_MAX_CHUNKS
    assert "__shared__ float As[16][65], Bs[16][65];" in text and "constexpr int NACC = 8;" in text


def test_weight_gradient_split_table():
    for R, want in pc.WGRAD_TABLE.items():
        assert pc.wgrad_split(R) == want, (R, pc.wgrad_split(R))
    assert set(pc.WGRAD_TABLE) <= set(pc.WGRAD_R)
    for R in pc.WGRAD_R:
        print("R %6d: chunk %d, %d splits, %d rows in the last" % ((R,) + pc.wgrad_split(R)))
    assert pc.wgrad_split(511)[:2] == (512, 1) and pc.wgrad_split(512) == (512, 1, 512)          # either side of one split
    assert pc.wgrad_split(131072) == (512, 256, 512)                                                # the last R with chunk 512
    # what each is for: the shortest tail, one slice in the tail, a tail that ends inside a slice under a grown chunk
    assert pc.wgrad_split(513)[2] == 1 and pc.wgrad_split(1040)[2] == 16 and pc.gemm_slices(pc.wgrad_split(1040)[2]) == (1, 16, 1)
    ch, _, tail = pc.wgrad_split(131073)
    assert ch > 512 and ch % 16 == 0 and tail % 16 != 0 and pc.gemm_slices(tail) == (9, 1, 8)
    assert 544 == 17 * 32 and 133120 == 2080 * 64
    assert 9 * max(pc.WGRAD_R) < 2 ** 24                                                            # every sum exact in float32
    # the tested shapes before this table: a single split, or whole chunks only
    for R in (20480, 10240, 8192, 160, 128, 5):
        ch, splits, tail = pc.wgrad_split(R)
        assert ch == 512 and (splits == 1 or tail == ch), R
    for R in pc.WGRAD_REAL_R:
        assert pc.wgrad_split(R)[1] > 1 and pc.wgrad_split(R)[2] < pc.wgrad_split(R)[0]


def test_statistics_chunk_table():
    for R, (n, rpc, last) in pc.STATS_TABLE.items():
        got = pc.stat_chunks(R)
        assert got[:2] == (n, rpc) and (last is None or got[2] == last), (R, got)
    for R in pc.STATS_R:
        print("R %6d: %d chunks of %d rows, %d in the last" % ((R,) + pc.stat_chunks(R)))
    assert pc.stat_chunks(513)[1] % 4 != 0 and pc.stat_chunks(544)[1] % 4 != 0                       # not a multiple of the 4 row lanes
    assert pc.stat_chunks(544) == (3, 182, 180)
    assert pc.stat_chunks(65536) == (256, 256, 256)                                                  # the cap, no remainder
    assert pc.stat_chunks(65537)[0] == pc.STAT_MAX_CHUNKS and pc.stat_chunks(70001)[0] == pc.STAT_MAX_CHUNKS
    for R in (1, 2, 3, 5, 255):
        assert pc.stat_chunks(R) == (1, R, R)
    assert pc.stat_chunks(257)[0] == 2 and pc.stat_chunks(257)[2] < pc.stat_chunks(257)[1]
    assert {r for r, _ in pc.STATS_CASES} == set(pc.STATS_R) and {c for _, c in pc.STATS_CASES} == set(pc.STATS_C)
    assert max(r * c for r, c in pc.STATS_CASES) <= 133120 * 64
    assert 64 * max(pc.STATS_R) < 2 ** 53
    # the tested shapes before this table divide evenly
    for R in (6144, 20480, 10240, 8192, 160, 128, 5, 4):
        n, rpc, last = pc.stat_chunks(R)
        assert last == rpc, R


def test_gemm_grid_takes_every_value_in_every_role():
    grid = pc.GEMM_GRID
    assert {t[0] for t in grid} >= set(pc.GEMM_R) and {t[1] for t in grid} >= set(pc.GEMM_C) and {t[2] for t in grid} >= set(pc.GEMM_KR)
    assert (1, 1, 1) in grid and (65, 65, 65) in grid and 24 <= len(grid) <= 48 and len(set(grid)) == len(grid)
    assert 9 * max(max(t) for t in grid) < 2 ** 24
    for kr in pc.GEMM_KR:
        kp = pc.kp_variants(kr)
        assert kr in kp and (kr + 7) // 8 * 8 in kp and kr + 9 in kp
    # K one either side of a 16-deep slice and of the 128 that fill the 8 accumulators once
    assert [pc.gemm_slices(k) for k in (15, 16, 17)] == [(1, 15, 1), (1, 16, 1), (2, 1, 2)]
    assert [pc.gemm_slices(k) for k in (127, 128, 129)] == [(8, 15, 8), (8, 16, 8), (9, 1, 8)]
    for t in pc.GEMM_REAL:
        assert any(v % 16 for v in t) and t[0] in pc.GEMM_R and t[1] in pc.GEMM_C + (65,) and t[2] in pc.GEMM_KR
    assert {t[2] for t in pc.GEMM_REAL} >= {1, 7, 17, 127, 129, 131, 259, 1024}


def test_exact_inputs_and_references():
    X, W, dZ = pc.gemm_operands(33, 31, 17)
    for t in (X, W, dZ):
        assert t.dtype == torch.float32 and torch.equal(t, t.round()) and float(t.abs().max()) == 3
    assert torch.equal(pc.exact(X, W.t()), (X.double() @ W.double().t()).float())
    p = pc.padded(X, 26, float("nan"))
    assert torch.equal(p[:, :17], X) and torch.isnan(p[:, 17:]).all()
    z = pc.stats_input(544, 65)
    assert float(z.abs().max()) == 8 and torch.equal(z, z.round())
    mean, rstd, var = pc.stats_expected(z)
    assert mean.dtype == np.float32 and np.allclose(var, z.double().var(0, unbiased=False).numpy(), rtol=1e-6)
    assert np.allclose(rstd, 1 / np.sqrt(var.astype(np.float64) + 1e-5), rtol=1e-6)
    one = pc.stats_expected(pc.stats_input(1, 64))
    assert (one[2] == 0).all() and np.allclose(one[1], 1e5 ** 0.5, rtol=1e-6)                          # one row: the eps alone


def test_pool_cases_hold_their_groups():
    """G * C on both sides of the 256-thread block, and the hand-made groups are what they are named."""
    sizes = [G * C for G, S, C in pc.POOL_CASES]
    assert min(sizes) < 256 < max(sizes) and any(s % 256 for s in sizes if s > 256)
    seen = set()
    for G, S, C in pc.POOL_CASES:
        Z, mean, rstd, gamma, beta, made = pc.pool_inputs(G, S, C)
        a, best, arg = pc.pool_expected(Z, mean, rstd, gamma, beta)
        assert a.dtype == torch.float32
        g = made["negative"]
        assert (a[g] == 0).all() and (arg[g] == 0).all()
        if "repeated" in made:
            g = made["repeated"]
            assert torch.equal(a[g, 0], a[g, S - 1]) and (a[g, 0] == best[g]).all() and (best[g] > 0).all() and (arg[g] == 0).all()
        if "last" in made:
            g = made["last"]
            assert (a[g, :S - 1] == 0).all() and (a[g, S - 1] > 0).all() and (arg[g] == S - 1).all()
        seen |= set(made)
    assert seen == {"negative", "repeated", "last"}


def test_ungroup_cases_hold_their_patterns():
    cs = pc.UNGROUP_CASES
    assert {c[2] for c in cs} == set(pc.UNGROUP_N) and {c[1] for c in cs} == set(pc.UNGROUP_E)
    assert {c[3] for c in cs} == set(pc.UNGROUP_CF) and {c[0] for c in cs} == {1, 3}
    empty_seen = False
    for B, E, n, Cf, kind in cs:
        idx, dG = pc.ungroup_inputs(B, E, n, Cf, kind)
        assert idx.shape == (B, E) and int(idx.min()) >= 0 and int(idx.max()) < n and torch.equal(dG, dG.round())
        want = pc.ungroup_expected(idx, dG, n)
        assert torch.equal(want.sum(1), dG.sum(1))
        if kind == "equal":
            assert (idx == idx[:, :1]).all()
        elif kind == "perm":
            assert all(sorted(idx[b].tolist()) == list(range(n)) for b in range(B))
        untouched = torch.ones(B, n, dtype=torch.bool).scatter_(1, idx, False)
        empty_seen = empty_seen or bool(untouched.any())
        assert (want[untouched] == 0).all()
    assert empty_seen and {"equal", "perm", "random"} == {c[4] for c in cs}
    assert any(c[4] == "equal" and c[1] > 64 for c in cs)              # one target takes more rows than one scan of the wave


@pytest.fixture(scope="module")
def restated():
    """Per whole-model case: the inputs, the sampling and the float64 / float32 restatements with free decisions."""
    out = {}
    for name, (B, M, np1, np2) in pc.WHOLE.items():
        x, idx = pc.whole_inputs(name)
        cpu = tg._model(np1, np2, 7)
        keep = (torch.rand(B, 256, generator=torch.Generator().manual_seed(11)) >= tg.P_DROP).to(torch.uint8)
        rec = {}
        for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
            with torch.no_grad():
                _, rec[tag] = rt.forward(rt.params_of(cpu, dtype), x, idx, keep, tg.P_DROP)
        out[name] = (x, idx, rec)
    return out


def test_whole_model_shapes_reach_their_chunks():
    B, M, np1, np2 = pc.WHOLE["E1"]
    assert B == 2 and M == np1 == np2 == 32
    B, M, np1, np2 = pc.WHOLE["E2"]
    assert B * np2 == 544 and pc.stat_chunks(544) == (3, 182, 180) and pc.wgrad_split(544) == (512, 2, 32)
    B, M, np1, np2 = pc.WHOLE["E3"]
    assert (np1, np2) == (512, 128) and B * np1 * 64 == 65536
    assert pc.wgrad_split(65536)[1] == 128 and pc.stat_chunks(65536)[0] == 256


def test_whole_model_inputs_mix_padded_and_truncated_balls(restated):
    """E3 has balls with fewer and with more than 64 hits at both levels, E2 at the first; E1 takes every point in both
    samplings."""
    got = {}
    for name in pc.WHOLE:
        x, idx, _ = restated[name]
        c1, c2 = pc.ball_counts(x, idx)
        got[name] = [(int((c < 64).sum()), int((c > 64).sum()), len(c)) for c in (c1, c2)]
        print(name, "balls with fewer / more than 64 hits: SA1 %d / %d of %d, SA2 %d / %d of %d" % (got[name][0] + got[name][1]))
    assert all(min(short, over) >= 10 for short, over, _ in got["E3"])
    assert min(got["E2"][0][:2]) >= 10
    x, idx, _ = restated["E1"]
    assert all(sorted(idx[k][b].tolist()) == list(range(32)) for k in ("fps1", "fps2") for b in range(2))
    # a ball over its 64 is cut to the first 64 hits, a short one repeats its first hit
    x, idx, _ = restated["E3"]
    c1, _ = pc.ball_counts(x, idx)
    ball = idx["ball1"].reshape(-1, 64)
    short = c1 < 64
    assert (ball[short][:, -1] == ball[short][:, 0]).all() and (ball[~short][:, 1:] > ball[~short][:, :-1]).all()


def test_the_inputs_leave_room_for_the_decision_caps(restated):
    """The caps of test_decisions_and_scores are conditions on the implementation: the float32 restatement itself meets
    them on these inputs (measured here: 0 of 3.3 M decisions differ at E1, 4 of 36.9 M at E2, 3 of 25.8 M at E3)."""
    for name in pc.WHOLE:
        _, _, rec = restated[name]
        e = max(float((a.double() - b).abs().max()) for a, b in zip(rec["32"]["y"], rec["64"]["y"]))
        total, differ, worst = pc.decisions_that_differ(rec["32"], rec["64"])
        print("%s: e_fwd %.3g, %d of %d decisions differ, worst margin %.3g (cap %.3g)" % (name, e, differ, total, worst, 16 * e))
        assert differ <= 1e-5 * total and worst <= 16 * e


def test_constant_input_has_no_variance_anywhere():
    B, M, np1, np2 = pc.WHOLE["E1"]
    x = pc.constant_input(B, M)
    assert (x == x[0, 0]).all() and float((x[0, 0, :3] ** 2).sum()) > 1e-3               # not one of the points FPS skips
    idx = rt.sample(x, np1, np2)
    assert int(idx["fps1"].max()) == 0 and int(idx["fps2"].max()) == 0                   # all distances tie: the first index
    cpu = tg._model(np1, np2, 7)
    with torch.no_grad():
        _, rec = rt.forward(rt.params_of(cpu, torch.float64), x, idx, torch.ones(B, 256), 0.5)
    assert all(float(v.max()) <= 1e-20 for v in rec["var"])


def test_workspace_table_has_the_ragged_split_and_the_grown_chunk():
    import workspace_cases as wc
    rows = {s[0] for s in wc.PN2W_SHAPES}
    assert {513, 131073} <= rows
