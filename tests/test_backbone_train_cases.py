"""CPU side of the image backbone's training tests: every case of tests/backbone_train_cases.py lands on the route of
ossid_conv_nhwc_fwd it is named for, by the restated route choice; the whole-backbone images give the maps they are chosen
for, and every entry point with a host-side size query accepts them. A later change to the routing that moves a case off
its edge fails here."""
from pathlib import Path

import torch

import backbone_train_cases as bc
import ref_densenet as rd

SRC = Path(__file__).resolve().parent.parent / "ossid_code_amd" / "csrc" / "conv.hip"


def test_the_restated_route_choice_is_the_sources():
    """The conditions the restatement copies, read off the source in their order: a change there has to come by here."""
    text = SRC.read_text()
    body = text[text.index("if (d->taps == 1) {"):text.index("if (d->taps == 4) {")]
    want = ["const long plain_wgs = (px + 63) / 64 * ((tiles + 3) / 4);",
            "if (tiles >= 4 && px >= 4096) return launch_conv<4, 1, 1, false, 2, 1, 64>",
            "if (plain_wgs < 160) return launch_conv<1, 4, 1, false, 8, 1, 256>",
            "if (tiles >= 4)",
            ": launch_conv<4, 1, 1, false, 1, 1, 16>",
            "if (tiles >= 2) return launch_conv<2, 1, 2, false, 2, 1, 16>",
            "return launch_conv<1, 1, 1, false, 2, 1, 16>"]
    assert want[0] in text
    pos = [body.index(w) for w in want[1:]]
    assert pos == sorted(pos)
    assert "a.n_cotiles = (Cout + 31) / 32" in text and "const long px = (long)B * H * W;" in text
    # the arm no case is named for: behind `tiles >= 4` only px < 4096 arrives
    assert "px >= 128L * 512 ? launch_conv<4, 1, 4, false, 2, 1, 16>" in body and 128 * 512 > 4096


def test_every_stage_case_lands_on_its_route():
    for cid, (kind, B, H, W, cin, cout, stride, fwd, dgrad) in bc.STAGES.items():
        px = B * H * W
        got = (bc.conv1x1_route(cout, px), bc.conv1x1_route(cin, px))
        print("%-18s %4d -> %4d at px %5d: forward %s, data gradient %s" % (cid, cin, cout, px, got[0], got[1]))
        assert got == (fwd, dgrad), cid
        assert cin % 16 == 0 and cout % 4 == 0 and (kind == "tail") == (stride == 0)
        assert kind == "tail" or (H >= 2 and W >= 2)
    routes = {r for c in bc.STAGES.values() for r in c[7:]}
    assert routes == {"4x64", "splitK256", "4x16", "2x16", "1x16"}


def test_the_named_pixel_counts_are_the_smallest():
    S = bc.STAGES
    px = lambda cid: S[cid][1] * S[cid][2] * S[cid][3]      # noqa: E731
    # 4x64 starts at exactly 4096 for four or more channel tiles, whatever plain_wgs says
    assert px("t1-px4096") == 4096 == bc.smallest_px(128, "4x64") == bc.smallest_px(256, "4x64")
    assert bc.conv1x1_route(128, 4095) == "splitK256" and bc.conv1x1_route(96, 1 << 15) != "4x64"
    assert px("t1-px4225-cin160") % 32 != 0 and S["t1-px4225-cin160"][4] % 64 == 32
    # transition2: under one 32-pixel tile, and a ragged 256-channel chunk
    assert px("t2-px30") == 30 < 32 and px("t2-px234-cin352") == 2 * 9 * 13 and 352 % 256 == 96
    # transition3: the first px at which 512 output channels leave split-K for 4x16, below 4096
    assert px("t3-px48") == 2 * 4 * 6
    assert px("t3-px2497") == 2497 == bc.smallest_px(512, "4x16") and bc.conv1x1_route(512, 2496) == "splitK256"
    assert bc.smallest_px(1024, "4x16") == 1217 and all(1217 % k for k in range(2, 35))      # (a prime: no B x H x W)
    # c1: the real map at batch 2, the smallest backbone's 3 x 5
    assert px("c1-px2262") == 2 * 29 * 39 == 2262 and px("c1-px15") == 15
    assert bc.smallest_px(640, "4x16") <= 2262 < 4096
    # two and one channel tile(s): split-K up to px = 10176, the 16-channel-chunk forms from 10177 on
    for cout, route in ((64, "2x16"), (32, "1x16")):
        assert bc.smallest_px(cout, route) == 10177 and bc.conv1x1_route(cout, 10176) == "splitK256"
    assert all(10177 % k for k in range(2, 101)) and 10178 == 2 * 7 * 727 and 10179 == 3 * 29 * 117
    assert px("tiles2-px33") == 33 and px("tiles1-px65") == 65 and px("tiles2-px10179") == px("tiles1-px10179") == 10179


def test_whole_backbone_maps():
    for cid, (B, H, W, gb, seed) in bc.IMAGES.items():
        assert bc.maps(H, W) == bc.MAPS[cid], cid
        assert gb in (1, B)
    m = bc.MAPS["B2-70x102"]
    assert m == [(35, 51), (18, 26), (9, 13), (4, 6), (3, 5)] and 2 * 3 * 5 == 30
    # pool0's last window is partial (odd stem map), AvgPool 2/2 drops a row and / or a column (odd block map)
    assert m[0][0] % 2 == 1 and m[0][1] % 2 == 1 and m[2][0] % 2 == 1 and m[2][1] % 2 == 1
    assert {gb == 1 and B > 1 for B, _, _, gb, _ in bc.IMAGES.values()} == {True, False}
    assert sum(gb == B for B, _, _, gb, _ in bc.IMAGES.values()) == 2
    # the maps are what torch computes
    x = torch.zeros(1, 1, 70, 102)
    x = torch.nn.functional.conv2d(x, torch.zeros(1, 1, 7, 7), stride=2, padding=3)
    assert tuple(x.shape[2:]) == m[0]
    x = torch.nn.functional.max_pool2d(x, 3, 2, 1)
    assert tuple(x.shape[2:]) == m[1]
    for stride, want in zip((2, 2, 1), m[2:]):
        x = torch.nn.functional.avg_pool2d(x, 2, stride)
        assert tuple(x.shape[2:]) == want


def test_every_entry_point_accepts_the_shapes(hiplib):
    """The host-side size queries answer with a positive count for every map of every case (0 = shape refused). None of
    the chosen sizes had to be replaced."""
    fn = hiplib.fn
    shapes = [(B, bc.MAPS[cid]) for cid, (B, _, _, _, _) in bc.IMAGES.items()]
    for B, m in shapes:
        assert fn("ossid_dw_add_stats_partials")(B, m[0][0], m[0][1], 64) > 0
        assert fn("ossid_stem_pool_bwd_partials")(B, m[0][0], m[0][1], 64) > 0
        for h, w in m[1:]:
            tiles = B * ((h + 3) // 4) * ((w + 7) // 8)
            assert 0 < fn("ossid_dense_dgrad3_mask_partials")(B, h, w) <= tiles
    for B, C, H, W, kb in bc.STEM_TAIL:
        assert fn("ossid_dw_add_stats_partials")(B, H, W, C) > 0 and fn("ossid_stem_pool_bwd_partials")(B, H, W, C) > 0
        assert kb in (1, B)
    assert fn("ossid_dw_add_stats_partials")(1, 5, 6, 48) == 0                  # (a refusal looks like this)


def test_seeded_backbone_is_reproducible_and_drawn_as_stated():
    a, b = bc.make_backbone(11), bc.make_backbone(11)
    for (n, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), n
    bns = [m for m in a.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) == 122
    for name in bc.NEGATIVE_GAMMA:
        w = a.get_submodule(name).weight.detach()
        assert float(w[3]) < -0.5 and int((w < 0).sum()) == 1
    assert a.get_submodule(rd.module_name("norm0")) is a.backdense_1[0]
    assert a.get_submodule(rd.module_name("transition2.norm")) is a.backdense_2[2].norm
    for m in bns:
        assert float(m.running_var.min()) >= 0.5 and float(m.running_mean.abs().max()) > 0.1


def test_float32_restatement_alone_stays_under_the_margin_cap():
    """Premise of the GPU test's decision check, at the committed seeds: float32 arithmetic alone (the restatement in
    float32 on the float64 pass's decisions) leaves at most 1e-3 of any layer's decisions within tau = 4 x its own forward
    error of the kink, and none outside tau on the other side."""
    worst = (0.0, "")
    for cid, (B, H, W, gb, seed) in bc.IMAGES.items():
        ife = bc.make_backbone(seed)
        image, g, gout = bc.backbone_inputs(cid)
        r64 = rd.backbone_train(ife, image, g, gout)
        r32 = rd.backbone_train(ife, image, g, gout, decisions=r64["decisions"], dtype=torch.float32)
        res = bc.decision_margins(r64, r32["pre"], r32["decisions"])
        total = inside = 0
        for name, (n, k, tau, wrong) in res.items():
            assert wrong == 0, (cid, name, wrong)
            assert k <= 1e-3 * n, (cid, name, k, n, tau)
            worst = max(worst, (k / n, "%s %s" % (cid, name)))
            total, inside = total + n, inside + k
        print("%-10s decisions %8d, inside tau %d" % (cid, total, inside))
    print("largest share of a layer inside tau: %.2e (%s)" % worst)
