"""GPU tests (pytest -m gpu) of the DTOID path: the hand-written HIP ops through the C ABI against the CPU
restatements (oracle/dtoid_oracle.py), the detector head against golden vectors from the REFERENCE classes, and the
finetune step against torch.optim.Adam. Floating point: fp32 everywhere; tolerances are written at each check
(the convolutions run in MIOpen on the GPU and in torch-CPU for the fixture, so sums are reordered)."""
import numpy as np
import pytest
import torch

from oracle import dtoid_oracle
from ossid_code_amd import dtoid
from ossid_code_amd.dtoid import finetune, ops
from test_dtoid_cpu import G, close, run_head

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,C,H,W", [(2, 640, 29, 39), (1, 64, 240, 320), (3, 5, 7, 9), (2, 64, 1, 1), (1, 3, 4, 70)])
def test_dw_xcorr_forward_and_both_gradients(hiplib, B, C, H, W):
    g = torch.Generator().manual_seed(B * 1000 + C)
    x = torch.randn(B, C, H, W, generator=g)
    k = torch.randn(B, C, 3, 3, generator=g)
    go = torch.randn(B, C, H, W, generator=g)
    xr, kr = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
    want = dtoid_oracle.dw_xcorr(xr, kr)
    want.backward(go)
    xd, kd = x.cuda().requires_grad_(True), k.cuda().requires_grad_(True)
    got = ops.dw_xcorr(xd, kd)
    got.backward(go.cuda())
    assert close(got, want.detach().numpy(), rtol=1e-5, atol=1e-5)                 # 9-term sums
    assert close(xd.grad, xr.grad.numpy(), rtol=1e-5, atol=1e-5)
    assert close(kd.grad, kr.grad.numpy(), rtol=1e-4, atol=1e-4 * max(1.0, (H * W) ** 0.5))   # H*W-term sums


def test_dw_xcorr_broadcasts_one_image_over_templates(hiplib):
    x = torch.randn(1, 16, 9, 11).cuda()
    k = torch.randn(4, 16, 3, 3).cuda()
    got = ops.dw_xcorr(x, k)
    assert close(got, dtoid_oracle.dw_xcorr(x.cpu(), k.cpu()).numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 1024, 1025, 3000])
def test_nms_matches_greedy_oracle(hiplib, n):
    g = torch.Generator().manual_seed(n)
    ctr = torch.rand(n, 2, generator=g) * 200
    wh = torch.rand(n, 2, generator=g) * 60 + 2
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    scores = torch.rand(n, generator=g)
    if n > 10:
        boxes[5] = boxes[2]                       # exact duplicates
        scores[7] = scores[3]                     # tied scores: stable order decides
    want = dtoid_oracle.nms(boxes, scores, 0.5)
    got = ops.nms(boxes.cuda(), scores.cuda(), 0.5)
    assert got.dtype == torch.long and got.cpu().tolist() == want.tolist()
    assert ops.nms(boxes[:0].cuda(), scores[:0].cuda(), 0.5).numel() == 0


def test_decode_clip_matches_reference_golden(hiplib):
    anc, reg = torch.from_numpy(G["anchors"]).cuda(), torch.from_numpy(G["reg"]).cuda()
    got = ops.decode_clip_boxes(anc, reg, 40, 32)
    want = dtoid_oracle.decode_clip_boxes(anc.cpu(), reg.cpu(), 40, 32)
    assert close(got, want.numpy(), rtol=1e-5, atol=1e-4)
    unclipped = torch.from_numpy(G["boxes"])            # the reference's BBoxTransform output
    ref = unclipped.clone()
    ref[..., 0].clamp_(min=0), ref[..., 1].clamp_(min=0), ref[..., 2].clamp_(max=40), ref[..., 3].clamp_(max=32)
    assert close(got, ref.numpy(), rtol=1e-5, atol=1e-4)


def test_head_forward_backward_on_gpu_matches_reference_golden(hiplib):
    out, _ = run_head("cuda")
    for k, v in out.items():
        assert close(v, G[k], rtol=2e-3, atol=2e-4), k        # MIOpen vs torch-CPU summation order, 5760-term convs


@pytest.mark.parametrize("steps", [1, 3])
def test_fused_amsgrad_matches_torch_adam(hiplib, steps):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).cuda()
    ref = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5)).cuda()
    ref.load_state_dict(net.state_dict())
    flat = finetune.FlatParams(net, unused_filter=lambda n: n.startswith("1.bias"))   # pretend one tensor is unused
    opt = finetune.FusedAMSGrad(flat, lr=1e-2, weight_decay=1e-3)
    used = [p for n, p in ref.named_parameters() if not n.startswith("1.bias")]
    ropt = torch.optim.Adam(used, lr=1e-2, weight_decay=1e-3, amsgrad=True)
    frozen = net[1].bias.detach().clone()
    for s in range(steps):
        x = torch.randn(11, 37, device="cuda")
        for m, o in ((net, opt), (ref, ropt)):
            o.zero_grad()
            m(x).square().mean().backward()
            o.step()
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        if n.startswith("1.bias"):
            assert torch.equal(p, frozen)                     # never touched, like a grad-less tensor under Adam
        else:
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), n


def _batch(cfg, B, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    H, W, hh, hw = cfg.model.img_h, cfg.model.img_w, cfg.model.heatmap_h, cfg.model.heatmap_w
    mask = torch.zeros(B, 1, H, W)
    mask[:, :, H // 4: H // 2, W // 4: W // 2] = 1
    b = {"img": torch.rand(B, 3, H, W, generator=g), "limg": torch.rand(B, 3, 124, 124, generator=g),
         "lmask": (torch.rand(B, 1, 124, 124, generator=g) > 0.5).float(),
         "gimg": torch.rand(B, 3, 124, 124, generator=g), "gmask": (torch.rand(B, 1, 124, 124, generator=g) > 0.5).float(),
         "bbox_gt": torch.tensor([[[W / 4.0, H / 4.0, W / 2.0, H / 2.0, 1.0]]]).repeat(B, 1, 1),
         "heatmap": torch.rand(B, 1, hh, hw, generator=g).double(), "mask": mask}
    return {k: v.to(dev) for k, v in b.items()}


def _condition_encoders(m):
    """He initialisation + visible biases for the two SqueezeNet template encoders. With torch's default init the
    activations of those 18-convolution stacks collapse to per-channel constants by the 7x7 stage; the training BatchNorms
    behind them then divide by sqrt(eps), and any two float32 evaluation orders (let alone two Adam trajectories) differ
    by per cent in everything downstream. Pretrained weights -- what the reference finetunes -- do not behave like that."""
    net = m.model if hasattr(m, "model") else m
    with torch.no_grad():
        for enc in (net.template_feature_extractor, net.template_feature_extractor_global):
            for mod in enc.modules():
                if isinstance(mod, torch.nn.Conv2d):
                    torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
                    mod.bias.normal_(0, 0.1)
    return m


def test_full_network_shapes_and_finetune_step_480x640(hiplib):
    """D11/D13/D14/D16 at the real size: shapes of every output, loss decreases under the fused step,
    template cache stays on the device, and test-time inference returns the reference's dict."""
    cfg = dtoid.DtoidConfig()
    torch.manual_seed(0)
    m = dtoid.DtoidNet(cfg).cuda()
    flat = finetune.FlatParams(m)
    assert flat.n_used < flat.total and m.model.classification.conv1.weight.data_ptr() >= flat.param.data_ptr()
    opt = finetune.FusedAMSGrad(flat, lr=1e-4, weight_decay=1e-6)
    m.train()
    batch = _batch(cfg, 2, "cuda")
    out = m(batch)
    assert out["classifications"].shape == (2, 27144, 2) and out["regressions"].shape == (2, 27144, 4)
    assert out["anchors"].shape == (1, 27144, 4) and out["heat_map"].shape == (2, 1, 29, 39)
    assert out["segmentation"].shape == (2, 1, 480, 640) and out["transformed_anchors"].shape == (2, 27144, 4)
    losses = [float(finetune.finetune_step(m, batch, opt)) for _ in range(4)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    m.eval()
    with torch.no_grad():   # untie the scores: with the zero-initialised output layers every anchor scores exactly 0.01
        m.model.classification.output.weight.normal_(0, 0.05)     # and torch.topk's order among exact ties is arbitrary
        m.model.regression.output.weight.normal_(0, 0.01)
    nt = 3
    test = {"img": batch["img"][:1], "obj_id": torch.tensor([5]), "limg": torch.rand(1, nt, 3, 124, 124).cuda(),
            "lmask": (torch.rand(1, nt, 1, 124, 124) > 0.5).float().cuda(), "mask": batch["mask"][:1],
            "heatmap": batch["heatmap"][:1]}
    res = m.forwardTestTime(test)
    k = res["pred_scores"].shape[0]
    assert 1 <= k <= 500 and res["pred_bbox"].shape == (k, 4) and res["segmentation"].shape == (k, 1, 480, 640)
    assert res["heat_map"].shape == (k, 1, 29, 39) and res["final_bbox"][0] is res["pred_bbox"]
    assert (res["pred_scores"][:-1] >= res["pred_scores"][1:]).all() and "seg_IoU" in res
    assert (res["pred_template_ids"] >= 0).all() and (res["pred_template_ids"] < nt).all()
    local, glob = m.template_feature_cache[5]
    assert local[0].is_cuda and local[0].shape == (nt, 640, 7, 7) and glob[0].shape == (1, 64, 3, 3)
    res2 = m.forwardTestTime(test)                           # second frame: served from the device-resident cache
    assert m.template_feature_cache[5][0][0] is local[0] and res2["pred_bbox"].shape[1] == 4
    # The convolutions MIOpen picks for the backbone are not run-to-run deterministic (differences ~1e-8 in the class
    # probabilities, eager and graph alike), and a random-weight network's scores are near ties, so post-NMS lists may
    # differ between two calls; the dense outputs are what can be compared:
    net = m.model
    with torch.no_grad():
        a = [t.clone() for t in net._graphed_dense(dtoid.normalizeImageRange(test["img"]), local, glob[0])[:4]]
        b = [t.clone() for t in net._graphed_dense(dtoid.normalizeImageRange(test["img"]), local, glob[0])[:4]]
    assert all(float((x - y).abs().max()) < 1e-5 for x, y in zip(a, b))


@pytest.mark.parametrize("B,Cin,Cout,H,W", [
    (3, 640, 256, 29, 39),     # correlation convs (WM=4, FLAT)
    (21, 768, 512, 29, 39),    # fusion conv at n_t = 21 (NT=4)
    (2, 512, 48, 29, 39),      # classification output: Cout not a multiple of 32 (WM=2)
    (2, 256, 96, 29, 39),      # regression output: 3 channel tiles
    (2, 256, 128, 58, 78),     # decoder s2
    (1, 128, 64, 116, 156),    # decoder s3 (ROWSEG, WM=2)
    (1, 32, 16, 480, 640),     # decoder s5 (ROWSEG, single channel tile)
    (2, 16, 32, 5, 7),         # tiny image, one chunk
    (21, 64, 32, 37, 150),     # 2-D pixel tiles with ragged rows and columns, XCD-contiguous block runs
    (4, 64, 640, 29, 39),      # 20 channel tiles = 5 groups: the plain (non XCD-aware) block mapping
    (3, 64, 1024, 29, 39),     # 8 channel-tile groups: one per XCD
    (64, 64, 256, 29, 39),     # many workgroups: the round-aware choice goes to the widest pixel tile
    (5, 64, 128, 29, 39),      # ... and here to a narrow one
    (1, 48, 32, 30, 40),       # split-K small path with a ragged last 128-channel chunk
    (1, 64, 32, 1, 1),         # degenerate spatial size
])
def test_conv3x3_mfma_matches_torch(hiplib, B, Cin, Cout, H, W):
    """Hand-written implicit-GEMM convolution vs torch (float64 on the CPU as ground truth).
    Tolerance: exact-f32 fmaf chains over up to 9*768 terms -> 2e-5 of the output scale."""
    g = torch.Generator().manual_seed(Cin * 7 + Cout)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1)
    bn = torch.nn.BatchNorm2d(Cout).eval()
    with torch.no_grad():
        bn.running_mean.copy_(0.1 * torch.randn(Cout, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(Cout, generator=g))
        bn.weight.copy_(1 + 0.2 * torch.randn(Cout, generator=g))
        bn.bias.copy_(0.1 * torch.randn(Cout, generator=g))
    x = torch.randn(B, Cin, H, W, generator=g)
    with torch.no_grad():
        ref_plain = conv.double()(x.double())
        ref_fused = bn.double()(torch.nn.functional.elu(ref_plain))
    conv, bn = conv.float().cuda(), bn.float().cuda()
    scale = float(ref_plain.abs().max())
    got = ops.PackedConv3x3(conv)(x.cuda())
    assert got.shape == (B, Cout, H, W) and got.is_contiguous(memory_format=torch.channels_last)
    assert float((got.cpu().double() - ref_plain).abs().max()) <= 2e-5 * scale
    got = ops.PackedConv3x3(conv, bn=bn, act=True)(x.cuda().contiguous(memory_format=torch.channels_last))
    assert float((got.cpu().double() - ref_fused).abs().max()) <= 2e-5 * max(scale, float(ref_fused.abs().max()))


def test_fused_head_matches_module_path(hiplib):
    """The test-time head on the hand-written conv (fused ELU+BN epilogues, channels-last) vs the nn.Module path
    (MIOpen convolutions), compared on the DENSE outputs (post-NMS lists of a random-weight network are ill-conditioned):
    class probabilities / box deltas / heat maps / segmentation logits within 1e-4 of the output scale."""
    torch.manual_seed(3)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    with torch.no_grad():   # the zero-initialised output layers would make every output a constant
        for conv in (net.classification.output, net.regression.output, net.correlation_model.seg_final,
                     net.correlation_model.corr_conv_heatmap):
            conv.weight.normal_(0, 0.05)
    feat = torch.randn(1, 640, 29, 39, device="cuda")
    tmpl = torch.randn(4, 640, 7, 7, device="cuda")

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp(min=1e-6))

    with torch.no_grad():
        x2r, heatr, segr = net.correlation_model(feat.expand(4, -1, -1, -1), tmpl, True)
        clsr, regr = net.classification(x2r)[0], net.regression(x2r)
        fused = net._fused_head()
        x2, heat, seg = fused.correlation(feat, tmpl)
        cls, reg = fused.classification(x2), fused.regression(x2)
    assert x2.shape == x2r.shape and seg.shape == (4, 1, 480, 640) and cls.shape == (4, 27144, 2)
    for name, a, b in (("x2", x2, x2r), ("heat", heat, heatr), ("seg", seg, segr), ("cls", cls, clsr), ("reg", reg, regr)):
        assert rel(a, b) < 1e-4, (name, rel(a, b))
    # weights changed (a finetune step) -> the packed plan is rebuilt
    with torch.no_grad():
        net.classification.conv1.weight.mul_(1.5)
        cls2r = net.classification(x2r)[0]
        cls2 = net._fused_head().classification(x2)
    assert net._fused_head() is fused and rel(cls2, cls2r) < 1e-4 and rel(cls2, cls) > 1e-3
    # and the whole test-time call runs on it
    img = torch.rand(1, 3, 480, 640, device="cuda")
    tm = torch.rand(5, 4, 124, 124, device="cuda")
    with torch.no_grad():
        g = [net.compute_template_global(tm[:1])]
        loc = [net.compute_template_local(tm[:3]), net.compute_template_local(tm[3:])]
        out = net.forward_all_templates(img, loc, g, topk=50)
    k = out[0].shape[0]
    assert 1 <= k <= 50 and out[1].shape == (k, 4) and out[3].shape == (k, 480, 640) and out[4].shape == (k, 29, 39)


def test_graphed_forward_equals_eager(hiplib):
    """hipGraph replay of the dense part of forward_all_templates gives the eager results, also for a second image
    through the same captured graph, and after a weight update."""
    torch.manual_seed(5)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    with torch.no_grad():
        for conv in (net.classification.output, net.regression.output, net.correlation_model.seg_final):
            conv.weight.normal_(0, 0.05)
        tm = torch.rand(4, 4, 124, 124, device="cuda")
        g = net.compute_template_global(tm[:1])
        loc = [net.compute_template_local(tm)]
        for trial in range(3):
            img = torch.rand(1, 3, 480, 640, device="cuda")
            if trial == 2:
                net.classification.conv2.bias.add_(0.01)       # "finetuned" weights: same storage, new values
            net.use_graph = False
            ref = net._dense_all_templates(img, loc, g)
            net.use_graph = True
            got = net._graphed_dense(img, loc, g)
            for a, b in zip(got[:4], ref[:4]):
                assert torch.allclose(a, b, rtol=1e-5, atol=1e-6)
        assert len(net._graph_cache) <= 2
        out = net.forward_all_templates(img, loc, [g], topk=20)
        assert out[0].numel() >= 1


@pytest.mark.parametrize("Hs,Ws,H,W,Cin,Cout", [(29, 39, 58, 78, 256, 128), (232, 312, 480, 640, 32, 16), (5, 7, 5, 7, 16, 8),
                                                 (58, 78, 116, 156, 128, 64), (10, 13, 23, 31, 16, 32)])
def test_conv3x3_fused_nearest_upsample(hiplib, Hs, Ws, H, W, Cin, Cout):
    """conv(F.interpolate(x, mode='nearest')) without materialising the up-sampled tensor: same index rule as torch."""
    g = torch.Generator().manual_seed(H)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).cuda()
    x = torch.randn(2, Cin, Hs, Ws, generator=g).cuda()
    with torch.no_grad():
        up = torch.nn.functional.interpolate(x, size=(H, W), mode="nearest")
        want = ops.PackedConv3x3(conv, wino=False)(up)           # the same (direct) kernel on the materialised tensor
        pk = ops.PackedConv3x3(conv)
        xl = x.contiguous(memory_format=torch.channels_last)
        got = pk.run(xl, 2, H, W, torch.empty_like(want), src_hw=(Hs, Ws))     # the 9-tap kernel with the fused index map
        via_call = pk(x, size=(H, W))        # exact 2x: four 2x2 phase convolutions with merged weights (not bit-identical)
        ref = conv.double()(up.double())
    assert torch.equal(got, want)                                # bit-identical: only the staging index differs
    assert float((got.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
    assert float((via_call.double() - ref).abs().max()) <= 2e-5 * float(ref.abs().max())


def test_graphed_finetune_step_matches_eager(hiplib):
    """forward+backward replayed from a hipGraph: same loss and same parameter trajectory as the eager step."""
    cfg = dtoid.DtoidConfig()
    results = []
    for graphed in (False, True):
        torch.manual_seed(0)
        m = _condition_encoders(dtoid.DtoidNet(cfg).cuda().train())
        flat = finetune.FlatParams(m)
        opt = finetune.FusedAMSGrad(flat, lr=1e-4, weight_decay=1e-6)
        batches = [_batch(cfg, 2, "cuda", seed=s) for s in (0, 1, 2)]
        g = finetune.GraphedForwardBackward(m, flat, batches[0]) if graphed else None
        losses, r_first = [], None
        for b in batches:
            losses.append(float(finetune.finetune_step(m, b, opt, graphed=g)))
            if r_first is None:
                r_first = m.model.correlation_model.nf.running_mean.clone()
        results.append((losses, flat.param.clone(), m.model.correlation_model.nf.running_mean.clone(), r_first))
    (l0, p0, r0, f0), (l1, p1, r1, f1) = results
    assert np.allclose(l0, l1, rtol=3e-4), (l0, l1)
    # BatchNorm statistics: the warm-up passes left no trace -- after the FIRST step the running mean of the graphed run equals
    # the eager run's to rounding (two extra momentum updates would be a +50 % change), and the first loss is the same number
    # (what tools/debug_graph_bn.py used to print). Later the two Adam trajectories part ways (step 1 moves EVERY parameter by
    # exactly +-lr, the sign taken from gradients that are rounding noise for most of this zero-initialised-output network),
    # which shows as a few per cent in the running means by step 3 (measured: 5-9 %)
    assert abs(l0[0] - l1[0]) <= 1e-6 * abs(l0[0]), (l0[0], l1[0])
    assert float((f0 - f1).abs().max()) <= 1e-5 * float(f0.abs().max()), float((f0 - f1).abs().max())
    assert float((r0 - r1).abs().mean() / r0.abs().mean()) < 0.15
    assert float((p0 - p1).abs().max()) < 5e-4                     # 3 Adam steps of lr 1e-4 (sign-like updates)


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(1, 1024, 640, 29, 39), (1, 256, 128, 120, 160), (2, 64, 128, 30, 40),
                                           (2, 96, 128, 60, 80), (1, 224, 128, 120, 160), (8, 992, 128, 29, 39),
                                             (1, 512, 256, 60, 80), (3, 32, 32, 7, 5), (1, 96, 24, 9, 11)])
def test_conv1x1_with_pre_and_post_fusion(hiplib, B, Cin, Cout, H, W):
    """1x1 conv with BN+ReLU folded into the input staging and ELU+BN into the epilogue vs float64 torch."""
    g = torch.Generator().manual_seed(Cin + Cout)

    def rbn(n):
        bn = torch.nn.BatchNorm2d(n).eval()
        with torch.no_grad():
            bn.running_mean.copy_(0.1 * torch.randn(n, generator=g)), bn.running_var.copy_(0.5 + torch.rand(n, generator=g))
            bn.weight.copy_(1 + 0.2 * torch.randn(n, generator=g)), bn.bias.copy_(0.1 * torch.randn(n, generator=g))
        return bn

    conv, pre, post = torch.nn.Conv2d(Cin, Cout, 1), rbn(Cin), rbn(Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    with torch.no_grad():
        ref = post.double()(torch.nn.functional.elu(conv.double()(torch.relu(pre.double()(x.double())))))
    conv, pre, post = conv.float().cuda(), pre.float().cuda(), post.float().cuda()
    got = ops.PackedConv(conv, bn=post, act=True, pre_bn=pre, pre_relu=True)(x.cuda())
    assert float((got.cpu().double() - ref).abs().max()) <= 3e-5 * float(ref.abs().max())


def test_conv_writes_into_a_channel_slice(hiplib):
    """DenseNet-style in-place concatenation: read the first c channels of a wide buffer, append 32 at an offset."""
    g = torch.Generator().manual_seed(9)
    B, H, W, C, ctot = 2, 9, 13, 64, 128
    buf = torch.randn(B, ctot, H, W, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    before = buf.clone()
    conv = torch.nn.Conv2d(C, 32, 3, padding=1, bias=False).cuda()
    pk = ops.PackedConv(conv)
    pk.run(buf, B, H, W, buf, in_cs=ctot, out_cs=ctot, out_coff=96)
    with torch.no_grad():
        want = conv(before[:, :C].contiguous())
    assert torch.equal(buf[:, :96], before[:, :96])                       # nothing else touched
    assert torch.allclose(buf[:, 96:], want, rtol=1e-4, atol=1e-4)


def test_fused_backbone_matches_module_path(hiplib):
    """DenseNet-121 trunk of ImageFeatExtract on the hand-written kernels vs the nn.Module path (MIOpen), 480x640."""
    torch.manual_seed(11)
    ife = dtoid.ImageFeatExtract().cuda().eval()
    with torch.no_grad():
        for m in ife.modules():                                           # non-trivial BatchNorm statistics
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 1.5), m.weight.normal_(1, 0.1), m.bias.normal_(0, 0.1)
        img = torch.rand(1, 3, 480, 640, device="cuda")
        tg = torch.randn(1, 64, 3, 3, device="cuda") * 0.1
        ref = ife(img, tg)
        got = dtoid.network.FusedBackbone(ife)(img, tg)
    assert got.shape == ref.shape == (1, 640, 29, 39)
    assert float((got - ref).abs().max()) <= 1e-3 * float(ref.abs().max())   # 120 chained layers, two f32 sum orders


@pytest.mark.parametrize("B,C0,L,H,W", [
    (1, 256, 24, 30, 40),      # DenseNet-121 block 3 of one 480x640 frame: 6 groups per tile at the first layers
    (1, 512, 16, 29, 39),      # block 4: ragged tiles in both directions
    (1, 128, 12, 60, 80),      # block 2: the group count is capped by the workgroup budget
    (2, 64, 6, 13, 9),         # two images, tiles cut by the right and bottom edge, the narrowest entry kernel
    (1, 64, 1, 4, 8),          # a single layer: no later layer to feed
])
def test_dense_block_one_launch_per_layer_matches_float64_and_the_two_launch_path(hiplib, B, C0, L, H, W):
    """csrc/dense.hip (incremental bottleneck sums, one launch per layer) against the same block in float64 on the CPU,
    and against the per-layer path on csrc/conv.hip. Tolerance: the block is up to 48 chained convolutions on the
    three-product bf16 form (~5e-6 of a layer's output scale each): the fused form has to be as close to float64 as the
    two-launch form is, within 2x, and both within 1e-4 of the output scale."""
    from ossid_code_amd.dtoid.backbones import DenseBlock
    if not hiplib.lib().ossid_conv_split_bf16():
        pytest.skip("csrc/dense.hip exists in the split-bf16 form only: an all-exact build (-DOSSID_CONV_F32) runs the two-launch path")
    torch.manual_seed(C0 + L)
    blk = DenseBlock(L, C0).eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 1.5), m.weight.normal_(1, 0.1), m.bias.normal_(0, 0.1)
        x = torch.randn(B, C0, H, W)
        ref = blk.double()(x.double())
    blk = blk.float().cuda()
    P = ops.PackedConv
    layers = [(P(l.conv1, pre_bn=l.norm1, pre_relu=True), P(l.conv2, pre_bn=l.norm2, pre_relu=True)) for l in blk.values()]
    table = ops.dense_block_table(layers, blk.growth)
    assert table is not None and tuple(table.shape) == (L, 4)
    ctot = C0 + 32 * L

    def fresh():
        buf = torch.empty((B, ctot, H, W), device="cuda").contiguous(memory_format=torch.channels_last)
        buf.fill_(float("nan"))                                           # every appended channel must be written
        buf[:, :C0] = x.cuda()
        return buf
    fused = ops.dense_block_fused(fresh(), B, H, W, C0, layers, table)
    two = fresh()
    tmp = torch.empty((B, 128, H, W), device="cuda").contiguous(memory_format=torch.channels_last)
    c = C0
    for c1, c2 in layers:
        c1.run(two, B, H, W, tmp, in_cs=ctot)
        c2.run(tmp, B, H, W, two, out_cs=ctot, out_coff=c)
        c += 32
    torch.cuda.synchronize()
    scale = float(ref.abs().max())
    e_f = float((fused.cpu().double() - ref).abs().max()) / scale
    e_t = float((two.cpu().double() - ref).abs().max()) / scale
    assert torch.equal(fused[:, :C0], two[:, :C0])
    assert e_t <= 1e-4 and e_f <= max(2 * e_t, 2e-5), (e_f, e_t)
    again = ops.dense_block_fused(fresh(), B, H, W, C0, layers, table)     # fixed summation order: bit-reproducible
    assert torch.equal(again, fused)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Hs,Ws,H,W", [(2, 232, 312, 480, 640), (1, 29, 39, 61, 83), (3, 20, 24, 40, 48),
                                         (1, 7, 9, 30, 31)])
def test_seg_tail_fused_matches_torch(hiplib, B, Hs, Ws, H, W):
    """up-sample + conv 32->16 + ELU + BN + conv 16->1 in one launch vs the same layers in torch (network.py:357-362);
    covers ragged tiles (sizes that are no multiple of the 14 x 30 tile) and non-integer up-sampling ratios."""
    import torch.nn.functional as F
    torch.manual_seed(B * 1000 + H)
    c1 = torch.nn.Conv2d(32, 16, 3, padding=1).cuda()
    bn = torch.nn.BatchNorm2d(16).cuda().eval()
    c2 = torch.nn.Conv2d(16, 1, 3, padding=1).cuda()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.2)
    x = torch.randn(B, 32, Hs, Ws, device="cuda")
    tail = ops.SegTail(c1, bn, c2)
    got = tail(x, size=(H, W))
    assert got is not None and got.shape == (B, 1, H, W)
    with torch.no_grad():
        want = c2(bn(F.elu(c1(F.interpolate(x, size=(H, W))))))
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), float((got - want).abs().max())
    # a shape the fused kernel does not take (no up-sampling): the caller falls back
    assert tail(x, size=(Hs, Ws)) is None


@pytest.mark.gpu
def test_graphed_test_time_path_follows_a_finetune_step(hiplib):
    """The packed plans and the captured hipGraph must see parameter updates made by the fused optimizer (a raw kernel on
    the flat buffer): detect, take finetune steps, detect again == a fresh network loaded with the updated weights."""
    cfg = dtoid.DtoidConfig()
    torch.manual_seed(3)
    m = dtoid.DtoidNet(cfg).cuda().eval()
    with torch.no_grad():   # non-degenerate outputs (the reference zero-initialises the output layers)
        for conv in (m.model.classification.output, m.model.regression.output, m.model.correlation_model.seg_final):
            conv.weight.normal_(0, 0.01)
    flat = finetune.FlatParams(m)
    opt = finetune.FusedAMSGrad(flat, lr=1e-3)
    g = torch.Generator().manual_seed(5)
    test = {"img": torch.rand(1, 3, 480, 640, generator=g).cuda(), "obj_id": torch.tensor([1]),
            "limg": torch.rand(1, 3, 3, 124, 124, generator=g).cuda(),
            "lmask": (torch.rand(1, 3, 1, 124, 124, generator=g) > 0.5).float().cuda()}
    net = m.model

    def dense():
        m.clearCache()
        local, glob = m._template_features(test, 1, torch.device("cuda", 0))
        from ossid_code_amd.dtoid.model import normalizeImageRange
        outs = net._graphed_dense(normalizeImageRange(test["img"]), local, glob[0])
        return [o.clone() for o in outs[:4]]
    before = dense()
    n_graphs = len(net.__dict__["_graph_cache"])
    b = _batch(cfg, 2, "cuda")
    m.train()
    for _ in range(2):
        finetune.finetune_step(m, b, opt)
    m.eval()
    after = dense()
    assert len(net.__dict__["_graph_cache"]) == n_graphs            # same graph, re-packed weights
    assert not torch.allclose(before[0], after[0])
    fresh = dtoid.DtoidNet(cfg).cuda().eval()
    fresh.load_state_dict(m.state_dict())
    fnet = fresh.model
    fnet.use_graph = False
    from ossid_code_amd.dtoid.model import normalizeImageRange
    local, glob = fresh._template_features(test, 1, torch.device("cuda", 0))
    want = fnet._dense_all_templates(normalizeImageRange(test["img"]), local, glob[0])
    for a, w in zip(after, want[:4]):
        assert torch.allclose(a, w, rtol=1e-4, atol=1e-5), float((a - w).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 37])
def test_gather_rows_with_sigmoid(hiplib, k):
    g = torch.Generator().manual_seed(k)
    src = torch.randn(9, 48, 64, generator=g).cuda()
    idx = torch.randint(0, 9, (k,), generator=g).cuda()
    assert torch.equal(ops.gather_rows(src, idx), src[idx])
    got = ops.gather_rows(src, idx, sigmoid=True)
    assert got.shape == (k, 48, 64) and torch.allclose(got, torch.sigmoid(src[idx]), rtol=1e-6, atol=1e-6)


@pytest.mark.gpu
def test_dw_xcorr_channels_last_broadcast_matches_grouped_conv(hiplib):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(1, 24, 9, 13, generator=g).cuda()
    k = torch.randn(5, 24, 3, 3, generator=g).cuda()
    got = ops.dw_xcorr_nhwc_bcast(x.contiguous(memory_format=torch.channels_last), k)
    want = dtoid_oracle.dw_xcorr(x.cpu().expand(5, -1, -1, -1), k.cpu())
    assert got.shape == (5, 24, 9, 13) and got.is_contiguous(memory_format=torch.channels_last)
    assert close(got.cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
def test_c_abi_rejects_bad_arguments_without_launching(hiplib):
    """The boundary's error convention (include/ossid_hip.h): a negative status for arguments a kernel could not take --
    checked on the host, before anything is launched -- and OK for empty work."""
    from ctypes import byref as C_byref
    from ossid_code_amd import _lib
    buf = torch.zeros(1 << 16, device="cuda")
    p, s = buf.data_ptr(), _lib.stream()
    d = _lib.ConvDesc()
    d.x = d.wpk = d.out = p
    d.batch, d.height, d.width, d.cin, d.cout, d.taps, d.in_batch_stride = 1, 8, 8, 24, 32, 9, -1     # cin % 16 != 0
    assert _lib.fn("ossid_conv_nhwc_fwd")(C_byref(d), s) < 0
    d.cin, d.taps = 32, 5                                                                               # taps: 1, 9 or 4 (phases)
    assert _lib.fn("ossid_conv_nhwc_fwd")(C_byref(d), s) < 0
    d.taps, d.out = 9, None                                                                             # null output
    assert _lib.fn("ossid_conv_nhwc_fwd")(C_byref(d), s) < 0
    d.out, d.batch = p, 0                                                                               # empty batch: fine
    assert _lib.fn("ossid_conv_nhwc_fwd")(C_byref(d), s) == 0
    # fused decoder tail: no up-sampling -> the source footprint does not fit the staged patch
    assert _lib.fn("ossid_seg_tail_fwd")(p, 1, 32, 32, 32, 32, 32, p, p, p, p, p, p, p, s) < 0
    assert _lib.fn("ossid_seg_tail_fwd")(p, 0, 16, 16, 32, 32, 32, p, p, p, p, p, p, p, s) == 0
    assert _lib.fn("ossid_gather_rows")(p, 4, 6, p, 2, 0, p, s) < 0                                     # rows % 4 != 0
    assert _lib.fn("ossid_gather_rows")(p, 4, 8, p, 0, 0, p, s) == 0
    assert _lib.fn("ossid_dw_xcorr_nhwc_bcast")(p, p, 2, 6, 4, 4, p, s) < 0                             # channels % 4 != 0
    assert _lib.fn("ossid_nms")(p, -1, 0.5, p, 1 << 16, p, p, s) < 0
    assert _lib.fn("ossid_nms")(p, 100, 0.5, p, 8, p, p, s) < 0                                         # workspace too small
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fused_test_time_path_at_the_reference_default_480x480(hiplib):
    """Network's own default geometry (network.py:381: img 480x480, heat map 29x29 -> 20 184 anchors): the fused + graphed
    dense path against the nn.Module path, two template chunks, the decoder tail at a different up-sampling ratio."""
    torch.manual_seed(9)
    net = dtoid.Network().cuda().eval()
    assert net.img_size == (480, 480) and net.heatmap_size == (29, 29)
    with torch.no_grad():
        for conv in (net.classification.output, net.regression.output, net.correlation_model.seg_final,
                     net.correlation_model.corr_conv_heatmap):
            conv.weight.normal_(0, 0.05)
        img = torch.rand(1, 3, 480, 480, device="cuda")
        tm = torch.rand(5, 4, 124, 124, device="cuda")
        g = net.compute_template_global(tm[:1])
        loc = [net.compute_template_local(tm[:3]), net.compute_template_local(tm[3:])]
        net.use_fused_head = net.use_fused_backbone = net.use_graph = False
        ref = net._dense_all_templates(img, loc, g)
        net.use_fused_head = net.use_fused_backbone = net.use_graph = True
        got = net._graphed_dense(img, loc, g)
        got2 = net._graphed_dense(img, loc, g)                 # replay with unchanged templates: cached template side
    assert got[0].shape == (5, 20184, 2) and got[2].shape == (5, 1, 480, 480) and got[3].shape == (5, 1, 29, 29)
    for name, a, b, c in zip(("cls", "reg", "seg", "heat"), got[:4], ref[:4], got2[:4]):
        scale = float(b.abs().max().clamp(min=1e-6))
        assert float((a - b).abs().max()) / scale < 2e-4, name
        assert torch.equal(a, c), name


@pytest.mark.gpu
def test_dot_by_channel_contraction_last_matches_module_path(hiplib):
    """conv(image * avg_t) as G (taps summed per channel, once per frame) + one GEMM over the channels, the form the fused
    head switches to for many templates: against the nn.Module correlation on the dense outputs."""
    torch.manual_seed(4)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    feat = torch.randn(1, 640, 29, 39, device="cuda")
    tmpl = torch.randn(6, 640, 7, 7, device="cuda")
    with torch.no_grad():
        x2r, heatr, segr = net.correlation_model(feat.expand(6, -1, -1, -1), tmpl, True)
        fused = net._fused_head()
        fused.DOT_GEMM_MIN_TEMPLATES = 1
        x2, heat, seg = fused.correlation(feat, tmpl)
    for name, a, b in (("x2", x2, x2r), ("heat", heat, heatr), ("seg", seg, segr)):
        assert float((a - b).abs().max() / b.abs().max().clamp(min=1e-6)) < 1e-4, name


@pytest.mark.gpu
@pytest.mark.parametrize("B,Cin,Cout,Hs,Ws", [(21, 256, 128, 29, 39), (3, 128, 64, 58, 78), (2, 64, 32, 116, 156),
                                              (2, 32, 48, 7, 5), (1, 512, 512, 9, 11)])
def test_phase_conv_equals_conv_of_2x_upsampled(hiplib, B, Cin, Cout, Hs, Ws):
    """conv3x3(F.interpolate(x, scale 2, nearest)) computed as four 2x2 phase convolutions of the source with merged
    weights (4/9 of the multiply-adds) vs torch on the up-sampled tensor, with the ELU + BatchNorm epilogue."""
    import torch.nn.functional as F
    torch.manual_seed(Cin + Cout + Hs)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).cuda()
    bn = torch.nn.BatchNorm2d(Cout).cuda().eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
    x = torch.randn(B, Cin, Hs, Ws, device="cuda")
    pk = ops.PackedConv3x3(conv, bn, act=True, phases=True)
    assert pk.wpk4 is not None
    xl = x.contiguous(memory_format=torch.channels_last)
    out = torch.empty((B, Cout, 2 * Hs, 2 * Ws), device="cuda").contiguous(memory_format=torch.channels_last)
    assert pk.run_phases(xl, B, Hs, Ws, out), "the phase path did not take this shape"
    with torch.no_grad():
        want = bn(F.elu(conv(F.interpolate(x, scale_factor=2, mode="nearest"))))
        full = pk.run(xl, B, 2 * Hs, 2 * Ws, torch.empty_like(out), src_hw=(Hs, Ws))      # the 9-tap fused-upsample path
    scale = float(want.abs().max())
    assert float((out - want).abs().max()) / scale < 2e-5
    assert float((out - full).abs().max()) / scale < 2e-5


@pytest.mark.gpu
def test_template_side_cache_is_not_fooled_by_recycled_addresses(hiplib):
    """Template features of one object are freed and another object's features land at the same device address (the caching
    allocator recycles it): the cached template-only tensors of the first object must not be used for the second."""
    torch.manual_seed(11)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    with torch.no_grad():
        for conv in (net.classification.output, net.regression.output, net.correlation_model.seg_final):
            conv.weight.normal_(0, 0.05)
        img = torch.rand(1, 3, 480, 640, device="cuda")
        g = net.compute_template_global(torch.rand(1, 4, 124, 124, device="cuda"))
        loc = [net.compute_template_local(torch.rand(3, 4, 124, 124, device="cuda"))]
        ptr = loc[0].data_ptr()
        first = [t.clone() for t in net._graphed_dense(img, loc, g)[:4]]
        del loc
        loc = [net.compute_template_local(torch.rand(3, 4, 124, 124, device="cuda") * 0.5)]
        recycled = loc[0].data_ptr() == ptr
        got = net._graphed_dense(img, loc, g)
        net.use_graph = False
        want = net._dense_all_templates(img, loc, g)
    for a, b in zip(got[:4], want[:4]):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5)
    assert not torch.allclose(got[0], first[0])
    print("address recycled:", recycled)


@pytest.mark.gpu
def test_batched_test_time_api_equals_per_image_calls(hiplib):
    """BASELINE configs[2] shape, reduced: forwardTestTimeBatch on B images x n_t templates gives, image by image, what
    forwardTestTime gives (the batched backbone reorders no sums per image: same kernels, same tiles -> tight tolerance;
    the dense head outputs are compared, post-NMS lists of a random-weight network are ill-conditioned)."""
    cfg = dtoid.DtoidConfig()
    torch.manual_seed(11)
    m = dtoid.DtoidNet(cfg).cuda().eval()
    with torch.no_grad():
        for conv in (m.model.classification.output, m.model.regression.output, m.model.correlation_model.seg_final,
                     m.model.correlation_model.corr_conv_heatmap):
            conv.weight.normal_(0, 0.05)
    g = torch.Generator().manual_seed(3)
    B, nt = 3, 5
    imgs = torch.rand(B, 3, 480, 640, generator=g).cuda()
    test = {"obj_id": torch.tensor([1]), "limg": torch.rand(1, nt, 3, 124, 124, generator=g).cuda(),
            "lmask": (torch.rand(1, nt, 1, 124, 124, generator=g) > 0.5).float().cuda()}
    outs = m.forwardTestTimeBatch(dict(test, img=imgs))
    assert len(outs) == B
    local, glob = m._template_features(test, 1, imgs.device)
    net = m.model
    with torch.no_grad():
        feats = net._features(dtoid.normalizeImageRange(imgs), glob[0])
        for i in range(B):
            one = net._features(dtoid.normalizeImageRange(imgs[i:i + 1]), glob[0])
            assert float((feats[i:i + 1] - one).abs().max()) <= 2e-4 * float(one.abs().max())
            single = m.forwardTestTime(dict(test, img=imgs[i:i + 1]))
            k = outs[i]["pred_scores"].shape[0]
            assert outs[i]["segmentation"].shape == (k, 1, 480, 640) and outs[i]["pred_bbox"].shape == (k, 4)
            assert abs(float(outs[i]["pred_scores"][0]) - float(single["pred_scores"][0])) < 1e-4
            assert set(outs[i]) == set(single)
            # dense outputs of the head-only graph on the batched features vs the single-image graph
            a = [t.clone() for t in net._graphed_dense(feats[i:i + 1], local, None, head_only=True)[:4]]
            b = net._graphed_dense(dtoid.normalizeImageRange(imgs[i:i + 1]), local, glob[0])[:4]
            for x, y in zip(a, b):
                assert float((x - y).abs().max()) <= 2e-4 * float(y.abs().max().clamp(min=1e-6))


@pytest.mark.gpu
def test_network_forward_on_pairs_eval_runs_on_the_fused_kernels_and_matches_the_module_path(hiplib):
    """configs[2] (ii): Network.forward on (image, template) pairs in eval / no_grad mode goes through FusedBackbone +
    FusedHead (per-pair images: no broadcast) and agrees with the nn.Module path."""
    torch.manual_seed(12)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    with torch.no_grad():
        for conv in (net.classification.output, net.regression.output, net.correlation_model.seg_final,
                     net.correlation_model.corr_conv_heatmap):
            conv.weight.normal_(0, 0.05)
    g = torch.Generator().manual_seed(4)
    B = 3
    args = [torch.rand(B, 3, 480, 640, generator=g), torch.rand(B, 3, 124, 124, generator=g),
            (torch.rand(B, 1, 124, 124, generator=g) > 0.5).float(), torch.rand(B, 3, 124, 124, generator=g),
            (torch.rand(B, 1, 124, 124, generator=g) > 0.5).float()]
    args = [a.cuda() for a in args]
    with torch.no_grad():
        got = net(*args)
        net.use_fused_head = net.use_fused_backbone = False
        want = net(*args)
        net.use_fused_head = net.use_fused_backbone = True
    assert got[0].shape == (B, 27144, 2) and got[1].shape == (B, 27144, 4) and got[4].shape == (B, 1, 480, 640)
    for name, a, b in zip(("cls", "reg", "anchors", "heat", "seg"), got, want):
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max().clamp(min=1e-6)), name


@pytest.mark.gpu
@pytest.mark.parametrize("wino", [False, True])
def test_hip_training_head_matches_reference_golden(hiplib, wino, monkeypatch):
    """The PRODUCT training path of the head (Network._head_train_hip: FusedConv / BNFold / wgrad / chan_op kernels,
    channels-last, BatchNorm folded into the next conv) against the REFERENCE's forward and backward
    (tests/golden/dtoid_head.npz, produced by the reference classes): outputs, the four losses, and the gradients with
    respect to both inputs and a sample of parameters -- same keys and tolerances as the module-path test above.
    wino: forward and data gradient of every plain 3x3 layer on the Winograd kernel (the fixture's 4x5 grid is far
    below the dispatch threshold, which is lowered to force it), with the branches on their side streams either way."""
    from ossid_code_amd.dtoid import train_ops
    monkeypatch.setattr(train_ops, "WINO_MIN_WGS", 1 if wino else 10 ** 9)
    from test_dtoid_cpu import GRID, IMG, SEED, seeded_inputs, seeded_state
    net = dtoid.Network(img_size=IMG, heatmap_size=GRID)
    for i, m in enumerate((net.correlation_model, net.classification, net.regression)):
        m.load_state_dict(seeded_state(m, SEED + i))
    net = net.cuda().train()
    corr, cls, reg = net.correlation_model, net.classification, net.regression
    feat, tmpl, ann, heat_t, mask_t = (t.cuda() for t in seeded_inputs(SEED + 10))
    feat.requires_grad_(True)
    tmpl.requires_grad_(True)
    c, r, anc, heat, seg = net._head_train_hip(feat.view_as(feat), tmpl.view_as(tmpl))      # (non-leaf, as in the product)
    boxes = dtoid.BBoxTransform()(anc, r)
    lc, lr = dtoid.DetectionLoss()(c, r, anc, ann)
    l_center = torch.nn.L1Loss()(heat_t, heat)
    l_seg = torch.nn.BCELoss()(torch.sigmoid(seg), mask_t)
    (20 * l_seg + 20 * l_center + lc + lr).sum().backward()
    out = dict(heat=heat, seg=seg, cls=c, reg=r, anchors=anc, boxes=boxes, loss_cls=lc, loss_reg=lr,
               loss_center=l_center, loss_seg=l_seg, grad_feat=feat.grad, grad_tmpl=tmpl.grad,
               grad_c1=corr.c1.weight.grad[:8], grad_cf_bias=corr.cf.bias.grad,
               grad_cls_conv1_bias=cls.conv1.bias.grad, grad_reg_out=reg.output.weight.grad[:4])
    for k, v in out.items():
        assert close(v, G[k], rtol=2e-3, atol=2e-4), k
    assert int(corr.ns3.num_batches_tracked) == 1 and int(corr.nf.num_batches_tracked) == 1


@pytest.mark.gpu
def test_hip_training_path_matches_module_path_whole_network(hiplib):
    """DtoidNet.forward + 4-term loss + backward at 480x640 on the hand-written training kernels (channels-last,
    BatchNorm folded into the next conv, dense blocks with shared batch statistics) vs the nn.Module path (MIOpen).
    Outputs, losses and BatchNorm buffers agree to 2e-4. The GRADIENT of this random-init network at batch 2 is
    ill-conditioned -- two runs of the module path itself differ by ~1e-2 in relative L2 (MIOpen's atomics), and
    gradients of biases in front of a training-mode BatchNorm are near-total cancellations -- so the whole gradient is
    compared as one vector against that run-to-run noise; layer-level gradient parity at 1e-3..1e-4 is what
    tests/test_train_ops_gpu.py and the reference-golden head test above establish."""
    import copy
    cfg = dtoid.DtoidConfig()
    torch.manual_seed(21)
    m = _condition_encoders(dtoid.DtoidNet(cfg).cuda().train())
    with torch.no_grad():   # the zero-initialised output layers would make three of the four losses blind to the trunk
        for conv in (m.model.classification.output, m.model.regression.output, m.model.correlation_model.seg_final,
                     m.model.correlation_model.corr_conv_heatmap):
            conv.weight.normal_(0, 0.02)
    ref, ref2 = copy.deepcopy(m), copy.deepcopy(m)
    batch = _batch(cfg, 2, "cuda", seed=5)
    m.model.use_hip_training, ref.model.use_hip_training, ref2.model.use_hip_training = True, False, False
    out, outr, outr2 = m(batch), ref(batch), ref2(batch)
    out["loss"].backward()
    outr["loss"].backward()
    outr2["loss"].backward()

    def rel(a, b):
        return float((a.detach().double() - b.detach().double()).abs().max() / b.detach().double().abs().max().clamp(min=1e-12))
    for k in ("classifications", "regressions", "heat_map", "segmentation", "loss", "loss_seg", "loss_center", "loss_cls",
              "loss_reg"):
        # (5e-4: at batch 2 the global template branch normalises over 2 x 3 x 3 values per channel, which amplifies the
        # rounding differences between two float32 paths; or three times what two runs of the module path differ by)
        assert rel(out[k], outr[k]) < max(5e-4, 3 * rel(outr2[k], outr[k])), (k, rel(out[k], outr[k]))
    num = den = noise = 0.0
    worst = []
    for (n, p), q, q2 in zip(m.named_parameters(), ref.parameters(), ref2.parameters()):
        if q.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0, n
            continue
        e = float((p.grad.double() - q.grad.double()).pow(2).sum())
        nz = float((q2.grad.double() - q.grad.double()).pow(2).sum())
        num, noise, den = num + e, noise + nz, den + float(q.grad.double().pow(2).sum())
        worst.append((e, nz, n))
    err, floor = (num / den) ** 0.5, (noise / den) ** 0.5
    worst = [(n, "%.2e" % (e / den) ** 0.5, "%.2e" % (nz / den) ** 0.5) for e, nz, n in sorted(worst, reverse=True)[:6]]
    assert err < max(3e-2, 3 * floor), (err, floor, worst)
    for (n, b), q in zip(m.named_buffers(), ref.buffers()):
        assert (rel(b, q) < 5e-4) if b.dtype.is_floating_point else torch.equal(b, q), n


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,kind", [(570024, 1000, "sigmoid"), (27144, 1000, "randn"), (5000, 1, "randn"), (1000, 1000, "randn"),
                                      (570024, 1000, "all_equal"), (100000, 500, "ties"), (70000, 2048, "negative"), (3, 2, "randn")])
def test_topk_radix_select_matches_torch(hiplib, n, k, kind):
    """ossid_topk through the C ABI vs torch.topk: same values; same indices wherever the value is unique; equal values are
    ordered -- and at the cut chosen -- by increasing index (zero-initialised output layers give 570 k identical scores)."""
    g = torch.Generator().manual_seed(n + k)
    if kind == "sigmoid":
        x = torch.sigmoid(torch.randn(n, generator=g) * 3)
    elif kind == "all_equal":
        x = torch.full((n,), 0.01)
    elif kind == "ties":
        x = torch.randint(0, 50, (n,), generator=g).float() / 50
    elif kind == "negative":
        x = -torch.rand(n, generator=g) * 1e-3 - 1.0
    else:
        x = torch.randn(n, generator=g)
    xd = x.cuda()
    vals, idx = ops.topk_scores(xd, k)
    rv, ri = torch.topk(x, k)
    assert idx.dtype == torch.int64 and torch.equal(vals.cpu(), rv)
    assert torch.equal(x[idx.cpu()], rv)                                   # the indices point at those values
    assert idx.unique().numel() == k                                        # no element twice
    # the deterministic rule: among equal values increasing index, and the cut takes the lowest indices
    want = torch.sort(-x, stable=True).indices[:k]
    assert torch.equal(idx.cpu(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one_box", "no_box", "two_boxes_and_padding", "saturated_probabilities"])
def test_fused_detection_loss_matches_tensor_expressions(hiplib, case):
    """ossid_focal_smoothl1_loss_{fwd,bwd} (three launches) vs the whole-batch tensor form of dtoid/loss.py (itself
    pinned on the reference's DetectionLoss through the golden file): both losses and both gradients."""
    g = torch.Generator().manual_seed(len(case))
    B, A = 3, 27144
    anchors = dtoid.Anchors(pyramid_levels=[4], ratios=[0.5, 1, 2], sizes=[30], scales=[1, 2, 3, 4, 5, 6, 7, 8])([(29, 39)], device="cuda")
    cls = torch.rand(B, A, 2, generator=g).cuda()
    if case == "saturated_probabilities":
        cls = (cls * 1.2 - 0.1).clamp(0, 1)                               # values at / beyond the 1e-4 clamps
    reg = (torch.randn(B, A, 4, generator=g) * 0.3).cuda()
    ann = torch.tensor([[[160.0, 120.0, 320.0, 240.0, 1.0], [-1.0] * 5], [[300.0, 200.0, 420.0, 330.0, 1.0], [-1.0] * 5],
                        [[50.0, 60.0, 200.0, 300.0, 0.0], [-1.0] * 5]]).cuda()
    if case == "no_box":
        ann[1, 0] = -1.0
    if case == "two_boxes_and_padding":
        ann[0, 1] = torch.tensor([400.0, 100.0, 600.0, 400.0, 1.0])
    res = {}
    for fused in (True, False):
        c, r = cls.clone().requires_grad_(True), reg.clone().requires_grad_(True)
        lossf = dtoid.DetectionLoss()
        lossf.use_fused = fused
        lc, lr = lossf(c, r, anchors, ann)
        (1.7 * lc + 0.6 * lr).sum().backward()
        res[fused] = (lc.detach(), lr.detach(), c.grad, r.grad)
    for a, b, name in zip(res[True], res[False], ("loss_cls", "loss_reg", "dcls", "dreg")):
        scale = float(b.abs().max().clamp(min=1e-12))
        assert float((a - b).abs().max()) <= 2e-5 * scale + 1e-9, (case, name)


@pytest.mark.gpu
@pytest.mark.parametrize("B,Cin,H,W,k,stride,pad,kpad", [(2, 3, 48, 64, 7, 2, 3, 160), (3, 4, 124, 124, 3, 2, 0, 48), (1, 3, 9, 11, 7, 2, 3, 160)])
def test_strided_stem_as_im2col_plus_mfma_conv_matches_torch(hiplib, B, Cin, H, W, k, stride, pad, kpad):
    """D1 + D4/D2: the 7x7/s2/p3 (DenseNet) and 3x3/s2/p0 (SqueezeNet) stems = ossid_im2col_stem (with
    normalizeImageRange fused, zero padding in normalised space) + a 1x1 convolution on the MFMA kernel."""
    torch.manual_seed(k + Cin)
    conv = torch.nn.Conv2d(Cin, 64, k, stride=stride, padding=pad, bias=Cin == 4).cuda()
    img = torch.rand(B, Cin, H, W, device="cuda")
    normalize = Cin == 3
    ref_in = dtoid.normalizeImageRange(img) if normalize else img
    with torch.no_grad():
        want = conv(ref_in)
        pk = ops.PackedConv(ops._StemAsMatrix(conv, kpad))
        got = pk(ops.im2col_stem(img, k, stride, pad, kpad, normalize=normalize))
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("k,stride,pad,ceil,H,W", [(3, 2, 1, False, 240, 320), (3, 2, 0, True, 61, 61), (3, 2, 0, True, 30, 30),
                                                   (3, 2, 0, True, 15, 15), (3, 2, 0, True, 8, 10)])
def test_maxpool_and_stem_tail_channels_last(hiplib, k, stride, pad, ceil, H, W):
    x = torch.randn(2, 64, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    want = torch.nn.functional.max_pool2d(x, k, stride, pad, ceil_mode=ceil)
    got = ops.maxpool_nhwc(x, k, stride, pad, ceil)
    assert got.shape == want.shape and torch.equal(got, want)
    for kb in (1, 2):
        kern = torch.randn(kb, 64, 3, 3, device="cuda")
        sc, sh = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda")
        ref = torch.relu((x + dtoid_oracle.dw_xcorr(x, kern.expand(2, -1, -1, -1))) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
        assert float((ops.stem_tail(x, kern, sc, sh) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.gpu
def test_template_encoders_and_stem_on_own_kernels_match_module_path(hiplib):
    """D2/D3/D4 at the real sizes: [n_t,4,124,124] -> [n_t,640,7,7] (TemplateFeatExtract), [1,4,124,124] -> [1,64,3,3]
    (TemplateFeatExtractGlobal, incl. the two valid 3x3 convs), and the image feature map [1,640,29,39] with the stem
    (normalizeImageRange fused) on this repo's kernels -- against the nn.Module path (MIOpen), and weights changed by a
    'finetune' are picked up."""
    torch.manual_seed(31)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    tm = torch.rand(5, 4, 124, 124, device="cuda")
    img = torch.rand(1, 3, 480, 640, device="cuda")

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp(min=1e-9))
    with torch.no_grad():
        for trial in range(2):
            if trial == 1:       # same storage, new values
                net.template_feature_extractor.backbone_1[2].squeeze.weight.mul_(1.3)
                net.template_feature_extractor_global.final_conv_2.bias.add_(0.05)
                net.image_feature_extractor.backdense_0[0].weight.mul_(0.9)
                net.image_feature_extractor.backdense_1[0].bias.add_(0.1)
            loc, glob = net.compute_template_local(tm), net.compute_template_global(tm[:1])
            feat = net._features(img, glob, raw_image=True)
            net.use_fused_templates = False
            loc_r, glob_r = net.compute_template_local(tm), net.compute_template_global(tm[:1])
            net.use_fused_templates = True
            net.use_fused_backbone = False
            feat_r = net._features(img, glob, raw_image=True)
            net.use_fused_backbone = True
            assert loc.shape == (5, 640, 7, 7) and glob.shape == (1, 64, 3, 3) and feat.shape == (1, 640, 29, 39)
            assert rel(loc, loc_r) < 1e-4 and rel(glob, glob_r) < 1e-4 and rel(feat, feat_r) < 1e-4, trial
    # and the whole test-time call goes through them (raw image in, template cache filled by the fused encoders)
    m = dtoid.DtoidNet(dtoid.DtoidConfig()).cuda().eval()
    test = {"img": img, "obj_id": torch.tensor([3]), "limg": torch.rand(1, 4, 3, 124, 124).cuda(),
            "lmask": (torch.rand(1, 4, 1, 124, 124) > 0.5).float().cuda()}
    out = m.forwardTestTime(test)
    assert out["pred_bbox"].shape[1] == 4 and "_fused_tfe_local" in m.model.__dict__


def _encoder_decisions(mod, sv):
    """The ReLU masks and max-pool argmaxes of one _encoder_forward run, named as tests/ref_squeezenet.py names them: a ReLU
    decided "on" where its saved output is > 0 (what mask_mode 3 reads in backward), a pool by its saved uint8 argmax."""
    B = sv["cols"].shape[0]
    dec = {"stem": (sv["x0"] > 0).cpu()}
    names = ["%s.%d" % (part, j) for part in ("backbone_1", "backbone_2") for j, m in enumerate(mod.get_submodule(part))
             if not isinstance(m, torch.nn.ReLU)]
    assert len(names) == len(sv["stages"])
    for name, st in zip(names, sv["stages"]):
        if st[0] == "pool":
            _, (C, H, W, k, stride, pad, Ho, Wo), idx = st
            dec[name] = idx.view(B, Ho, Wo, C).permute(0, 3, 1, 2).long().cpu()
        else:
            _, m, x_in, s, out, _ = st
            dec[name + ".squeeze"], dec[name + ".expand"] = (s > 0).cpu(), (out > 0).cpu()
    return dec


# Bounds of the template-encoder training node against the float64 restatement on the node's own decisions (max |error|
# relative to max |float64 value|), with the maxima measured over all eight parametrizations x three rounds. The gradient
# bound is 2.5x the single-launch weight-gradient bound of tests/test_encoder_train_gpu.py (4e-5): a gradient in front of
# eight Fire modules has been through ~25 split-bf16 data-gradient launches and BatchNorm backward passes before its own.
NODE_TAU = 1e-4                 # a decision whose float64 margin is above NODE_TAU x its layer's scale must agree (all did)
NODE_OUT = 5e-5                 # output                        (measured 1.8e-5)
NODE_GRAD = 1e-4                # every parameter gradient      (measured 4.5e-5)
NODE_RUNNING = 4.5e-6           # running mean / var            (measured 1.6e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["local", "global"])
@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("B", [3, 8])
def test_template_encoder_training_node_matches_module_path(hiplib, which, replay, B, monkeypatch):
    """D2 / D3 in TRAINING mode (models/dtoid/network.py:223-239, :265-279): TemplateEncoderTrain -- one autograd node per
    SqueezeNet encoder on this repo's kernels -- against float64 and against the nn.Module path (MIOpen) on the same
    weights: output, every parameter gradient, every BatchNorm running statistic, three rounds with fresh templates, at
    B = 3 and at the finetune step's B = 8. With `replay` round 0 records the launch sequences and rounds 1 and 2 replay
    them from the persistent buffers (a launch missing from the recording, or a torch kernel inside it, would leave round 1
    with round 0's values).

    Float64 (tests/ref_squeezenet.py), hard in every round: ~2 M ReLU / max-pool decisions per pass mean some decision
    always lies within float32 rounding of its kink, and a float32 path that lands it differently is as right as float64's
    own choice. So the node's decisions are read back -- from a companion call of _encoder_forward / _encoder_backward that
    must reproduce the node bit for bit, so they provably are the decisions of the run under test -- and (1) every decision
    whose float64 margin exceeds NODE_TAU x its layer's scale must agree with float64's, (2) the restatement run ON those
    decisions is the float64 value of the very function the node differentiated, to which output, gradients and running
    statistics are held by max-abs relative bounds. The module path is held to its old bounds (relative L2: a flipped
    decision on ITS side moves whole gradients)."""
    import copy
    import ref_squeezenet as R
    from ossid_code_amd.dtoid import train_encoders as TE
    from ossid_code_amd.dtoid import train_ops
    monkeypatch.setattr(train_ops, "SEQ_REPLAY", replay)
    torch.manual_seed(17)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().train()
    mod = net.template_feature_extractor if which == "local" else net.template_feature_extractor_global
    with torch.no_grad():
        # He initialisation + visible biases: with torch's default init the activations of this 18-convolution stack collapse
        # to per-channel constants by the 7x7 stage, and gradients in front of the BatchNorms become pure cancellation noise
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.normal_(1, 0.2)
                m.bias.normal_(0, 0.2)
            elif isinstance(m, torch.nn.Conv2d):
                torch.nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                m.bias.normal_(0, 0.1)
    ref = copy.deepcopy(mod)
    mod_off = copy.deepcopy(mod)              # this repo's node again, with the weight gradients on the main stream
    mod_dec = copy.deepcopy(mod)              # ... and its forward / backward called directly, to read the decisions
    monkeypatch.setattr(train_ops, "WGRAD_SIDE", True)
    gen = torch.Generator().manual_seed(29 + B)
    used = {id(p) for p in TE.encoder_params(mod)}

    def l2(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).norm() / b.norm().clamp(min=1e-30))

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))
    for rnd in range(3):
        img = (torch.rand(B, 4, 124, 124, generator=gen) * (0.5 + 0.5 * rnd)).cuda()
        for m in (mod, ref, mod_off):
            for p in m.parameters():
                p.grad = None
        start = {n: b.detach().clone() for n, b in mod.named_buffers()}
        y_ref = ref(img)
        go = torch.randn(y_ref.shape, generator=gen).cuda()
        y_ref.backward(go)
        y = TE.template_encoder_train(mod, img)
        y.backward(go)
        # WGRAD_SIDE only moves the weight-gradient launches to another stream: the same node with it off must give every bit
        monkeypatch.setattr(train_ops, "WGRAD_SIDE", False)
        y_off = TE.template_encoder_train(mod_off, img)
        y_off.backward(go)
        monkeypatch.setattr(train_ops, "WGRAD_SIDE", True)
        train_ops.join_wgrad_stream()
        out_d, sv = TE._encoder_forward(mod_dec, ops.im2col_stem(img, 3, 2, 0, TE.STEM_KPAD))
        grads_d = TE._encoder_backward(mod_dec, go.float().clone(memory_format=torch.channels_last), sv, side=False)
        torch.cuda.synchronize()
        assert torch.equal(y, y_off), rnd
        for (n, p), q in zip(mod.named_parameters(), mod_off.parameters()):
            assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), (rnd, n)
        assert torch.equal(out_d, y), rnd
        for p, gd in zip(TE.encoder_params(mod), grads_d):
            assert torch.equal(gd, p.grad), rnd
        assert y.shape == y_ref.shape == ((B, 640, 7, 7) if which == "local" else (B, 64, 3, 3))
        # float64 on its own decisions (margins), then on the node's
        free = R.encoder_train(mod, img, go, buffers=start)
        dec = _encoder_decisions(mod_dec, sv)
        assert sorted(dec) == sorted(free["decisions"])
        inside, n_dec, differ = 0, 0, {}
        for k, d in dec.items():
            far = free["margin"][k] > NODE_TAU * free["scale"][k]
            inside += int((~far).sum())
            n_dec += d.numel()
            n_diff = int((far & (d != free["decisions"][k])).sum())
            if n_diff:
                differ[k] = n_diff
        assert not differ, (rnd, "decisions beyond tau that differ, by layer: %s" % differ,
                            "%d of %d decisions inside tau" % (inside, n_dec))
        pin = R.encoder_train(mod, img, go, decisions=dec, buffers=start)
        errs = {"out": rel(y, pin["out"])}
        for n, p in mod.named_parameters():
            if id(p) not in used:
                assert p.grad is None and n not in pin["grads"], n      # the SqueezeNet classifier / 3-channel stem never run
                continue
            assert p.grad is not None and p.grad.shape == p.shape, n
            errs[n] = rel(p.grad, pin["grads"][n])
        for (n, b), q in zip(mod.named_buffers(), ref.buffers()):
            if b.dtype.is_floating_point:
                errs[n] = rel(b, pin["running"][n])
                assert l2(b, q) < 1e-4, (rnd, n)
            else:
                assert int(b) == int(q), (rnd, n)
        e_out = errs.pop("out")
        e_run = max((v, n) for n, v in errs.items() if "running" in n)
        e_grad = max((v, n) for n, v in errs.items() if "running" not in n)
        print("node %s B=%d replay=%d round %d: %d of %d decisions inside tau; out %.2e, grad %.2e (%s), running %.2e (%s)"
              % (which, B, replay, rnd, inside, n_dec, e_out, e_grad[0], e_grad[1], e_run[0], e_run[1]))
        assert e_out < NODE_OUT and e_grad[0] < NODE_GRAD and e_run[0] < NODE_RUNNING, (rnd, e_out, e_grad, e_run)
        # the module path (MIOpen, its own float32 decisions)
        assert l2(y, y_ref) < 2e-4, rnd
        assert l2(y, free["out"]) < max(2e-5, 3 * l2(y_ref, free["out"])), (rnd, l2(y, free["out"]), l2(y_ref, free["out"]))


@pytest.mark.gpu
def test_finetune_step_with_stem_and_template_encoders_on_own_kernels(hiplib):
    """The whole step with the stem and both SqueezeNet encoders on this repo's kernels vs the same step with them on the
    nn.Module path (MIOpen): same loss on the first step, finite and decreasing afterwards."""
    cfg = dtoid.DtoidConfig()
    losses = {}
    for own in (False, True):
        torch.manual_seed(4)
        m = dtoid.DtoidNet(cfg).cuda().train()
        m.model.use_hip_stem_training = m.model.use_hip_template_training = own
        flat = finetune.FlatParams(m)
        opt = finetune.FusedAMSGrad(flat, lr=1e-4, weight_decay=1e-6)
        batch = _batch(cfg, 2, "cuda", seed=3)
        losses[own] = [float(finetune.finetune_step(m, batch, opt)) for _ in range(3)]
    assert abs(losses[True][0] - losses[False][0]) <= 2e-4 * abs(losses[False][0])
    assert all(np.isfinite(losses[True])) and losses[True][-1] < losses[True][0]


@pytest.mark.gpu
def test_side_streams_do_not_change_the_finetune_step(hiplib, monkeypatch):
    """Weight gradients on the side stream (train_ops.WGRAD_SIDE) and the independent branches on theirs
    (Network.use_train_streams) only reorder launches. Since round 4 no library kernel is left in the step, so each
    configuration is BIT-reproducible run to run -- which is what rules out a race (a missing join or a recycled buffer would
    differ from run to run, or by O(1)). Between the one-stream and the multi-stream step the only difference left is the
    ORDER in which autograd adds the gradients that meet at a tensor (the forks create the nodes in another order): 2-3e-5 of
    the whole gradient, measured (tools/tmp history in DESIGN.md 5f). Parameters are frozen (no optimizer step) so that this
    rounding is not amplified by the chaotic small-batch training trajectory; four passes = record, two replays, and the first
    batch again. The gradient is read straight after a bare loss.backward(): only the autograd-engine callback joins the
    weight-gradient stream."""
    from ossid_code_amd.dtoid import train_ops
    cfg = dtoid.DtoidConfig()
    results = []
    for streams in (False, False, True, True):
        monkeypatch.setattr(train_ops, "WGRAD_SIDE", streams)
        torch.manual_seed(6)
        m = _condition_encoders(dtoid.DtoidNet(cfg).cuda().train())
        with torch.no_grad():   # the zero-initialised output layers would make the trunks' gradients exactly zero
            for conv in (m.model.classification.output, m.model.regression.output, m.model.correlation_model.seg_final,
                         m.model.correlation_model.corr_conv_heatmap):
                conv.weight.normal_(0, 0.02)
        m.model.use_train_streams = streams
        flat = finetune.FlatParams(m)
        per = []
        for seed in (0, 1, 2, 0):
            out = m(_batch(cfg, 4, "cuda", seed=seed))
            flat.detach_grads()
            out["loss"].backward()                             # no finetune_step around it
            flat.gather_grads()
            per.append((float(out["loss"]), flat.used_grad().double().cpu()))
        results.append(per)
    one, one_again, multi, multi_again = results
    for i in range(4):
        assert one[i][0] == one_again[i][0] and torch.equal(one[i][1], one_again[i][1]), i          # bit-reproducible
        assert multi[i][0] == multi_again[i][0] and torch.equal(multi[i][1], multi_again[i][1]), i  # ... with the streams too
        assert abs(multi[i][0] - one[i][0]) <= 1e-6 * abs(one[i][0]), i
        d = float((multi[i][1] - one[i][1]).norm() / one[i][1].norm())
        assert d < 2e-4, (i, d)
        assert float(multi[i][1].abs().max()) > 0
    assert torch.equal(one[3][1], one[0][1]) and torch.equal(multi[3][1], multi[0][1])      # same batch, same weights: same bits


@pytest.mark.gpu
def test_head_remainder_kernels_match_torch(hiplib):
    """The last library calls of the correlation head as own kernels (csrc/dtoid.hip, D6): nn.Conv2d(C, 1, 1) forward (with the
    fused sigmoid) and its three gradients, F.avg_pool2d over the whole 7x7 window forward / backward in both memory formats,
    and the few-row matrix product -- against float64 torch on the CPU; run-to-run bit-stable."""
    import torch.nn.functional as F
    from ossid_code_amd.dtoid import train_ops as T
    g = torch.Generator().manual_seed(77)

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))
    for (B, C, H, W) in ((3, 512, 29, 39), (2, 16, 5, 7), (21, 512, 29, 39)):
        conv = torch.nn.Conv2d(C, 1, 1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(1, C, 1, 1, generator=g) * 0.1)
            conv.bias.fill_(-0.3)
        x = torch.randn(B, C, H, W, generator=g)
        c64 = torch.nn.Conv2d(C, 1, 1).double()
        c64.load_state_dict(conv.state_dict())
        x64 = x.double().requires_grad_(True)
        want = c64(x64)
        go = torch.randn(want.shape, generator=g)
        want.backward(go.double())
        cg = conv.cuda()
        xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        got = T.conv1x1_c1(xg, cg)
        got.backward(go.cuda())
        assert rel(got, want) < 1e-5 and rel(xg.grad, x64.grad) < 1e-6
        assert rel(cg.weight.grad, c64.weight.grad) < 1e-5 and rel(cg.bias.grad, c64.bias.grad) < 1e-5
        with torch.no_grad():
            sg = ops.conv1x1_c1(xg.detach(), cg, sigmoid=True)
            assert rel(sg, torch.sigmoid(want)) < 1e-5
            assert torch.equal(sg, ops.conv1x1_c1(xg.detach(), cg, sigmoid=True))
    for cl in (False, True):
        x = torch.randn(5, 640, 7, 7, generator=g)
        x64 = x.double().requires_grad_(True)
        want = F.avg_pool2d(x64, 7)
        go = torch.randn(want.shape, generator=g)
        want.backward(go.double())
        xg = x.cuda()
        if cl:
            xg = xg.contiguous(memory_format=torch.channels_last)
        xg.requires_grad_(True)
        got = ops.spatial_mean(xg)
        got.backward(go.cuda())
        assert got.shape == want.shape and rel(got, want) < 1e-6 and rel(xg.grad, x64.grad) < 1e-6
    a, b = torch.randn(21, 640, generator=g), torch.randn(640, 2304, generator=g)
    assert rel(ops.small_matmul(a.cuda(), b.cuda()), a.double() @ b.double()) < 1e-5


@pytest.mark.parametrize("n_t,topk,spread", [(21, 500, 1.0), (3, 5, 1.0), (21, 500, 0.02), (1, 1, 1.0)])
def test_fused_post_processing_equals_the_step_by_step_one(hiplib, n_t, topk, spread, monkeypatch):
    """ossid_detect_post + ossid_detect_emit (decode of the candidates only, top-k on the strided object column, NMS, one
    gather launch) against the step-by-step path (decode of every box, ossid_topk, index, ossid_nms, gathers): the same
    detection list, bit for bit -- also with heavily tied scores (spread 0.02: quantised probabilities) and with boxes that
    overlap enough for NMS to drop most candidates."""
    torch.manual_seed(n_t * 7 + topk)
    net = dtoid.Network(img_size=(480, 640), heatmap_size=(29, 39)).cuda().eval()
    H, W, hh, hw = 480, 640, 29, 39
    A = hh * hw * 24
    cls = torch.rand(n_t, A, 2, device="cuda")
    if spread < 1:
        cls = (cls / spread).round() * spread
    reg = torch.randn(n_t, A, 4, device="cuda") * 0.5
    seg = torch.randn(n_t, 1, H, W, device="cuda")
    heat = torch.rand(n_t, 1, hh, hw, device="cuda")
    outs = {}
    for fused in (False, True):
        monkeypatch.setattr(dtoid.Network, "use_fused_post", fused)
        outs[fused] = net.postprocess(cls, reg, seg, heat, (hh, hw), (H, W), topk, True)
    for a, b in zip(outs[False], outs[True]):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b)
    assert 1 <= outs[True][0].shape[0] <= topk


@pytest.mark.parametrize("B,H,W,kb", [(1, 240, 320, 1), (2, 37, 51, 2), (1, 6, 5, 1), (3, 1, 1, 1)])
def test_stem_tail_with_pool0_in_one_pass_and_pooled_transition_front(hiplib, B, H, W, kb):
    """ossid_stem_tail_pool_nhwc = max-pool(3, 2, 1) of ossid_stem_tail_nhwc, bit for bit (same fmaf chain per modulated pixel,
    a maximum is exact), written into the channel prefix of a wider buffer whose other channels stay untouched;
    ossid_bn_relu_avgpool2_nhwc against avg_pool2d(relu(affine)) in torch (four-term sums: 1e-6)."""
    torch.manual_seed(H * 3 + W)
    C = 64
    x0 = torch.randn(B, C, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
    k = torch.randn(kb, C, 3, 3, device="cuda") * 0.2
    sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.3
    want = ops.maxpool_nhwc(ops.stem_tail(x0, k, sc, sh), 3, 2, 1)
    got = ops.stem_tail_pool(x0, k, sc, sh)
    assert got.shape == want.shape and torch.equal(got, want)
    wide = torch.full((B, C + 32, want.shape[2], want.shape[3]), 7.0, device="cuda").contiguous(memory_format=torch.channels_last)
    ops.stem_tail_pool(x0, k, sc, sh, out=wide)
    assert torch.equal(wide[:, :C], want) and bool((wide[:, C:] == 7.0).all())
    if H >= 2 and W >= 2:
        for stride in (1, 2):
            xw = torch.randn(B, C + 16, H, W, device="cuda").contiguous(memory_format=torch.channels_last)
            ref = torch.nn.functional.avg_pool2d(torch.relu(xw[:, :C] * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)), 2, stride)
            got = ops.bn_relu_avgpool2(xw, C, sc, sh, stride)
            assert got.shape == ref.shape and torch.allclose(got, ref, rtol=1e-6, atol=1e-6)
