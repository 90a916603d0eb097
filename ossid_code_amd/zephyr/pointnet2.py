"""PointNet2SSG -- host-side mirror of zephyr.models.pointnet2.PointNet2SSG.

Reference interface (the class itself lives in the un-vendored `zephyr` package):
  ctor  PointNet2SSG(dim_point, args, num_class=1)   /root/reference/python/ossid/scripts/online_learning.py:212,218,224
  use   .load_state_dict(ckpt['state_dict']); .to(0).eval(); .device; model({"point_x": x})
                                                      scripts/online_learning.py:213-227, utils/zephyr_utils.py:34
The module tree reproduces pointnet2_ops v3.0.0's PointNet2ClassificationSSG (SA_modules.{0,1,2}.mlps.0 =
Sequential(Conv2d 1x1 no-bias, BatchNorm2d, ReLU) x3; fc_layer = Linear/BN1d/ReLU/Linear/BN1d/ReLU/Dropout/
Linear) so a state_dict saved from that architecture loads key for key. The forward pass does not run in
torch: the parameters are folded (BN into the convolution), permuted into SPEC.md's canonical channel order,
packed into the MFMA operand layout of csrc/pn2.hip and handed to libossid_hip.so.

Training mode (SPEC.md 12): forward() of a module in .train() runs csrc/pn2_train.hip through a torch.autograd.Function --
pointnet2_ops' PointnetSAModule / SharedMLP and the classification head with batch-statistics BatchNorm and dropout, in
torch's own channel order -- so `model.train(); loss.backward(); optimizer.step()` fits the module the reference builds at
scripts/online_learning.py:212-227 on this build's features. zephyr's own training recipe is in neither tree: unpinned.
"""
import ctypes
import os

import numpy as np
import torch
import torch.nn as nn

from .. import _lib

BN_EPS = 1e-5
# (kpad, cout) of the 12 dense layers after folding, SPEC.md 4.3
LAYER_K = (8, 64, 64, 136, 128, 128, 264, 256, 512, 1024, 512, 256)
LAYER_C = (64, 64, 128, 128, 128, 256, 256, 512, 1024, 512, 256, 1)


def _shared_mlp(spec):
    layers = []
    for i in range(1, len(spec)):
        layers += [nn.Conv2d(spec[i - 1], spec[i], kernel_size=1, bias=False), nn.BatchNorm2d(spec[i]), nn.ReLU(True)]
    return nn.Sequential(*layers)


class _SAModule(nn.Module):
    """Parameter container shaped like pointnet2_ops.PointnetSAModule (single-scale)."""

    def __init__(self, npoint, radius, nsample, mlp, use_xyz=True):
        super().__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        spec = list(mlp)
        if use_xyz:
            spec[0] += 3
        self.mlps = nn.ModuleList([_shared_mlp(spec)])


def _fold_bn(weight, bn):
    """(W[cout,cin], BN) -> (W * s, beta - mean * s) with s = gamma / sqrt(var + eps); float32 numpy ops."""
    W = weight.detach().cpu().numpy().astype(np.float32).reshape(weight.shape[0], -1)
    gamma = bn.weight.detach().cpu().numpy().astype(np.float32)
    beta = bn.bias.detach().cpu().numpy().astype(np.float32)
    mean = bn.running_mean.detach().cpu().numpy().astype(np.float32)
    var = bn.running_var.detach().cpu().numpy().astype(np.float32)
    s = gamma / np.sqrt(var + np.float32(bn.eps))
    return (W * s[:, None]).astype(np.float32), (beta - mean * s).astype(np.float32)


def fold_pn2(model):
    """12 folded layers [(W'[cout,kpad], b'[cout])] in canonical input-channel order (SPEC.md 4.3)."""
    out = []
    for si, sa in enumerate(model.SA_modules):
        seq = sa.mlps[0]
        for li in range(3):
            W, b = _fold_bn(seq[3 * li].weight, seq[3 * li + 1])
            if li == 0 and si > 0:
                # torch order is (grouped_xyz(3), features(C)); canonical is (features(C), xyz(3), 0-pad to x8)
                C = W.shape[1] - 3
                Wc = np.zeros((W.shape[0], C + 8), np.float32)
                Wc[:, :C] = W[:, 3:]
                Wc[:, C:C + 3] = W[:, :3]
                W = Wc
            out.append((np.ascontiguousarray(W), np.ascontiguousarray(b)))
    fc = model.fc_layer
    out.append(_fold_bn(fc[0].weight, fc[1]))
    out.append(_fold_bn(fc[3].weight, fc[4]))
    out.append((fc[7].weight.detach().cpu().numpy().astype(np.float32).reshape(1, -1),
                fc[7].bias.detach().cpu().numpy().astype(np.float32).reshape(1)))
    for i, (W, b) in enumerate(out):
        assert W.shape == (LAYER_C[i], LAYER_K[i]), (i, W.shape)
    return out


def _pack_mfma(W):
    """W'[cout,kpad] -> [cout/32][kpad/8][64 lanes][4]: lane (c, h) holds W'[32mt+c][8kb+4h+0..3], the A operands
    of the four chained 32x32x2 MFMAs of k-block kb (csrc/pn2.hip)."""
    cout, kpad = W.shape
    return np.ascontiguousarray(W.reshape(cout // 32, 32, kpad // 8, 2, 4).transpose(0, 2, 3, 1, 4)).reshape(-1)


def pack_pn2(folded):
    """Folded layers -> (blob float32[...], w_off[12], b_off[12], wxyz2_off), offsets in floats, 64-float aligned."""
    parts, w_off, b_off = [], [], []
    pos = 0

    def add(a):
        nonlocal pos
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        off = pos
        pad = (-a.size) % 64
        parts.append(a)
        if pad:
            parts.append(np.zeros(pad, np.float32))
        pos += a.size + pad
        return off

    wxyz2_off = 0
    for i, (W, b) in enumerate(folded):
        if i == 3:  # SA2 L1: feature columns on the matrix core, xyz columns applied per sample
            w_off.append(add(_pack_mfma(W[:, :128])))
            wxyz2_off = add(np.stack([W[:, 128], W[:, 129], W[:, 130]], 0))
        elif i <= 8:
            w_off.append(add(_pack_mfma(W)))
        elif i <= 10:  # FC1/FC2 transposed [k][cout]
            w_off.append(add(W.T))
        else:
            w_off.append(add(W))
        b_off.append(add(b))
    return np.concatenate(parts), w_off, b_off, wxyz2_off


class PointNet2SSG(nn.Module):
    MAX_CHUNK = 4096  # hypotheses per C-ABI call (bounds the workspace at ~0.72 MB each)
    # Measured and NOT adopted (round 3, profiles/r03_scorer_overlap.txt): overlapping the sampling kernels (fps / ball query:
    # vector-ALU and LDS work, 6.5 % of the step) with the matrix-core stages INSIDE one call. The sampling stages read
    # coordinates only, so they can run ahead on a side stream -- but the MLP kernels fill the register file and 51-128 KB of LDS
    # per workgroup, so nothing co-resides with them: all a second stream can do is fill the tail of each launch, and cutting
    # one call into pieces adds more tails (and partial rounds: sa3 runs one workgroup per hypothesis, 1000 = 3.9 rounds of
    # 256) than it fills. One call, one stream: 15.19 ms; 4 pieces alternating two streams 15.78; sampling ahead on a side
    # stream in pieces [128, 872] 16.00, [504, 496] 15.55. Two whole FRAMES in flight on two streams (scoring.networkInferenceMany,
    # bench.py's timed region) do gain: 14.67 ms per frame.

    def __init__(self, dim_in, args=None, num_class=1):
        super().__init__()
        if dim_in != 8:
            raise NotImplementedError("the MI355X scorer is built for dim_point=8 (HSVD_diff_uv_norm), got %r" % dim_in)
        if num_class != 1:
            raise NotImplementedError("num_class must be 1 (online_learning.py:212)")
        self.args = args
        self.dim_in = dim_in
        extra = getattr(args, "extra_bottleneck_dim", 0) if args is not None else 0
        if extra:
            raise NotImplementedError("extra_bottleneck_dim must be 0 (online_learning.py:209)")
        self.SA_modules = nn.ModuleList([
            _SAModule(512, 0.2, 64, [dim_in - 3, 64, 64, 128]),
            _SAModule(128, 0.4, 64, [128, 128, 128, 256]),
            _SAModule(None, None, None, [256, 256, 512, 1024]),
        ])
        self.fc_layer = nn.Sequential(
            nn.Linear(1024, 512, bias=False), nn.BatchNorm1d(512), nn.ReLU(True),
            nn.Linear(512, 256, bias=False), nn.BatchNorm1d(256), nn.ReLU(True),
            nn.Dropout(0.5), nn.Linear(256, num_class))
        self._packed = None  # (version key, device blob, PN2Weights)
        self._ws = None

    @property
    def device(self):  # LightningModule attribute the caller reads (utils/zephyr_utils.py:34)
        return next(self.parameters()).device

    def _version_key(self, device):
        return (str(device),) + tuple(int(t._version) for t in list(self.parameters()) + list(self.buffers()))

    def packed_weights(self, device):
        key = self._version_key(device)
        if self._packed is None or self._packed[0] != key:
            blob, w_off, b_off, wxyz2_off = pack_pn2(fold_pn2(self))
            dblob = torch.from_numpy(blob).to(device)
            st = _lib.PN2Weights()
            st.blob = dblob.data_ptr()
            for i in range(12):
                st.w_off[i], st.b_off[i] = w_off[i], b_off[i]
            st.wxyz2_off = wxyz2_off
            st.npoint1, st.npoint2 = self.SA_modules[0].npoint, self.SA_modules[1].npoint
            st.radius1, st.radius2 = self.SA_modules[0].radius, self.SA_modules[1].radius
            self._packed = (key, dblob, st)
        return self._packed[2]

    def _workspace(self, nbytes, device, kind="score"):
        """Grow-only scratch buffer, one per (device, stream): frames in flight on different HIP streams must not
        share stage buffers. The training path's (kind "train") lives from a forward to its backward, apart from the
        inference path's."""
        if self._ws is None:
            self._ws = {}
        key = (str(device), torch.cuda.current_stream(device).cuda_stream) + (() if kind == "score" else (kind,))
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            self._ws[key] = ws
        return ws

    def score(self, point_x, debug=False, stage_events=None):
        """point_x [B, M, 8] float32 on the GPU -> scores [B] (and the stage tensors when debug).
        stage_events: a _lib.StageEvents to time every stage of the call."""
        _lib.require_cuda(point_x)
        if self.training:
            raise NotImplementedError("PointNet2SSG is inference-only on this path: call .eval() "
                                      "(online_learning.py:215,221,227)")
        if point_x.dtype != torch.float32 or point_x.dim() != 3 or point_x.shape[2] != 8:
            raise ValueError("point_x must be float32 [B, M, 8]")
        point_x = point_x.contiguous()
        B, M, _ = point_x.shape
        dev = point_x.device
        w = self.packed_weights(dev)
        np1, np2 = w.npoint1, w.npoint2
        if B and M < np1:
            raise ValueError("need at least npoint=%d model points per hypothesis, got %d" % (np1, M))
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        dbg = None
        if debug:
            i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
            dbg = dict(fps1=torch.empty(B, np1, **i32), ball1=torch.empty(B, np1, 64, **i32),
                       feat1=torch.empty(B, np1, 128, **f32), fps2=torch.empty(B, np2, **i32),
                       ball2=torch.empty(B, np2, 64, **i32), feat2=torch.empty(B, np2, 256, **f32),
                       feat3=torch.empty(B, 1024, **f32))
        f = _lib.fn("ossid_pn2_score")
        wsb = _lib.fn("ossid_pn2_workspace_bytes")
        w_ref = ctypes.byref(w)

        def launch(b0, nb, events):
            nbytes = wsb(nb, M, np1, np2)
            ws = self._workspace(nbytes, dev)
            dargs = [None] * 7
            if dbg is not None:
                dargs = [dbg[k][b0:b0 + nb].data_ptr() for k in ("fps1", "ball1", "feat1", "fps2", "ball2", "feat2", "feat3")]
            rc = f(point_x[b0:b0 + nb].data_ptr(), nb, M, w_ref, ws.data_ptr(), nbytes, scores[b0:b0 + nb].data_ptr(),
                   *dargs, None if events is None else events.arr, _lib.stream())
            _lib.check(rc, "ossid_pn2_score")

        with torch.cuda.device(dev):
            for b0 in range(0, B, self.MAX_CHUNK):
                launch(b0, min(self.MAX_CHUNK, B - b0), stage_events)
        return (scores, dbg) if debug else scores

    def forward(self, data, keep_mask=None, generator=None, debug=None):
        """Eval mode: score(). Training mode (SPEC.md 12): [B, 1] scores with a grad_fn, from csrc/pn2_train.hip.
        keep_mask: the dropout keep-mask, bool / u8 [B, 256] (default: drawn on the host from `generator`, a CPU
        torch.Generator, with the module's p); debug: a dict that receives the decisions the forward took."""
        x = data["point_x"] if isinstance(data, dict) else data
        if not self.training:
            return self.score(x).unsqueeze(1)
        return self.train_forward(x, keep_mask, generator, debug)

    # ---- training path ----------------------------------------------------------------------------------------------
    def train_layers(self):
        """([12 Conv2d / Linear], [11 BatchNorm]) in the kernels' layer order: SA1 x3, SA2 x3, SA3 x3, FC1, FC2, last."""
        lin, bns = [], []
        for sa in self.SA_modules:
            seq = sa.mlps[0]
            for li in range(3):
                lin.append(seq[3 * li])
                bns.append(seq[3 * li + 1])
        fc = self.fc_layer
        return lin + [fc[0], fc[3], fc[7]], bns + [fc[1], fc[4]]

    def draw_keep_mask(self, B, generator=None):
        """u8 [B, 256] on the host: 1 with probability 1 - p."""
        p = float(self.fc_layer[6].p)
        return (torch.rand(B, 256, generator=generator) >= p).to(torch.uint8)

    def train_forward(self, point_x, keep_mask=None, generator=None, debug=None):
        if point_x.dtype != torch.float32 or point_x.dim() != 3 or point_x.shape[2] != 8:
            raise ValueError("point_x must be float32 [B, M, 8]")
        if point_x.requires_grad:
            raise ValueError("no gradient is defined for point_x: the featurizer is not trained (SPEC.md 12)")
        B, M, _ = point_x.shape
        if B < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                             % (torch.Size([B, 512]),))
        np1 = self.SA_modules[0].npoint
        if M < np1:
            raise ValueError("need at least npoint=%d model points per hypothesis, got %d" % (np1, M))
        if keep_mask is None:
            keep_mask = self.draw_keep_mask(B, generator)
        keep_mask = keep_mask.to(device=point_x.device, dtype=torch.uint8).contiguous()
        if keep_mask.shape != (B, 256):
            raise ValueError("keep_mask must be [B, 256]")
        lin, bns = self.train_layers()
        params = [m.weight for m in lin] + [b.weight for b in bns] + [b.bias for b in bns] + [lin[11].bias]
        return _TrainFn.apply(self, point_x.contiguous(), keep_mask, debug, *params)

    def _train_backend_for(self, point_x):
        backend = getattr(self, "_train_backend", None)
        return backend if backend is not None else HipTrainBackend()


class HipTrainBackend:
    """The two C-ABI calls of the training path. A backend is what _TrainFn needs: forward(model, x, W, gamma, beta, bias,
    run_mean, run_var, keep, p, debug) -> (scores [B], state) updating run_mean / run_var in place, and
    backward(state, dscores [B]) -> (dW list, dgamma list, dbeta list, dbias), every gradient in the flat [cout, cin] /
    [C] / [1] layout of the kernels."""

    def forward(self, model, x, W, gamma, beta, bias, run_mean, run_var, keep, p, debug):
        _lib.require_cuda(x, keep, *W)
        dev = x.device
        B, M, _ = x.shape
        np1, np2 = model.SA_modules[0].npoint, model.SA_modules[1].npoint
        st = _lib.PN2TrainParams()
        tensors = [t.contiguous().float() for t in W + gamma + beta + [bias]]
        for i in range(12):
            st.w[i] = tensors[i].data_ptr()
        for i in range(11):
            st.gamma[i], st.beta[i] = tensors[12 + i].data_ptr(), tensors[23 + i].data_ptr()
            st.run_mean[i], st.run_var[i] = run_mean[i].data_ptr(), run_var[i].data_ptr()
        st.bias = tensors[34].data_ptr()
        st.npoint1, st.npoint2 = np1, np2
        st.radius1, st.radius2 = model.SA_modules[0].radius, model.SA_modules[1].radius
        nbytes = _lib.fn("ossid_pn2_train_workspace_bytes")(B, M, np1, np2)
        if nbytes == 0:
            raise ValueError("the training path refuses B=%d, M=%d, npoint=%d/%d (SPEC.md 12)" % (B, M, np1, np2))
        ws = model._workspace(nbytes, dev, kind="train")
        scores = torch.empty(B, dtype=torch.float32, device=dev)
        dbg = None
        if debug is not None:
            C = LAYER_C[:11]
            rows = [B * np1 * 64] * 3 + [B * np2 * 64] * 3 + [B * np2] * 3 + [B] * 2
            i32, u8 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.uint8, device=dev)
            debug.update(relu=[torch.empty(r, c, **u8) for r, c in zip(rows, C)],
                         argmax=[torch.empty(B, np1, 128, **i32), torch.empty(B, np2, 256, **i32), torch.empty(B, 1, 1024, **i32)],
                         fps1=torch.empty(B, np1, **i32), ball1=torch.empty(B, np1, 64, **i32),
                         fps2=torch.empty(B, np2, **i32), ball2=torch.empty(B, np2, 64, **i32))
            dbg = _lib.PN2TrainDbg()
            for i in range(11):
                dbg.relu[i] = debug["relu"][i].data_ptr()
            for i in range(3):
                dbg.argmax[i] = debug["argmax"][i].data_ptr()
            for k in ("fps1", "ball1", "fps2", "ball2"):
                setattr(dbg, k, debug[k].data_ptr())
        with torch.cuda.device(dev):
            rc = _lib.fn("ossid_pn2_train_forward")(x.data_ptr(), B, M, ctypes.byref(st), keep.data_ptr(), float(p),
                                                    ws.data_ptr(), nbytes, scores.data_ptr(),
                                                    None if dbg is None else ctypes.byref(dbg), _lib.stream())
        _lib.check(rc, "ossid_pn2_train_forward")
        return scores, (st, tensors, ws, nbytes, B, M, float(p), dev)

    def backward(self, state, dscores):
        st, tensors, ws, nbytes, B, M, p, dev = state
        grads = [torch.empty_like(t) for t in tensors]
        g = _lib.PN2TrainGrads()
        for i in range(12):
            g.w[i] = grads[i].data_ptr()
        for i in range(11):
            g.gamma[i], g.beta[i] = grads[12 + i].data_ptr(), grads[23 + i].data_ptr()
        g.bias = grads[34].data_ptr()
        dscores = dscores.contiguous().float()
        with torch.cuda.device(dev):
            rc = _lib.fn("ossid_pn2_train_backward")(dscores.data_ptr(), B, M, ctypes.byref(st), p, ws.data_ptr(), nbytes,
                                                     ctypes.byref(g), _lib.stream())
        _lib.check(rc, "ossid_pn2_train_backward")
        return grads[:12], grads[12:23], grads[23:34], grads[34]


class _TrainFn(torch.autograd.Function):
    """Scores of the training-mode forward as a function of the 35 parameters (12 weights, 11 gamma, 11 beta, the last bias).
    point_x gets no gradient. The running statistics are updated through copy_ from staging tensors, so the buffers' version
    counters move and the inference path's packed-weight cache (PointNet2SSG._version_key) sees the change."""

    @staticmethod
    def forward(ctx, model, point_x, keep, debug, *params):
        lin, bns = model.train_layers()
        backend = model._train_backend_for(point_x)
        W = [p.detach().reshape(p.shape[0], -1) for p in params[:12]]
        gamma, beta, bias = [p.detach() for p in params[12:23]], [p.detach() for p in params[23:34]], params[34].detach()
        stage = torch.cat([b.running_mean for b in bns] + [b.running_var for b in bns]).to(torch.float32)
        sizes = [b.num_features for b in bns]
        parts = list(torch.split(stage, sizes + sizes))
        scores, state = backend.forward(model, point_x, W, gamma, beta, bias, parts[:11], parts[11:], keep,
                                        float(model.fc_layer[6].p), debug)
        for b, m, v in zip(bns, parts[:11], parts[11:]):
            b.running_mean.copy_(m)
            b.running_var.copy_(v)
            b.num_batches_tracked.add_(1)
        model._train_gen = getattr(model, "_train_gen", 0) + 1
        ctx.model, ctx.backend, ctx.state, ctx.gen = model, backend, state, model._train_gen
        ctx.shapes = [p.shape for p in params]
        return scores.unsqueeze(1)

    @staticmethod
    def backward(ctx, dscores):
        if ctx.state is None or ctx.gen != ctx.model._train_gen:
            raise RuntimeError("PointNet2SSG's training workspace holds one forward pass and its backward runs in place: "
                               "call backward once, before the next training-mode forward")
        dW, dgamma, dbeta, dbias = ctx.backend.backward(ctx.state, dscores[:, 0])
        ctx.state = None
        flat = list(dW) + list(dgamma) + list(dbeta) + [dbias]
        grads = [g.reshape(s) if need else None for g, s, need in zip(flat, ctx.shapes, ctx.needs_input_grad[4:])]
        return (None, None, None, None) + tuple(grads)
