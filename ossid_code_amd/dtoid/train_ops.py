"""Training-mode (finetune) execution of the DTOID convolutions on the hand-written kernels, channels-last end to end.

Reference step being reproduced: scripts/online_learning.py:650-679 (`model.train(); out = model(batch);
out['loss'].backward(); optimizer.step()`) over models/dtoid/network.py:439-471. What is MI355X-specific:

  * every 3x3 / 1x1 convolution runs forward, data gradient and weight gradient on the f32 matrix cores
    (csrc/conv.hip, csrc/train.hip), exact f32, on [B][H][W][C] tensors -- no NCHW<->NHWC transposes;
  * training-mode BatchNorm never materialises its output: batch statistics are column sums of the producer's output
    (`ossid_chan_op`), folded with gamma / beta into a per-channel (scale, shift) (`ossid_bn_fold_fwd`) that the NEXT
    convolution applies -- with the ReLU -- while it stages its input. In a dense block the statistics of a feature
    channel are computed ONCE, when the channel is produced, and shared by every later layer (they all normalise the
    same values): O(L) reductions instead of DenseNet's O(L^2);
  * backward passes are the same few kernels: ELU' / ReLU masks, the BatchNorm-statistics gradient and the bias /
    scale / shift reductions are all instances of one generic pass (`ossid_chan_op`); a dense block keeps ONE gradient
    buffer and every layer accumulates into its channel prefix in place.

autograd sees a handful of coarse Functions (FusedConv, BNFold, ColStats, AvgPool2, DenseBlockTrain); tensors are
logical NCHW in torch.channels_last memory format, so torch ops (losses, the few layers left on MIOpen) interoperate.
"""
import ctypes

import torch

from .. import _lib

_byref = ctypes.byref


def nhwc(x):
    return x.float().contiguous(memory_format=torch.channels_last)


def empty_nhwc(B, C, H, W, device):
    return torch.empty((B, C, H, W), dtype=torch.float32, device=device, memory_format=torch.channels_last)


def flat(t, offset=0):
    """1-D alias of a channels-last tensor's memory ([B][H][W][C] order), from element `offset` on: how a channel
    slice of a wider buffer is handed to the raw ops (pointer to its first element + the buffer's channel stride)."""
    v = t.permute(0, 2, 3, 1).reshape(-1)
    assert v.data_ptr() == t.data_ptr(), "expected a dense channels-last tensor"
    return v[offset:]


# ---- scratch: column-sum partials, split-K slabs ------------------------------------------------------------------------
# Eager launches share one grow-only buffer per (purpose, device, stream): launches on one stream are ordered, so the next
# user finds the previous one done. A RECORDED launch sequence owns its scratch instead (_lib.Seq.scratch, per stream slot):
# the addresses are baked into the recorded arguments, and a replay runs on whatever stream is current THEN -- two sequences
# recorded on one stream (a capture's warm-up, a step with the branches off) and replayed side by side on the branch streams
# would otherwise write the same partials buffer.
_SCRATCH = {}


def _scratch(name, nbytes, device):
    rec = _lib.recording()
    if rec is not None:
        return rec.scratch(name, nbytes, device)
    key = (name, str(device), _lib.stream())
    t = _SCRATCH.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _SCRATCH[key] = t
    return t


# Where a parameter's gradient finally lives (finetune.FlatParams' slice of the flat gradient buffer), by the parameter's
# address. A weight-gradient kernel may write there directly -- saving the per-step copy of the 34 M convolution weights'
# gradients into the flat buffer -- exactly when autograd will TAKE the returned tensor as p.grad without reading it, i.e.
# while p.grad is None (the finetune_step protocol); with a gradient already in place (`p.grad += dw` on the very same
# memory) it must not. Weak values: the views die with their FlatParams.
import weakref                                                        # noqa: E402

_GRAD_HOME = weakref.WeakValueDictionary()


def register_grad_home(param, view):
    _GRAD_HOME[(param.data_ptr(), tuple(param.shape))] = view


def grad_home(w, direct):
    """The tensor a weight-gradient kernel for parameter `w` should write: w's slice of the flat gradient buffer when
    `direct` (the caller established that w.grad is None, see above) and one is registered, else a fresh buffer."""
    if direct:
        v = _GRAD_HOME.get((w.data_ptr(), tuple(w.shape)))
        if v is not None and v.device == w.device:
            return v
    return new_buf(w.shape, w.device)


def new_buf(shape, device, zero=False, channels_last=False):
    """A float32 work buffer of the raw ops. Inside a recorded launch sequence (_lib.record) the sequence keeps it alive --
    its address is baked into the recorded arguments -- and `zero` becomes a recorded ossid_fill_zero, so that every
    replay starts from a cleared buffer (torch.zeros would clear it at record time only)."""
    if channels_last:
        t = torch.empty(tuple(shape), dtype=torch.float32, device=device, memory_format=torch.channels_last)
    else:
        t = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    rec = _lib.recording()
    if rec is not None:
        rec.keep(t)
    if zero:
        with _lib.on_device(device):
            _lib.check(_lib.fn("ossid_fill_zero")(t.data_ptr(), t.numel() * 4, _lib.stream()), "ossid_fill_zero")
    return t


# ---- raw ops (no autograd) --------------------------------------------------------------------------------------------
def chan_op(g, n_rows, C, x=None, out=None, g_cs=0, x_cs=0, out_cs=0, alpha=None, beta=None, kappa=None, mask_mode=0,
            mask_scale=None, mask_shift=None, accumulate=False, sum_mode=0, sums=None, sums_row_stride=0, defer=False,
            pivot=None):
    """include/ossid_hip.h ossid_chan_op on raw channels-last buffers (tensors only provide pointers; a tensor that is a
    channel slice of a wider buffer is passed as its first-element pointer + the buffer's channel count as stride).
    Returns `sums` ([2, C] float32, allocated when sum_mode != 0 and none was given). defer=True: the column sums stay
    as per-block partials in a scratch buffer and (scratch, P) is returned for bn_fold_fwd / bn_fold_bwd to combine --
    valid until the next deferred chan_op on this stream."""
    d = _lib.ChanOpDesc()
    dev = g.device
    d.g, d.x, d.out = g.data_ptr(), dptr(x), dptr(out)
    d.alpha, d.beta, d.kappa, d.mask_scale, d.mask_shift = dptr(alpha), dptr(beta), dptr(kappa), dptr(mask_scale), dptr(mask_shift)
    d.pivot = dptr(pivot)
    d.n_rows, d.channels, d.g_stride, d.x_stride, d.out_stride = int(n_rows), int(C), int(g_cs), int(x_cs), int(out_cs)
    d.mask_mode, d.accumulate, d.sum_mode, d.sums_row_stride = int(mask_mode), 1 if accumulate else 0, int(sum_mode), int(sums_row_stride)
    if sum_mode:
        P = _lib.fn("ossid_chan_op_partials")(int(n_rows), int(C))
        if defer:
            part = _scratch("chan_defer", P * 2 * C * 4, dev)
            d.partials, d.defer_finalize = part.data_ptr(), 1
            sums = (part, P)
        else:
            if sums is None:
                sums = new_buf((3 if sum_mode == 3 else 2, C), dev)
            d.partials = _scratch("chan", P * 2 * C * 4, dev).data_ptr()
            d.sums = sums.data_ptr()
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_chan_op")(_byref(d), _lib.stream()), "ossid_chan_op")
    return sums


def batch_stats(x_flat, n_rows, C, cs=0, sums=None, sums_row_stride=0, defer=False):
    """Column sums of a channels-last tensor (or channel slice: pointer to its first element + channel stride) for a
    training BatchNorm, taken about the tensor's FIRST ROW as pivot (sum_mode 3): [3, C] = (sum (x - p), sum (x - p)^2, p).
    defer=True: (partials, P, pivot pointer tensor) for bn_fold_fwd to finish."""
    res = chan_op(x_flat, n_rows, C, g_cs=cs, sum_mode=3, pivot=x_flat, sums=sums, sums_row_stride=sums_row_stride, defer=defer)
    return res + (x_flat,) if defer else res


class _Packed:
    """Per-weight-tensor device buffers for the MFMA operand layouts (forward and data-gradient), re-filled every step
    IN PLACE (the step is captured in a hipGraph: addresses must not change)."""
    _cache = {}

    @classmethod
    def get(cls, w, kind):
        key = (w.data_ptr(), tuple(w.shape), kind)
        ent = cls._cache.get(key)
        if ent is None:
            cout, cin = int(w.shape[0]), int(w.shape[1])
            taps = int(w.shape[2] * w.shape[3])
            if kind in ("wino_fwd", "wino_dgrad"):
                n = _lib.fn("ossid_conv_wino_packed_floats")(*((cout, cin) if kind == "wino_fwd" else (cin, cout)))
            else:
                form = _KIND_FORM[kind]
                n = _lib.fn("ossid_conv_packed_floats_form")(cout, cin, taps, form) if kind.startswith("fwd") else \
                    _lib.fn("ossid_conv_packed_floats_form")(cin, cout, taps, form)
            if len(cls._cache) > 4096:
                cls.clear()
            ent = cls._cache[key] = torch.empty(n, dtype=torch.float32, device=w.device)
            ent._ossid_exact = _KIND_FORM.get(kind, 0)      # conv_raw sets ossid_conv_desc.exact from the buffer it is handed
        return ent

    @classmethod
    def clear(cls):
        """Forget every packed buffer. A live PackPlan keeps its own buffers alive (PackPlan.bufs) but is no longer
        `valid_for` anything (its buffers are not the cache's any more) and nothing it packed counts as fresh."""
        global _ACTIVE_PLAN
        cls._cache.clear()
        _ACTIVE_PLAN = None


_ACTIVE_PLAN = None  # weakref to the PackPlan that packed last. Its `fresh` dict maps (weight pointer, shape, kind) -> the
#                      weight's version counter at that moment: _pack() skips its own launch while the weight has not been
#                      written since. The plan holds its weights strongly, so while it lives their addresses cannot be
#                      recycled for other tensors; when its network dies the weakref dies with it and nothing is "fresh".


# ossid_conv_desc::exact of each direct-kernel layout (include/ossid_hip.h): 0 split-bf16, 1 exact-f32 instruction, 2 three-way split
_KIND_FORM = {"fwd": 0, "dgrad": 0, "fwd_exact": 1, "dgrad_exact": 1, "fwd_x6": 2}
# The forward layout of layers whose output a ReLU / max-pool decides on: f32-level accuracy is needed (a pre-activation on the
# other side of zero changes the gradient's path) -- the three-way split delivers it at 2x the split form's
# matrix-pipe time instead of 5x ("fwd_exact" would put these layers on the exact-f32 instruction). Data gradients and the ELU
# head run split-bf16.
FWD_DECIDING = "fwd_x6"
# The two SqueezeNet template encoders keep the exact-f32 instruction: their convolutions are small (0.3 ms of the step), and
# with ~2 M ReLU / max-pool decisions per pass ANY f32-level path lands one of them differently from torch's in some passes
# (2e-3 .. 1e-2 on the gradients in front of it instead of 2e-5: measured in round 3, one pass in six with the exact
# instruction, three in six with the three-way split) -- the tests' bound is calibrated on the exact one.
FWD_ENCODER = "fwd_exact"


def _pack(w, kind):
    """kind: "fwd" / "dgrad" (split-bf16 launches), "fwd_exact" / "dgrad_exact" (exact-f32 launches), "fwd_x6" (three-way
    split), "wino_fwd" / "wino_dgrad"."""
    w = w.detach()
    assert w.is_contiguous() and w.dtype == torch.float32
    cout, cin, taps = int(w.shape[0]), int(w.shape[1]), int(w.shape[2] * w.shape[3])
    buf = _Packed.get(w, kind)
    plan = _ACTIVE_PLAN() if _ACTIVE_PLAN is not None else None
    key = (w.data_ptr(), tuple(w.shape), kind)
    if plan is not None and plan.fresh.get(key) == w._version and plan.buf_ptr.get(key) == buf.data_ptr():
        return buf
    if plan is not None and key[0] in plan.weight_ptrs:
        plan.misses.add((key[0], kind))          # a layout the plan did not foresee: whoever owns the plan adds it (next step)
    with _lib.on_device(w.device):
        if kind in ("wino_fwd", "wino_dgrad"):
            name = "ossid_conv_pack_weights_wino"
            _lib.check(_lib.fn(name)(w.data_ptr(), cout, cin, 1 if kind == "wino_dgrad" else 0, buf.data_ptr(), _lib.stream()), name)
        else:
            name = "ossid_conv_pack_weights_form"
            _lib.check(_lib.fn(name)(w.data_ptr(), cout, cin, taps, 1 if kind.startswith("dgrad") else 0,
                                     _KIND_FORM[kind], buf.data_ptr(), _lib.stream()), name)
    return buf


class PackPlan:
    """All convolution weights of the training step re-packed (forward + data-gradient layouts) by ONE launch at the top
    of the forward pass instead of two small launches per layer. Built once per set of weight tensors (their addresses
    are stable: FlatParams views); `run()` marks them fresh so the per-layer _pack() calls only look the buffers up."""

    def __init__(self, convs, kinds=None, split_at=None):
        """kinds: optional {conv: tuple of layouts} -- which of ("fwd", "fwd_exact", "dgrad", "wino_fwd", "wino_dgrad") the step will ask
        for (a layout left out is simply packed by its layer's own _pack() launch if it is asked for after all).
        split_at: the first `split_at` convolutions are packed by a launch of their own, in front of the rest (run() can
        hand back an event between the two: what the step needs first -- the backbone, 7 of the 34 M weights -- is ready
        after a fifth of the packing time)."""
        rows, keys = [], []
        self.bufs, self.buf_ptr = [], {}       # strong references: the tables below hold raw addresses of these buffers
        # split_at: one index, or an increasing sequence of them (one launch per segment of the list)
        cuts = [] if split_at is None else ([int(split_at)] if isinstance(split_at, int) else [int(c) for c in split_at])
        parts = [[] for _ in range(len(cuts) + 1)]
        firsts = [0] * (len(cuts) + 1)
        for ci, conv in enumerate(convs):
            part = sum(1 for c in cuts if ci >= c)
            w = conv.weight.detach()
            cout, cin, taps = int(w.shape[0]), int(w.shape[1]), int(w.shape[2] * w.shape[3])
            for kind in (("fwd", "dgrad") if kinds is None else kinds.get(conv, ("fwd", "dgrad"))):
                if kind in ("dgrad", "dgrad_exact") and cout % 16:
                    continue
                if kind.startswith("fwd") and (cin % 16 or cout % 4):
                    continue
                if kind == "wino_fwd" and not (USE_WINO and taps == 9 and cin % 16 == 0 and cout >= 64):
                    continue
                if kind == "wino_dgrad" and not (USE_WINO and taps == 9 and cout % 16 == 0 and cin >= 64):
                    continue
                buf = _Packed.get(w, kind)
                parts[part].append((w.data_ptr(), buf.data_ptr(), firsts[part], cout, cin, taps,
                                    {"fwd": 0, "dgrad": 1, "wino_fwd": 2, "wino_dgrad": 3, "fwd_exact": 4, "dgrad_exact": 5, "fwd_x6": 6}[kind]))
                keys.append((w.data_ptr(), tuple(w.shape), kind))
                self.bufs.append(buf)
                self.buf_ptr[keys[-1]] = buf.data_ptr()
                firsts[part] += (buf.numel() // 4 + 255) // 256
        self.device = convs[0].weight.device
        self.tables = []                       # (device table, rows, blocks) per launch
        for rows, blocks in zip(parts, firsts):
            if not rows:
                continue
            arr = (_lib.PackRow * len(rows))()
            for i, r in enumerate(rows):
                arr[i].w, arr[i].wpk, arr[i].first_block, arr[i].cout, arr[i].cin, arr[i].taps, arr[i].kind = r
            self.tables.append((torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device), len(rows), blocks))
        self.keys = keys
        self.weights = [c.weight for c in convs]
        self.sig = tuple(w.data_ptr() for w in self.weights)
        self.weight_ptrs = frozenset(self.sig)
        self.misses = set()                    # (weight address, layout) a layer packed by itself while this plan was active
        self.fresh = {}

    def valid_for(self, convs):
        """Same weight tensors at the same addresses, and the packed buffers in the table are still the cache's."""
        if len(convs) != len(self.sig) or any(c.weight.data_ptr() != p for c, p in zip(convs, self.sig)):
            return False
        return all(_Packed._cache.get(k) is b for k, b in zip(self.keys, self.bufs))

    def run(self, want_first_event=False, want_events=False):
        """Enqueue the packing launches on the current stream. want_first_event: return a torch.cuda.Event recorded behind
        the first launch (the `split_at` part), else None. want_events: return the list of events, one behind every launch."""
        ev, evs = None, []
        with _lib.on_device(self.device):
            for i, (table, n_rows, blocks) in enumerate(self.tables):
                rc = _lib.fn("ossid_conv_pack_weights_table")(table.data_ptr(), n_rows, blocks, _lib.stream())
                _lib.check(rc, "ossid_conv_pack_weights_table")
                if want_events:
                    evs.append(torch.cuda.Event())
                    evs[-1].record(torch.cuda.current_stream(self.device))
                elif i == 0 and want_first_event and len(self.tables) > 1:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(self.device))
        global _ACTIVE_PLAN
        import weakref
        vers = {w.data_ptr(): w._version for w in self.weights}
        self.fresh = {k: vers[k[0]] for k in self.keys}
        _ACTIVE_PLAN = weakref.ref(self)
        return evs if want_events else ev


def end_step():
    """Forget the active plan (nothing is fresh any more)."""
    global _ACTIVE_PLAN
    _ACTIVE_PLAN = None


def conv_raw(x, wpk, B, H, W, cin, cout, taps, out, bias=None, pre=None, pre_relu=False, act=0, in_cs=0, out_cs=0,
             out_coff=0, src_hw=(0, 0), epi=None, wino=False, post=None):
    """ossid_conv_nhwc_fwd / ossid_conv3x3_wino_fwd on raw channels-last buffers. epi: {"timing_buf": tensor} for the
    -DOSSID_TIMING diagnostic builds only (tools/conv_timeline.py)."""
    d = _lib.ConvDesc()
    d.x, d.wpk, d.bias, d.out = x.data_ptr(), wpk.data_ptr(), dptr(bias), out.data_ptr()
    if pre is not None:
        d.pre_scale, d.pre_shift = pre[0].data_ptr(), pre[1].data_ptr()
    d.in_batch_stride, d.pre_batch_stride = -1, 0
    d.batch, d.height, d.width, d.cin, d.cout, d.taps = B, H, W, cin, cout, taps
    d.act, d.pre_relu = int(act), 1 if pre_relu else 0
    d.exact = int(getattr(wpk, "_ossid_exact", 0))                   # the arithmetic the weights were packed for (_pack kinds)
    d.src_height, d.src_width = int(src_hw[0]), int(src_hw[1])
    d.in_channel_stride, d.out_channel_stride, d.out_channel_offset = int(in_cs), int(out_cs), int(out_coff)
    if epi is not None and epi.get("timing_buf") is not None:
        d.scratch, d.scratch_bytes = epi["timing_buf"].data_ptr(), 1 << 30
    if post is not None:
        d.post_scale, d.post_shift = post[0].data_ptr(), post[1].data_ptr()
    name = "ossid_conv3x3_wino_fwd" if wino else "ossid_conv_nhwc_fwd"       # wino: wpk is the Winograd layout
    with _lib.on_device(out.device):
        _lib.check(_lib.fn(name)(_byref(d), _lib.stream()), name)
    return out


def colsum_finalize(partials, C, sums, sums_row_stride=0):
    part, P = partials
    with _lib.on_device(part.device):
        _lib.check(_lib.fn("ossid_colsum_finalize")(part.data_ptr(), int(P), int(C), sums.data_ptr(), int(sums_row_stride),
                                                    _lib.stream()), "ossid_colsum_finalize")


def _wgrad_desc(d, x, dy, dw, B, H, W, cin, cout, taps, pre=None, pre_relu=False, in_cs=0, dy_cs=0, src_hw=(0, 0),
                accumulate=False, dy_add=None):
    """Fills the ossid_wgrad_desc `d` (the workspace fields are the caller's)."""
    d.x, d.dy, d.dw = dptr(x), dptr(dy), dptr(dw)
    d.pre_scale, d.pre_shift = map(dptr, pre or (None, None))
    d.batch, d.height, d.width, d.cin, d.cout, d.taps = B, H, W, cin, cout, taps
    d.pre_relu, d.accumulate = 1 if pre_relu else 0, 1 if accumulate else 0
    d.in_channel_stride, d.dy_channel_stride = int(in_cs), int(dy_cs)
    d.src_height, d.src_width = int(src_hw[0]), int(src_hw[1])
    # dy = dy + scale * add + shift while it is staged (ossid_wgrad_desc.dy_add)
    d.dy_add, d.dy_add_scale, d.dy_add_shift = map(dptr, dy_add or (None, None, None))


def wgrad_raw(x, dy, B, H, W, cin, cout, taps, dw, pre=None, pre_relu=False, in_cs=0, dy_cs=0, src_hw=(0, 0),
              accumulate=False):
    d = _lib.WgradDesc()
    dev = dw.device
    nbytes = _lib.fn("ossid_conv_wgrad_workspace_bytes")(B, H, W, cin, cout, taps)
    _wgrad_desc(d, x, dy, dw, B, H, W, cin, cout, taps, pre, pre_relu, in_cs, dy_cs, src_hw, accumulate)
    d.workspace, d.workspace_bytes = dptr(_scratch("wgrad", nbytes, dev)), nbytes
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_conv_wgrad")(_byref(d), _lib.stream()), "ossid_conv_wgrad")
    return dw


def wgrad_group(items):
    """Several independent weight gradients in one launch per tiling variant (ossid_conv_wgrad_group). items: dicts with
    the keyword arguments of wgrad_raw (x, dy, B, H, W, cin, cout, taps, dw, pre, pre_relu, in_cs, dy_cs) and dy_add."""
    n = len(items)
    arr = (_lib.WgradDesc * n)()
    for d, it in zip(arr, items):
        _wgrad_desc(d, it["x"], it["dy"], it["dw"], it["B"], it["H"], it["W"], it["cin"], it["cout"], it["taps"], it.get("pre"),
                    it.get("pre_relu"), it.get("in_cs", 0), it.get("dy_cs", 0), dy_add=it.get("dy_add"))
    dev = items[0]["dw"].device
    nbytes = _lib.fn("ossid_conv_wgrad_group_workspace_bytes")(arr, n)
    if nbytes == 0:
        raise RuntimeError("ossid_conv_wgrad_group_workspace_bytes rejected the group")
    ws = _scratch("wgrad_group", nbytes, dev)
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_conv_wgrad_group")(arr, n, dptr(ws), nbytes, _lib.stream()), "ossid_conv_wgrad_group")


def bn_fold_fwd(sums, C, n, gamma, beta, eps, momentum, running_mean, running_var, sums_row_stride=0, pivot=None):
    """sums: a [2 or 3, C] tensor (third row = pivot) or a pointer into a wider table (sums_row_stride; pivot given
    separately), or the (scratch, P, pivot) triple of a deferred batch_stats. Returns [4, C] = scale, shift, mean, rstd."""
    part, P = None, 0
    if isinstance(sums, tuple):
        part, P = sums[0], sums[1]
        pivot = sums[2] if len(sums) > 2 else pivot
        dev = part.device
    else:
        dev = sums.device
        if pivot is None and sums.dim() == 2 and sums.shape[0] == 3:
            pivot = sums[2]
    out = new_buf((4, C), dev)                                          # scale, shift, mean, rstd
    with _lib.on_device(dev):
        rc = _lib.fn("ossid_bn_fold_fwd")(None if part is not None else sums.data_ptr(), int(sums_row_stride), dptr(part), int(P),
                                          dptr(pivot), C, float(n), dptr(gamma), dptr(beta), float(eps),
                                          float(momentum), dptr(running_mean), dptr(running_var), out[0].data_ptr(),
                                          out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_bn_fold_fwd")
    return out


def bn_fold_bwd(dscale, dshift, gamma, mean, rstd, C, n, dgamma, dbeta, coef_x, coef_1, accumulate=False, partials=None,
                zero_row=None):
    """partials = (scratch, P) of a deferred chan_op (row 0 = d shift, row 1 = d scale) instead of dscale / dshift.
    zero_row: C floats the same launch clears."""
    part, P = partials if partials is not None else (None, 0)
    with _lib.on_device(coef_x.device):
        rc = _lib.fn("ossid_bn_fold_bwd")(dptr(dscale), dptr(dshift), dptr(part), int(P), dptr(gamma), mean.data_ptr(), rstd.data_ptr(),
                                          C, float(n), dptr(dgamma), dptr(dbeta), coef_x.data_ptr(), coef_1.data_ptr(),
                                          1 if accumulate else 0, dptr(zero_row), _lib.stream())
    _lib.check(rc, "ossid_bn_fold_bwd")


def _mom(bn):
    return 0.1 if bn.momentum is None else bn.momentum


_UP_TABLES = {}


def _upsample_tables(Hs, Ws, H, W, device):
    """row_start / col_start of ossid_upsample_nearest_bwd_nhwc, from the forward's index formula
    (min(floor(dst * (float)in / (float)out), in - 1) in float32, csrc/conv.hip)."""
    key = (Hs, Ws, H, W, str(device))
    if key not in _UP_TABLES:
        def table(n_src, n_dst):
            scale = torch.tensor(n_src, dtype=torch.float32) / torch.tensor(n_dst, dtype=torch.float32)
            src = torch.clamp(torch.floor(torch.arange(n_dst, dtype=torch.float32) * scale).to(torch.int64), max=n_src - 1)
            start = torch.searchsorted(src, torch.arange(n_src + 1, dtype=torch.int64))
            return start.to(torch.int32).to(device)
        _UP_TABLES[key] = (table(Hs, H), table(Ws, W))
    return _UP_TABLES[key]


def upsample_bwd(dup, B, Hs, Ws, H, W, C):
    rs, cs = _upsample_tables(Hs, Ws, H, W, dup.device)
    out = empty_nhwc(B, C, Hs, Ws, dup.device)
    with _lib.on_device(dup.device):
        rc = _lib.fn("ossid_upsample_nearest_bwd_nhwc")(dup.data_ptr(), B, Hs, Ws, H, W, C, rs.data_ptr(), cs.data_ptr(),
                                                        out.data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_upsample_nearest_bwd_nhwc")
    return out


# ---- autograd Functions -----------------------------------------------------------------------------------------------
_ZEROS = {}


def _zeros(C, device):
    """A read-only all-zero [C] vector per (size, device): a per-channel coefficient that is zero (saves a fill launch per use)."""
    key = (int(C), str(device))
    z = _ZEROS.get(key)
    if z is None:
        z = torch.zeros(int(C), dtype=torch.float32, device=device)
        if not torch.cuda.is_current_stream_capturing():       # (memory allocated under a capture belongs to that graph's pool)
            _ZEROS[key] = z
    return z


class ColStats(torch.autograd.Function):
    """x [B,C,H,W] channels-last -> stats [3,C] = (sum (x - p), sum (x - p)^2, p) over B*H*W with p = x's first row (the
    pivot: a channel whose spread is small against its mean loses nothing to E[x^2] - E[x]^2). The gradient arriving on
    `stats` is, by the private convention shared with BNFold, g[0] = d/d(mean) / n-form constant term, g[1] = the
    coefficient of x: dx = g[0][c] + g[1][c] * x (g[2] is ignored: mean and variance do not depend on the pivot)."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        B, C, H, W = x.shape
        ctx.save_for_backward(x)
        return batch_stats(flat(x), B * H * W, C)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, C, H, W = x.shape
        g = g.contiguous()
        dx = torch.empty_like(x)
        chan_op(x, B * H * W, C, x=x, out=dx, alpha=_zeros(C, x.device), beta=g[1], kappa=g[0])
        return dx


class BNFold(torch.autograd.Function):
    """Training-mode BatchNorm2d as a per-channel (scale, shift): forward(sums, gamma, beta) with the module's running
    buffers updated in place (momentum, unbiased variance) exactly as nn.BatchNorm2d.train() does. Returns
    (scale, shift), each [C] -- two outputs, so that their gradients arrive as two tensors: as rows of ONE [2, C] output they
    came back through two select-backward nodes (a fill and a copy each) and an add, five launches per BatchNorm on the
    backward pass's critical chain, and the [3, C] gradient of the sums was stacked by two more."""

    @staticmethod
    def forward(ctx, sums, gamma, beta, n, bn):
        C = int(sums.shape[1])
        out = bn_fold_fwd(sums, C, n, gamma, beta, bn.eps, _mom(bn),
                          bn.running_mean if bn.track_running_stats else None,
                          bn.running_var if bn.track_running_stats else None)
        ctx.save_for_backward(gamma, out)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_scale, g_shift):
        gamma, out = ctx.saved_tensors
        C = int(out.shape[1])
        dev = out.device
        g_scale = _zeros(C, dev) if g_scale is None else g_scale.contiguous()
        g_shift = _zeros(C, dev) if g_shift is None else g_shift.contiguous()
        # rows 0..2 = the gradient of the sums in ColStats' convention [constant, x coefficient, - (cleared by the launch)],
        # rows 3, 4 = dgamma, dbeta
        res = torch.empty((5, C), dtype=torch.float32, device=dev)
        bn_fold_bwd(g_scale, g_shift, gamma, out[2], out[3], C, ctx.n, res[3], res[4], res[1], res[0], zero_row=res[2])
        return res[:3], res[3], res[4], None, None


def bn_fold(sums, n, bn):
    """(scale, shift) of a training-mode nn.BatchNorm2d given the column sums of its input."""
    return BNFold.apply(sums, bn.weight, bn.bias, n, bn)


# Weight gradients on a second HIP stream. A convolution's weight gradient feeds nothing but the optimizer, while its data
# gradient is on the critical path of backward -- a chain of small launches that occupy a fraction of the chip each. With
# WGRAD_SIDE the weight-gradient launches go to a side stream that waits for the main stream at the point of issue; the main
# stream joins it when the backward pass ends (an autograd engine callback, so a bare loss.backward() is as safe as
# finetune_step) and wherever gradients are read earlier (GradSync's per-bucket hooks). The caching allocator must keep what
# such a launch reads or writes until it has run (record_stream), and nobody lists that by hand: a launcher that may be issued
# there takes EVERY device address through dptr(), which notes the tensor while _wgrad_async is issuing; that records them.
WGRAD_SIDE = True
_wg_streams, _wg_dirty = {}, set()
_SIDE_OPERANDS = None      # what dptr() noted for the _wgrad_async under way (set around a region like _lib._REC: one process per GPU)


def dptr(t):
    """Device address of a tensor / None, for the C ABI."""
    if t is None:
        return None
    if _SIDE_OPERANDS is not None:
        _SIDE_OPERANDS.append(t)
    return t.data_ptr()


def _side_operands_of(fn):
    """Run fn(); the distinct tensor objects it passed to dptr() -- views as they came: record_stream acts on the storage's block."""
    global _SIDE_OPERANDS
    prev, _SIDE_OPERANDS = _SIDE_OPERANDS, []
    try:
        fn()
        return list({id(t): t for t in _SIDE_OPERANDS}.values())
    finally:
        _SIDE_OPERANDS = prev


from ..streams import N_STREAM_CANDIDATES, _side_pools, side_streams  # noqa: E402,F401  (the probe lives in ossid_code_amd/streams.py)


def join_wgrad_stream():
    """Main stream(s) wait for the weight gradients in flight on the side stream(s)."""
    for idx in list(_wg_dirty):
        torch.cuda.current_stream(idx).wait_stream(_wg_streams[idx])
    _wg_dirty.clear()


def _wgrad_side_ok(device, weights=()):
    """May weight-gradient launches for `weights` go to the side stream right now? Returning a tensor the side stream is
    still writing is safe ONLY while autograd's AccumulateGrad takes it over without reading it, i.e. while the parameter's
    .grad is None (finetune_step's protocol: FlatParams.detach_grads() before backward). A parameter that already holds a
    gradient (optimizer.zero_grad() that keeps the tensors, gradient accumulation over two backward passes) gets
    `p.grad += dw` on the caller's stream straight after the node returns: for those the launches stay in line. Neither
    under a graph capture (a captured graph does not run a side branch to any profit: measured 48.4 vs 47.3 ms)."""
    if not WGRAD_SIDE or device.type != "cuda" or torch.cuda.is_current_stream_capturing():
        return False
    return all(w is None or _grad_taken_unread(w) for w in weights)


def _grad_taken_unread(w):
    """Will autograd hand the gradient returned for `w` to AccumulateGrad, which takes it over without reading it? Only for
    a LEAF that holds no gradient yet. A non-leaf `w` (a relaid / padded / concatenated view of a parameter) always has
    .grad None, but the tensor returned for it is READ by the next backward nodes (reshape / pad / permute backward) on the
    caller's stream straight away: its gradient must be complete on that stream when backward() returns."""
    return w.is_leaf and w.grad is None


def _wgrad_stream(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _wg_streams:
        _wg_streams[idx] = side_streams(device)["wgrad"]
    return idx, _wg_streams[idx]


def _wgrad_in_flight(idx):
    # one callback per call, not "one while the set is empty": a backward pass that died in an exception never runs its
    # callbacks, and a set left non-empty would then suppress the join of every later pass (the join itself is a no-op
    # when nothing is in flight)
    torch.autograd.Variable._execution_engine.queue_callback(join_wgrad_stream)
    _wg_dirty.add(idx)


def _wgrad_async(fn, device, weights=(), side=None):
    """Run fn() -- weight-gradient launches writing the `dw` tensors a backward() is about to return -- on the side stream
    (side=None: decide here, see _wgrad_side_ok) and record_stream() its operands. Inside a recorded launch sequence the
    launches are stored under stream slot 1 behind a wait entry; the replay (_run_seq) records none: Seq.keep holds them."""
    if side is None:
        side = _wgrad_side_ok(device, weights)
    if not side:
        return fn()
    idx, st = _wgrad_stream(device)
    st.wait_stream(torch.cuda.current_stream(idx))
    rec = _lib.recording()
    if rec is not None:
        rec.wait(1, 0)
        rec.cur_slot, rec.seq.uses_side = 1, True
    try:
        with torch.cuda.stream(st):
            operands = _side_operands_of(fn)
    finally:
        if rec is not None:
            rec.cur_slot = 0
    for t in operands:
        t.record_stream(st)
    _wgrad_in_flight(idx)


USE_WINO = True
# The Winograd launches of the training step run without the tail split (the last, partial round of workgroups cut along the
# reduction + a finishing launch: fills an otherwise idle chip): three or four streams keep the chip busy there, and the split's
# partial sums and finishing launches (27 per step, 0.8 ms of kernel time, most of them on the two detection trunks' streams) are
# then only work: step 23.55 -> 23.40 ms without it (same box, two runs each). The test-time head keeps it (one stream:
# ops.FusedConv).
WINO_MIN_WGS = 128


def wino_fits(B, H, W, cin, cout, taps, plain=True):
    """Should this 3x3 convolution (cin -> cout on [B][H][W], no fused up-sampling) run on csrc/wino.hip? Needs the
    reduction channels in 16s, at least a pair of channel tiles and enough workgroups (32 tiles of 2x2 outputs x 64
    channels each) to occupy the chip; measured per layer in profiles/r02_train_layers_wino.txt."""
    if not (USE_WINO and plain and taps == 9 and cin % 16 == 0 and cout >= 64):
        return False
    return ((B * ((H + 1) // 2) * ((W + 1) // 2) + 31) // 32) * ((cout + 63) // 64) >= WINO_MIN_WGS


class _Flag:
    def __init__(self):
        self.v = False

    def get(self):
        return self.v


_EXACT_FWD = _Flag()


class exact_forward:
    """`with exact_forward():` -- FusedConv forwards inside run the exact-f32 launch (their output feeds a hard decision)."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.old, _EXACT_FWD.v = _EXACT_FWD.v, self.on or _EXACT_FWD.v

    def __exit__(self, *a):
        _EXACT_FWD.v = self.old
        return False


class FusedConv(torch.autograd.Function):
    """u = ELU?( conv( relu?( x * pre_scale + pre_shift ) [nearest-up-sampled to `size`], w ) + bias ), optionally with
    the column sums of u as a second output (for the BatchNorm that follows). 3x3 / pad 1 / stride 1 or 1x1.
    Backward: one generic pass for ELU' + the statistics' gradient + the bias gradient, the weight gradient on the
    prologue'd input, the data gradient as the forward kernel on the rotated weights, an up-sampling window sum, one
    generic pass for the prologue's mask / scale and the (d scale, d shift) sums."""

    @staticmethod
    def forward(ctx, x, w, bias, pre_scale, pre_shift, pre_relu, act_elu, size, want_stats):
        x = nhwc(x)
        B, Cin, Hs, Ws = x.shape
        Cout, taps = int(w.shape[0]), int(w.shape[2] * w.shape[3])
        H, W = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))
        pre = None if pre_scale is None else (pre_scale.contiguous(), pre_shift.contiguous())
        u = empty_nhwc(B, Cout, H, W, x.device)
        act = int(act_elu)                       # 0 none, 1 ELU, 2 ReLU (True = ELU: the head's `F.elu(conv(x))`)
        wino = wino_fits(B, H, W, Cin, Cout, taps, plain=(H, W) == (Hs, Ws))
        deciding = act == 2 or _EXACT_FWD.get()
        conv_raw(x, _pack(w, "wino_fwd" if wino else (FWD_DECIDING if deciding else "fwd")), B, H, W, Cin, Cout, taps, u,
                 bias=None if bias is None else bias.detach(), pre=pre, pre_relu=pre_relu, act=act,
                 src_hw=(Hs, Ws) if size is not None else (0, 0), wino=wino)
        sums = batch_stats(flat(u), B * H * W, Cout) if want_stats else None
        ctx.save_for_backward(x, w, u if (act or want_stats) else None, None if pre is None else pre[0],
                              None if pre is None else pre[1])
        ctx.cfg = (pre_relu, act, (H, W), want_stats, bias is not None)
        if want_stats:
            return u, sums
        return u

    @staticmethod
    def backward(ctx, du, dsums=None):
        x, w, u, ps, pt = ctx.saved_tensors
        pre_relu, act_elu, (H, W), want_stats, has_bias = ctx.cfg
        B, Cin, Hs, Ws = x.shape
        Cout, taps = int(w.shape[0]), int(w.shape[2] * w.shape[3])
        dev = x.device
        N = B * H * W
        du = nhwc(du)
        need = ctx.needs_input_grad
        # 1. through ELU and the statistics: dv = (du + dsums[1] * u + dsums[0]) * ELU'(u); column sums = bias gradient
        db = None
        use_stats = want_stats and dsums is not None
        if act_elu or use_stats or (has_bias and need[2]):
            dv = torch.empty_like(du) if (act_elu or use_stats) else None
            sums = chan_op(du, N, Cout, x=u if (act_elu or use_stats) else None, out=dv,
                           beta=dsums[1].contiguous() if use_stats else None,
                           kappa=dsums[0].contiguous() if use_stats else None, mask_mode=(0, 2, 3)[act_elu],
                           sum_mode=2 if (has_bias and need[2]) else 0)
            if dv is None:
                dv = du
            if sums is not None:
                db = sums[0]                     # (a row of a fresh [2, C] tensor: AccumulateGrad takes it over as it is)
        else:
            dv = du
        pre = None if ps is None else (ps, pt)
        # 2. weight gradient on the (prologue'd, up-sampled) input
        dw = None
        if need[1]:
            dwb = grad_home(w, _grad_taken_unread(w))     # straight into the flat gradient buffer when autograd will take it over
            _wgrad_async(lambda: wgrad_raw(x, dv, B, H, W, Cin, Cout, taps, dwb, pre=pre, pre_relu=pre_relu,
                                           src_hw=(Hs, Ws) if (H, W) != (Hs, Ws) else (0, 0)), dev, weights=(w,))
            dw = _alias(dwb)
        # 3. data gradient
        dx = dps = dpt = None
        if need[0] or (pre is not None and (need[3] or need[4])):
            dxu = empty_nhwc(B, Cin, H, W, dev)
            wino = wino_fits(B, H, W, Cout, Cin, taps)
            conv_raw(dv, _pack(w, "wino_dgrad" if wino else "dgrad"), B, H, W, Cout, Cin, taps, dxu, wino=wino)
            if (H, W) != (Hs, Ws):
                dxu = upsample_bwd(dxu, B, Hs, Ws, H, W, Cin)
            if pre is not None:
                dx = torch.empty_like(x)
                sums = chan_op(dxu, B * Hs * Ws, Cin, x=x, out=dx, alpha=ps, mask_mode=1 if pre_relu else 0, mask_scale=ps,
                               mask_shift=pt, sum_mode=1)
                dpt, dps = sums[0], sums[1]
            else:
                dx = dxu
        return dx, dw, db, dps, dpt, None, None, None, None


def fused_conv(x, conv, pre=None, pre_relu=False, act_elu=False, size=None, want_stats=False, act=None):
    """Apply an nn.Conv2d (3x3 / pad 1 or 1x1, stride 1) through FusedConv. pre = (scale, shift) or None; act: 0 none,
    1 ELU, 2 ReLU (act_elu=True is act=1)."""
    ps, pt = (None, None) if pre is None else pre
    a = int(act) if act is not None else (1 if act_elu else 0)
    return FusedConv.apply(x, conv.weight, conv.bias, ps, pt, bool(pre_relu), a, size, bool(want_stats))


class AvgPool2(torch.autograd.Function):
    """nn.AvgPool2d(2, stride) on a channels-last tensor."""

    @staticmethod
    def forward(ctx, x, stride):
        x = nhwc(x)
        B, C, H, W = x.shape
        Ho, Wo = (H - 2) // stride + 1, (W - 2) // stride + 1
        out = empty_nhwc(B, C, Ho, Wo, x.device)
        with _lib.on_device(x.device):
            _lib.check(_lib.fn("ossid_avgpool2_nhwc")(x.data_ptr(), B, H, W, C, stride, out.data_ptr(), 0, _lib.stream()),
                       "ossid_avgpool2_nhwc")
        ctx.cfg = (B, C, H, W, stride)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, H, W, stride = ctx.cfg
        g = nhwc(g)
        dx = empty_nhwc(B, C, H, W, g.device)
        with _lib.on_device(g.device):
            _lib.check(_lib.fn("ossid_avgpool2_nhwc")(g.data_ptr(), B, H, W, C, stride, dx.data_ptr(), 1, _lib.stream()),
                       "ossid_avgpool2_nhwc")
        return dx, None


# Recorded launch sequences (_lib.Seq) for the fixed-shape pieces of the step: on (default) the dense blocks -- and the template
# encoders and the stem, below -- build their launch sequence once per (shape, parameter addresses) into persistent buffers and
# replay it afterwards; off: every step runs the Python bodies with fresh buffers (what the sequences are recorded from).
SEQ_REPLAY = True


class _Plan:
    """Persistent buffers + the recorded forward / backward sequences of one module at one input shape."""
    __slots__ = ("fwd", "bwd", "t", "gen", "side")

    def __init__(self):
        self.fwd = self.bwd = None
        self.t, self.gen, self.side = {}, 0, False


def _plan_for(module, key):
    plans = module.__dict__.setdefault("_train_plans", {})
    plan = plans.get(key)
    if plan is None:
        if len(plans) >= 2:                # shapes change rarely (a last, smaller batch): keep two sets of buffers at most
            plans.clear()
        plan = plans[key] = _Plan()
    return plan


def _run_seq(seq, dev):
    """Replay on the current stream (slot 0) and, if the sequence has side launches, the weight-gradient stream (slot 1),
    with the bookkeeping _wgrad_async does for an eager launch (the end-of-backward join)."""
    main = torch.cuda.current_stream(dev)
    if seq.uses_side:
        idx, side = _wgrad_stream(dev)
        seq.run((main, side))
        _wgrad_in_flight(idx)
    else:
        seq.run((main,))


# The dense layers' 1x1 forward with norm2's batch statistics in its epilogue (csrc/dense_bwd.hip) instead of the convolution +
# a pass that reads its output again for two sums (the split-bf16 build only).
def dense_fwd1_stats(buf, wpk_x6, y1, N, c, Ct, ps, pt):
    """y1 = conv1x1(relu(ps * buf[:, :c] + pt)); returns (rows [P][3][128], counts [P], P) for bn_fold_fwd_rows -- valid until
    the next call on this stream."""
    dev = buf.device
    P = _lib.fn("ossid_dense_fwd1_stats_partials")(int(N))
    part = _scratch("fwd1_stats", (P * 3 * 128 + P + 64) * 4, dev)
    counts = part[P * 3 * 128 * 4:]
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_dense_fwd1_stats")(buf.data_ptr(), int(Ct), int(c), ps.data_ptr(), pt.data_ptr(), wpk_x6.data_ptr(),
                                                     int(N), y1.data_ptr(), part.data_ptr(), counts.data_ptr(), _lib.stream()),
                   "ossid_dense_fwd1_stats")
    return part, counts, P


def bn_fold_fwd_rows(rows, C, n, gamma, beta, eps, momentum, running_mean, running_var):
    """bn_fold_fwd for partial rows that carry their own pivots (dense_fwd1_stats). Returns [4, C] = scale, shift, mean, rstd."""
    part, counts, P = rows
    out = new_buf((4, C), part.device)
    with _lib.on_device(part.device):
        rc = _lib.fn("ossid_bn_fold_fwd_rows")(part.data_ptr(), counts.data_ptr(), int(P), C, float(n), dptr(gamma), dptr(beta), float(eps),
                                               float(momentum), dptr(running_mean), dptr(running_var), out[0].data_ptr(),
                                               out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _lib.stream())
    _lib.check(rc, "ossid_bn_fold_fwd_rows")
    return out


def _dense_forward(buf, table, block, params, C0):
    """The forward launches of a dense block whose input already sits in buf[:, :C0] (raw ops only: recordable).
    Returns the per-layer (f1, y1, f2) the backward pass needs."""
    B, Ct, H, W = buf.shape
    dev = buf.device
    N = B * H * W
    growth = block.growth
    batch_stats(flat(buf), N, C0, cs=Ct, sums=table, sums_row_stride=Ct)
    fused_fwd = (FWD_DECIDING == "fwd_x6" and growth == 32 and bool(_lib.fn("ossid_conv_split_bf16")()) and
                 all(int(params[6 * li + 2].shape[0]) == 128 for li in range(len(block))))
    saved = []
    c = C0
    tail = None                     # the previous layer's slab statistics, still partial rows (finalized by this layer's fold)
    L = len(block)
    for li, layer in enumerate(block.values()):
        g1, b1, w1, g2, b2, w2 = params[6 * li:6 * li + 6]
        if tail is not None:
            part, P, piv = tail
            f1 = new_buf((4, c), dev)
            with _lib.on_device(dev):
                rc = _lib.fn("ossid_bn_fold_fwd_tail")(table.data_ptr(), Ct, c - growth, part.data_ptr(), int(P), piv.data_ptr(), c,
                                                       float(N), g1.data_ptr(), b1.data_ptr(), float(layer.norm1.eps),
                                                       float(_mom(layer.norm1)), layer.norm1.running_mean.data_ptr(),
                                                       layer.norm1.running_var.data_ptr(), f1[0].data_ptr(), f1[1].data_ptr(),
                                                       f1[2].data_ptr(), f1[3].data_ptr(), _lib.stream())
            _lib.check(rc, "ossid_bn_fold_fwd_tail")
        else:
            f1 = bn_fold_fwd(table, c, N, g1, b1, layer.norm1.eps, _mom(layer.norm1), layer.norm1.running_mean,
                             layer.norm1.running_var, sums_row_stride=Ct, pivot=table[2])
        mid = int(w1.shape[0])
        y1 = new_buf((B, mid, H, W), dev, channels_last=True)
        if fused_fwd:
            rows = dense_fwd1_stats(buf, _pack(w1, "fwd_x6"), y1, N, c, Ct, f1[0], f1[1])
            f2 = bn_fold_fwd_rows(rows, mid, N, g2, b2, layer.norm2.eps, _mom(layer.norm2), layer.norm2.running_mean,
                                  layer.norm2.running_var)
        else:
            conv_raw(buf, _pack(w1, FWD_DECIDING), B, H, W, c, mid, 1, y1, pre=(f1[0], f1[1]), pre_relu=True, in_cs=Ct)
            s2 = batch_stats(flat(y1), N, mid, defer=True)
            f2 = bn_fold_fwd(s2, mid, N, g2, b2, layer.norm2.eps, _mom(layer.norm2), layer.norm2.running_mean,
                             layer.norm2.running_var)
        conv_raw(y1, _pack(w2, FWD_DECIDING), B, H, W, mid, growth, 9, buf, pre=(f2[0], f2[1]), pre_relu=True, out_cs=Ct, out_coff=c)
        if li + 1 < L:
            tail = batch_stats(flat(buf, c), N, growth, cs=Ct, defer=True)       # finished by the next layer's fold
        else:
            batch_stats(flat(buf, c), N, growth, cs=Ct, sums=table.view(-1)[c:], sums_row_stride=Ct)
        saved.append((f1, y1, f2))
        c += growth
    return saved


# The dense layers' 1x1 data gradient with the masked, scaled accumulation onto the block's gradient buffer and norm1's column
# sums in ONE launch (csrc/dense_bwd.hip) instead of the convolution + a generic pass over a [N][c] tensor in between.
# ... and the layers' 3x3 data gradient with norm2 / ReLU's backward in its epilogue. (The dense layers' second convolution then
# needs the DIRECT data-gradient layout, not the Winograd one: Network._train_pack_plan asks this function.) Both take the
# split-bf16 build only: the all-exact build runs the plain convolutions and the generic passes.
def dense_bwd3_fused():
    return bool(_lib.fn("ossid_conv_split_bf16")())


def dense_dgrad1_acc(dz, wpk_dgrad, buf, G, N, c, Ct, alpha, ms, mt, add=None):
    """G[:, :c] += alpha * relu'(ms * buf + mt) * (dz @ W1); returns the (partials, P) pair of norm1's column sums for
    bn_fold_bwd -- valid until the next call on this stream. add = (y, scale, shift): dz is dz + scale * y + shift."""
    dev = dz.device
    P = _lib.fn("ossid_dense_dgrad1_acc_partials")(int(N))
    part = _scratch("dgrad1_acc", P * 2 * c * 4, dev)
    with _lib.on_device(dev):
        _lib.check(_lib.fn("ossid_dense_dgrad1_acc")(dz.data_ptr(), wpk_dgrad.data_ptr(), buf.data_ptr(), G.data_ptr(), int(N), int(c),
                                                     int(Ct), alpha.data_ptr(), ms.data_ptr(), mt.data_ptr(), part.data_ptr(),
                                                     None if add is None else add[0].data_ptr(),
                                                     None if add is None else add[1].data_ptr(),
                                                     None if add is None else add[2].data_ptr(), _lib.stream()),
                   "ossid_dense_dgrad1_acc")
    return part, P


def _dense_backward(G, buf, saved, block, params, C0, side, direct=False):
    """The backward launches of a dense block whose output gradient already sits in G (ours to accumulate into); raw ops
    only. Returns (dx [B,C0,H,W] compact, parameter gradients in `params` order). side: the block's grouped weight-gradient
    launch goes to the weight-gradient stream (decided by the caller: _wgrad_side_ok)."""
    B, Ct, H, W = buf.shape
    dev = buf.device
    N = B * H * W
    L, growth = block.nlayers, block.growth
    coef = new_buf((2, Ct), dev, zero=True)                       # [coef_x, coef_1] of the statistics' gradient
    grads = [None] * len(params)
    mid = int(params[2].shape[0])
    dz_all = new_buf((L, B, H, W, mid), dev)                      # per layer: the 1x1 wgrad runs at the end
    deferred = []                                                 # the block's 2 L weight gradients: ONE grouped launch below
    da = None
    fused_bwd = (mid == 128 and Ct <= 1024 and N * Ct < (1 << 32) and
                 bool(_lib.fn("ossid_conv_split_bf16")()))
    fused_bwd3 = dense_bwd3_fused() and mid == 128 and growth == 32 and N * mid < (1 << 31)
    c = C0 + L * growth
    for li in range(L - 1, -1, -1):
        c -= growth
        g1, b1, w1, g2, b2, w2 = params[6 * li:6 * li + 6]
        f1, y1, f2 = saved[li]
        db = dz_all[li]
        # the layer's own 32 channels: every later consumer has added its share; add the statistics term
        gs, xs = flat(G, c), flat(buf, c)
        chan_op(gs, N, growth, x=xs, out=gs, g_cs=Ct, x_cs=Ct, out_cs=Ct, beta=coef[0, c:c + growth],
                kappa=coef[1, c:c + growth])
        # 3x3: weight gradient on relu(bn2(y1)) (deferred: this slice of G is final from here on), data gradient
        # to the bottleneck (reads the strided slice: in_cs = Ct)
        dw2 = grad_home(w2, direct)
        deferred.append(dict(x=y1, dy=gs, B=B, H=H, W=W, cin=mid, cout=growth, taps=9, dw=dw2, pre=(f2[0], f2[1]),
                             pre_relu=True, dy_cs=Ct))
        if fused_bwd3:
            # ... with the ReLU mask of relu(bn2(y1)), the scale and the (d shift, d scale) sums in its epilogue (csrc/dense_bwd.hip)
            P3 = _lib.fn("ossid_dense_dgrad3_mask_partials")(B, H, W)
            part3 = _scratch("dgrad3_mask", P3 * 2 * mid * 4, dev)
            with _lib.on_device(dev):
                _lib.check(_lib.fn("ossid_dense_dgrad3_mask")(gs.data_ptr(), Ct, _pack(w2, "dgrad").data_ptr(), y1.data_ptr(),
                                                              db.data_ptr(), B, H, W, f2[0].data_ptr(), f2[0].data_ptr(),
                                                              f2[1].data_ptr(), part3.data_ptr(), _lib.stream()),
                           "ossid_dense_dgrad3_mask")
            s = (part3, P3)
        else:
            wino = wino_fits(B, H, W, growth, mid, 9)
            conv_raw(gs, _pack(w2, "wino_dgrad" if wino else "dgrad"), B, H, W, growth, mid, 9, db, in_cs=Ct, wino=wino)
            # ... then the ReLU mask of relu(bn2(y1)), the scale and the (d shift, d scale) sums
            s = chan_op(db, N, mid, x=y1, out=db, alpha=f2[0], mask_mode=1, mask_scale=f2[0], mask_shift=f2[1],
                        sum_mode=1, defer=True)
        r2 = new_buf((4, mid), dev)
        bn_fold_bwd(None, None, g2, f2[2], f2[3], mid, N, r2[0], r2[1], r2[2], r2[3], partials=s)
        # dz = scale*db*mask + coef_x*y1 + coef_1: a pass of its own, or -- with the fused 1x1 data gradient -- formed while dz is
        # staged, there and in the (deferred) 1x1 weight gradient
        add = (y1, r2[2], r2[3]) if fused_bwd else None
        if add is None:
            chan_op(db, N, mid, x=y1, out=db, beta=r2[2], kappa=r2[3])
        # 1x1: weight gradient on relu(bn1(buf[:, :c])) (deferred), data gradient to the c input channels
        dw1 = grad_home(w1, direct)
        deferred.append(dict(x=buf, dy=db, B=B, H=H, W=W, cin=c, cout=mid, taps=1, dw=dw1, pre=(f1[0], f1[1]),
                             pre_relu=True, in_cs=Ct, dy_add=add))
        # ... then one pass that masks with relu(bn1(buf)), scales, ACCUMULATES onto the gradient buffer's channel prefix
        # and sums (d shift, d scale)
        if fused_bwd:
            s = dense_dgrad1_acc(db, _pack(w1, "dgrad"), buf, G, N, c, Ct, f1[0], f1[0], f1[1], add=add)
        else:
            if da is None:
                da = new_buf((B, Ct, H, W), dev, channels_last=True)
            conv_raw(db, _pack(w1, "dgrad"), B, H, W, mid, c, 1, da)
            s = chan_op(da, N, c, x=buf, out=G, x_cs=Ct, out_cs=Ct, alpha=f1[0], mask_mode=1, mask_scale=f1[0],
                        mask_shift=f1[1], accumulate=True, sum_mode=1, defer=True)
        r1 = new_buf((2, c), dev)
        bn_fold_bwd(None, None, g1, f1[2], f1[3], c, N, r1[0], r1[1], coef[0], coef[1], accumulate=True, partials=s)
        grads[6 * li:6 * li + 6] = [r1[0], r1[1], dw1, r2[0], r2[1], dw2]
    _wgrad_async(lambda: wgrad_group(deferred), dev, side=side)
    # the block's input channels, written compactly
    dx = new_buf((B, C0, H, W), dev, channels_last=True)
    chan_op(G, N, C0, x=buf, out=dx, g_cs=Ct, x_cs=Ct, beta=coef[0, :C0], kappa=coef[1, :C0])
    return dx, grads


def _alias(t):
    """A fresh tensor object on the same memory: what a replayed plan hands to autograd (AccumulateGrad takes a gradient
    over without a copy only when nothing else refers to the tensor OBJECT; the plan keeps the buffer itself)."""
    return t.detach().view(t.shape) if t.is_contiguous() else t.detach().as_strided(t.shape, t.stride(), t.storage_offset())


class DenseBlockTrain(torch.autograd.Function):
    """A DenseNet block in training mode (models/dtoid/network.py:164-184 builds torchvision's densenet121; each layer is
    BN-ReLU-Conv1x1(128) - BN-ReLU-Conv3x3(32) on the concatenation of everything before it).

    Forward: ONE resident [B][H][W][C_total] buffer; a [3][C_total] table of column sums filled once per produced channel;
    per layer two folded BatchNorms and two convolutions with the fold applied in their input staging; the layer's 32
    channels are appended in place. Backward: ONE gradient buffer; per layer (last to first): finish the layer's own
    channel slice (statistics term), data gradient of the 3x3, ReLU/BatchNorm backward on the 128-channel bottleneck (two
    generic passes), data gradient of the 1x1, and one generic pass that masks, scales and ACCUMULATES the input gradient
    onto the channel prefix while summing (d shift, d scale); the 2 L weight gradients as one grouped launch.

    With SEQ_REPLAY the ~14 launches per layer are recorded once per (shape, parameter addresses) into persistent buffers
    and replayed (_lib.Seq): the host's share of a block drops from ~10 us per launch to the bare call. The persistent
    buffers belong to the LAST forward: a backward pass of an older forward raises."""

    @staticmethod
    def forward(ctx, x, block, *params):
        x = nhwc(x)
        B, C0, H, W = x.shape
        L, growth = block.nlayers, block.growth
        Ct = C0 + L * growth
        dev = x.device
        N = B * H * W
        plan = None
        if SEQ_REPLAY and not torch.cuda.is_current_stream_capturing():
            plan = _plan_for(block, (B, C0, H, W, str(dev), params[0].data_ptr(), params[-1].data_ptr(),
                                     block[next(iter(block))].norm1.running_mean.data_ptr(),
                                     _Packed.get(params[2].detach(), FWD_DECIDING).data_ptr()))
        if plan is None:
            buf = empty_nhwc(B, Ct, H, W, dev)
            table = torch.empty((3, Ct), dtype=torch.float32, device=dev)
        elif "buf" not in plan.t:
            buf = plan.t["buf"] = empty_nhwc(B, Ct, H, W, dev)
            table = plan.t["table"] = torch.empty((3, Ct), dtype=torch.float32, device=dev)
        else:
            buf, table = plan.t["buf"], plan.t["table"]
        chan_op(flat(x), N, C0, out=flat(buf), out_cs=Ct)                 # the block's input into the buffer's prefix
        if plan is None:
            saved = _dense_forward(buf, table, block, params, C0)
        elif plan.fwd is None:
            seq = _lib.Seq()
            with _lib.record(seq):
                plan.t["saved"] = _dense_forward(buf, table, block, params, C0)
            plan.fwd = seq
            saved = plan.t["saved"]
        else:
            plan.fwd.run((torch.cuda.current_stream(dev),))
            saved = plan.t["saved"]
        out = buf if plan is None else _alias(buf)
        # The OUTPUT must go through save_for_backward: `ctx.buf = buf` would close a cycle ctx -> buf -> grad_fn -> ctx
        # through a C++ shared_ptr that Python's collector cannot see, so a training-mode forward whose backward never runs
        # (a forward-only timing pass, a backward that raises) leaked the whole upstream graph -- and with it every
        # AccumulateGrad node, which then carried a stale stream into the next hipGraph capture.
        ctx.save_for_backward(out)
        ctx.block, ctx.saved, ctx.params, ctx.C0, ctx.plan = block, saved, params, C0, plan
        if plan is not None:
            plan.gen += 1
            ctx.gen = plan.gen
        return out

    @staticmethod
    def backward(ctx, gbuf):
        block, saved, params, C0, plan = ctx.block, ctx.saved, ctx.params, ctx.C0, ctx.plan
        (buf,) = ctx.saved_tensors
        B, Ct, H, W = buf.shape
        dev = buf.device
        weights = [params[6 * li + k] for li in range(block.nlayers) for k in (2, 5)]
        side = _wgrad_side_ok(dev, weights)
        direct = all(_grad_taken_unread(w) for w in weights)      # (the plan's `side` slot holds the pair)
        if plan is not None and ctx.gen != plan.gen:
            raise RuntimeError("DenseBlockTrain: this block ran another training forward since the one being differentiated; "
                               "its persistent buffers hold the later pass (run backward before the next forward, or set "
                               "train_ops.SEQ_REPLAY = False)")
        if plan is not None and torch.cuda.is_current_stream_capturing():
            plan = None                                                    # (forward outside, backward inside a capture)
        if plan is None:
            G = gbuf.float().clone(memory_format=torch.channels_last)      # ours to accumulate into
            dx, grads = _dense_backward(G, buf, saved, block, params, C0, side, direct)
            ctx.saved = None
            return (dx, None) + tuple(_alias(g) if g is not None else None for g in grads)
        if "G" not in plan.t:
            plan.t["G"] = empty_nhwc(B, Ct, H, W, dev)
        G = plan.t["G"]
        G.copy_(gbuf)
        if plan.bwd is None or plan.side != (side, direct):
            seq = _lib.Seq()
            with _lib.record(seq):
                plan.t["dx"], plan.t["grads"] = _dense_backward(G, buf, saved, block, params, C0, side, direct)
            plan.bwd, plan.side = seq, (side, direct)
        else:
            _run_seq(plan.bwd, dev)
        ctx.saved = None
        return (_alias(plan.t["dx"]), None) + tuple(_alias(g) for g in plan.t["grads"])


class DwXcorrAdd(torch.autograd.Function):
    """y = x + conv2d_dw_group(x, k) (network.py:178-179) on a channels-last x [B,C,H,W], k [B,C,3,3]."""

    @staticmethod
    def forward(ctx, x, k):
        x = nhwc(x)
        B, C, H, W = x.shape
        k = k.float().contiguous()
        out = torch.empty_like(x)
        with _lib.on_device(x.device):
            _lib.check(_lib.fn("ossid_dw_add_nhwc")(x.data_ptr(), k.data_ptr(), C * 9 if k.shape[0] > 1 else 0, B, H, W, C, 0,
                                                    out.data_ptr(), _lib.stream()), "ossid_dw_add_nhwc")
        ctx.save_for_backward(x, k)
        return out

    @staticmethod
    def backward(ctx, g):
        x, k = ctx.saved_tensors
        B, C, H, W = x.shape
        g = nhwc(g)
        dx = dk = None
        with _lib.on_device(x.device):
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                _lib.check(_lib.fn("ossid_dw_add_nhwc")(g.data_ptr(), k.data_ptr(), C * 9 if k.shape[0] > 1 else 0, B, H, W, C, 1,
                                                        dx.data_ptr(), _lib.stream()), "ossid_dw_add_nhwc")
            if ctx.needs_input_grad[1]:
                ws = _scratch("dwk", _lib.fn("ossid_dw_bwd_k_workspace_floats")(B, H, W, C) * 4, x.device)
                dkb = torch.empty((B, C, 3, 3), dtype=torch.float32, device=x.device)
                _lib.check(_lib.fn("ossid_dw_bwd_k_nhwc")(x.data_ptr(), g.data_ptr(), B, H, W, C, ws.data_ptr(), dkb.data_ptr(),
                                                          _lib.stream()), "ossid_dw_bwd_k_nhwc")
                dk = dkb if k.shape[0] > 1 else dkb.sum(0, keepdim=True)
        return dx, dk


class MaxPoolNHWC(torch.autograd.Function):
    """nn.MaxPool2d(k, stride, pad, ceil_mode) on a channels-last tensor; the argmax window position is kept as uint8."""

    @staticmethod
    def forward(ctx, x, k, stride, pad, ceil_mode):
        x = nhwc(x)
        B, C, H, W = x.shape

        def osz(n):
            o = -(-(n + 2 * pad - k) // stride) + 1 if ceil_mode else (n + 2 * pad - k) // stride + 1
            return o - 1 if ceil_mode and (o - 1) * stride >= n + pad else o
        Ho, Wo = osz(H), osz(W)
        out = empty_nhwc(B, C, Ho, Wo, x.device)
        idx = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device=x.device)
        with _lib.on_device(x.device):
            _lib.check(_lib.fn("ossid_maxpool_idx_nhwc")(x.data_ptr(), B, H, W, C, k, stride, pad, 1 if ceil_mode else 0,
                                                         out.data_ptr(), idx.data_ptr(), _lib.stream()), "ossid_maxpool_idx_nhwc")
        ctx.save_for_backward(idx)
        ctx.cfg = (B, C, H, W, k, stride, pad, Ho, Wo)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        B, C, H, W, k, stride, pad, Ho, Wo = ctx.cfg
        g = nhwc(g)
        dx = empty_nhwc(B, C, H, W, g.device)
        with _lib.on_device(g.device):
            _lib.check(_lib.fn("ossid_maxpool_bwd_nhwc")(g.data_ptr(), idx.data_ptr(), B, H, W, C, k, stride, pad, Ho, Wo,
                                                         dx.data_ptr(), _lib.stream()), "ossid_maxpool_bwd_nhwc")
        return dx, None, None, None, None


class AffineAct(torch.autograd.Function):
    """y = relu?(x * scale[c] + shift[c]) materialised (a training BatchNorm whose consumer is not a convolution: in front
    of a max-pool, a bilinear resize, a concatenation). One generic pass forward, one backward (with the (d shift, d scale)
    sums)."""

    @staticmethod
    def forward(ctx, x, scale, shift, relu):
        x = nhwc(x)
        B, C, H, W = x.shape
        scale, shift = scale.contiguous(), shift.contiguous()
        y = torch.empty_like(x)
        chan_op(x, B * H * W, C, x=x, out=y, alpha=scale, kappa=shift, mask_mode=1 if relu else 0, mask_scale=scale,
                mask_shift=shift)
        ctx.save_for_backward(x, scale, shift)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, g):
        x, scale, shift = ctx.saved_tensors
        B, C, H, W = x.shape
        g = nhwc(g)
        dx = torch.empty_like(x)
        s = chan_op(g, B * H * W, C, x=x, out=dx, alpha=scale, mask_mode=1 if ctx.relu else 0, mask_scale=scale,
                    mask_shift=shift, sum_mode=1)
        return dx, s[1], s[0], None


def conv3x3_c1_wgrad_raw(x, g, B, H, W, C, dwb, dbb):
    """ossid_conv3x3_c1_wgrad: dwb [1,C,3,3], dbb [1] from x [B][H][W][C] and g [B][H][W]."""
    nbytes = _lib.fn("ossid_conv3x3_c1_wgrad_workspace_bytes")()
    with _lib.on_device(x.device):
        ws = _scratch("c1_wgrad", nbytes, x.device)
        _lib.check(_lib.fn("ossid_conv3x3_c1_wgrad")(dptr(x), dptr(g), B, H, W, C, dptr(ws), nbytes, dptr(dwb), dptr(dbb),
                                                     _lib.stream()), "ossid_conv3x3_c1_wgrad")


class Conv3x3C1(torch.autograd.Function):
    """nn.Conv2d(C, 1, 3, padding=1) on a channels-last x [B,C,H,W] -> [B,1,H,W] (the decoder's seg_final, network.py:362) on the
    vector-ALU kernels of csrc/train.hip (ossid_conv3x3_c1_*): MIOpen's implicit-GEMM kernels for this one-row layer plus
    their layout transposes were ~0.7 ms of the step around the loss."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = nhwc(x)
        B, C, H, W = x.shape
        wc = w.detach().contiguous()
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            _lib.check(_lib.fn("ossid_conv3x3_c1_fwd")(x.data_ptr(), B, H, W, C, wc.data_ptr(), dptr(None if bias is None else bias.detach()),
                                                       out.data_ptr(), _lib.stream()), "ossid_conv3x3_c1_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        g = g.float().contiguous()
        dx = dw = db = None
        with _lib.on_device(dev):
            if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
                dwb = grad_home(w, _grad_taken_unread(w))
                dbb = torch.empty(1, dtype=torch.float32, device=dev)
                _wgrad_async(lambda: conv3x3_c1_wgrad_raw(x, g, B, H, W, C, dwb, dbb), dev, weights=(w,))
                # (fresh tensor objects on the same memory: AccumulateGrad takes a gradient over unread only when nothing else
                # refers to the tensor OBJECT, and clones it -- i.e. reads it -- otherwise)
                dw, db = _alias(dwb), (_alias(dbb) if ctx.has_bias else None)
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                _lib.check(_lib.fn("ossid_conv3x3_c1_dgrad")(g.data_ptr(), B, H, W, C, w.detach().contiguous().data_ptr(), dx.data_ptr(),
                                                             _lib.stream()), "ossid_conv3x3_c1_dgrad")
        return dx, dw, db


def conv3x3_c1(x, conv):
    """Apply an nn.Conv2d(C, 1, 3, padding=1) through Conv3x3C1."""
    return Conv3x3C1.apply(x, conv.weight, conv.bias)


class Conv1x1C1(torch.autograd.Function):
    """nn.Conv2d(C, 1, 1) on a channels-last x [B,C,H,W] -> [B,1,H,W] (`corr_conv_heatmap` 512 -> 1, network.py:334, :349) on the
    deterministic vector-ALU kernels ossid_conv1x1_c1_fwd / _bwd: MIOpen's implicit-GEMM kernels for this one-row layer were
    the last library convolutions of the step (forward, data and weight gradient)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = nhwc(x)
        B, C, H, W = x.shape
        wf = w.detach().reshape(-1).contiguous()
        out = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
        with _lib.on_device(x.device):
            _lib.check(_lib.fn("ossid_conv1x1_c1_fwd")(x.data_ptr(), B * H * W, C, wf.data_ptr(), dptr(None if bias is None else bias.detach()),
                                                       0, out.data_ptr(), _lib.stream()), "ossid_conv1x1_c1_fwd")
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        rows = B * H * W
        g = g.float().contiguous()
        wf = w.detach().reshape(-1).contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ws = _scratch("c1x1_bwd", _lib.fn("ossid_conv1x1_c1_bwd_workspace_floats")(rows, C) * 4, dev)
        dwb = torch.empty(C + 1, dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.fn("ossid_conv1x1_c1_bwd")(x.data_ptr(), g.data_ptr(), rows, C, wf.data_ptr(), ws.data_ptr(), dptr(dx),
                                                       dwb.data_ptr(), _lib.stream()), "ossid_conv1x1_c1_bwd")
        return dx, dwb[:C].reshape(w.shape), (dwb[C:] if ctx.has_bias else None)


def conv1x1_c1(x, conv):
    """Apply an nn.Conv2d(C, 1, 1) through Conv1x1C1."""
    return Conv1x1C1.apply(x, conv.weight, conv.bias)


def bn_act_train(x, bn, relu=False):
    """Training-mode BatchNorm (+ReLU) with a materialised output, on this repo's passes: column sums -> fold -> apply."""
    B, C, H, W = x.shape
    scale, shift = bn_fold(ColStats.apply(x), B * H * W, bn)
    return AffineAct.apply(x, scale, shift, bool(relu))


def stem_wgrad_raw(img, g, B, Cin, H, W, Cout, k, dwb):
    """ossid_stem_conv_wgrad (stride 2, padding 3): dwb [Cout,Cin,k,k] from the NCHW image and g [B][Ho][Wo][Cout]."""
    with _lib.on_device(img.device):
        ws = _scratch("stem_wgrad", _lib.fn("ossid_stem_conv_wgrad_workspace_bytes")(B, H, W), img.device)
        _lib.check(_lib.fn("ossid_stem_conv_wgrad")(dptr(img), dptr(g), B, Cin, H, W, Cout, k, 2, 3, None, None, dptr(ws),
                                                    ws.numel(), dptr(dwb), 0, _lib.stream()), "ossid_stem_conv_wgrad")


class StemConv(torch.autograd.Function):
    """DenseNet conv0 = nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False) (network.py:164-170) on the NCHW image as the
    caller holds it -> channels-last [B,64,Ho,Wo]: implicit-im2col MFMA kernel of csrc/stem.hip, exact f32. Backward: the
    weight gradient only (the image is an input), on the weight-gradient stream; written straight into the flat gradient
    buffer when autograd will take it over unread."""

    @staticmethod
    def forward(ctx, img, w, bias):
        img = img.float().contiguous()
        B, Cin, H, W = img.shape
        Cout, k = int(w.shape[0]), int(w.shape[2])
        Ho, Wo = (H + 6 - k) // 2 + 1, (W + 6 - k) // 2 + 1
        out = empty_nhwc(B, Cout, Ho, Wo, img.device)
        wd = w.detach()
        assert wd.is_contiguous()
        with _lib.on_device(img.device):
            _lib.check(_lib.fn("ossid_stem_conv_fwd")(img.data_ptr(), B, Cin, H, W, wd.data_ptr(), Cout, k, 2, 3,
                                                      dptr(None if bias is None else bias.detach()), None, None, out.data_ptr(),
                                                      _lib.stream()), "ossid_stem_conv_fwd")
        ctx.save_for_backward(img, w)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        img, w = ctx.saved_tensors
        B, Cin, H, W = img.shape
        Cout, k = int(w.shape[0]), int(w.shape[2])
        g = nhwc(g)
        dw = db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum((0, 2, 3))
        if ctx.needs_input_grad[1]:
            dwb = grad_home(w, _grad_taken_unread(w))
            _wgrad_async(lambda: stem_wgrad_raw(img, g, B, Cin, H, W, Cout, k, dwb), img.device, weights=(w,))
            dw = _alias(dwb)
        return None, dw, db


class StemTail(torch.autograd.Function):
    """pool0(relu(norm0(x0 + conv2d_dw_group(x0, k)))) in training mode (network.py:177-181 with torchvision's densenet121
    features norm0 / relu0 / pool0 = BatchNorm2d(64), ReLU, MaxPool2d(3, 2, 1)) on the channels-last stem output x0
    [B,64,H,W], k [B or 1,64,3,3], in three passes over the 157 MB tensor forward and four backward (csrc/stem.hip):
      forward   m = x0 + dw(x0, k) with norm0's batch statistics as column-sum partials in the same pass; fold; max-pool of
                relu(scale m + shift) with argmax bytes -- the normalised tensor is never written
      backward  pass 1 re-forms the masked un-pooled gradient on the fly for (d shift, d scale); fold; pass 2 re-forms it
                again and writes dm through BatchNorm's output and statistics; dx0 = dm + dw(dm, rot180 k); dk.
    Returns the pooled tensor; gradients for x0, k, gamma, beta."""

    @staticmethod
    def forward(ctx, x0, k, gamma, beta, bn):
        x0 = nhwc(x0)
        B, C, H, W = x0.shape
        dev = x0.device
        kc = k.detach().float().contiguous()
        kbs = C * 9 if kc.shape[0] > 1 else 0
        n = B * H * W
        m = torch.empty_like(x0)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        out = empty_nhwc(B, C, Ho, Wo, dev)
        idx = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            P = _lib.fn("ossid_dw_add_stats_partials")(B, H, W, C)
            if P <= 0:
                raise ValueError("StemTail: unsupported shape %s" % (tuple(x0.shape),))
            part = _scratch("stem_stats", P * 2 * C * 4, dev)
            pivot = new_buf((C,), dev)
            _lib.check(_lib.fn("ossid_dw_add_stats_nhwc")(x0.data_ptr(), kc.data_ptr(), kbs, B, H, W, C, 0, m.data_ptr(),
                                                          part.data_ptr(), pivot.data_ptr(), _lib.stream()), "ossid_dw_add_stats_nhwc")
            f = bn_fold_fwd((part, P, pivot), C, n, gamma, beta, bn.eps, _mom(bn),
                            bn.running_mean if bn.track_running_stats else None,
                            bn.running_var if bn.track_running_stats else None)
            _lib.check(_lib.fn("ossid_stem_pool_fwd")(m.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), B, H, W, C, out.data_ptr(),
                                                      idx.data_ptr(), _lib.stream()), "ossid_stem_pool_fwd")
        ctx.save_for_backward(x0, m, kc, idx, f, gamma)
        ctx.k_shape = tuple(k.shape)
        return out

    @staticmethod
    def backward(ctx, dp):
        x0, m, kc, idx, f, gamma = ctx.saved_tensors
        B, C, H, W = x0.shape
        dev = x0.device
        n = B * H * W
        dp = nhwc(dp)
        kbs = C * 9 if kc.shape[0] > 1 else 0
        pool_bwd = _lib.fn("ossid_stem_pool_bwd")
        with _lib.on_device(dev):
            P = _lib.fn("ossid_stem_pool_bwd_partials")(B, H, W, C)
            part = _scratch("stem_stats", P * 2 * C * 4, dev)
            _lib.check(pool_bwd(m.data_ptr(), idx.data_ptr(), dp.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), None, None,
                                B, H, W, C, part.data_ptr(), None, _lib.stream()), "ossid_stem_pool_bwd")
            r = torch.empty((4, C), dtype=torch.float32, device=dev)            # dgamma, dbeta, coef_x, coef_1
            bn_fold_bwd(None, None, gamma, f[2], f[3], C, n, r[0], r[1], r[2], r[3], partials=(part, P))
            dm = torch.empty_like(m)
            _lib.check(pool_bwd(m.data_ptr(), idx.data_ptr(), dp.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), r[2].data_ptr(),
                                r[3].data_ptr(), B, H, W, C, None, dm.data_ptr(), _lib.stream()), "ossid_stem_pool_bwd")
            dx0 = dk = None
            if ctx.needs_input_grad[0]:
                dx0 = torch.empty_like(x0)
                _lib.check(_lib.fn("ossid_dw_add_nhwc")(dm.data_ptr(), kc.data_ptr(), kbs, B, H, W, C, 1, dx0.data_ptr(), _lib.stream()),
                           "ossid_dw_add_nhwc")
            if ctx.needs_input_grad[1]:
                ws = _scratch("dwk", _lib.fn("ossid_dw_bwd_k_workspace_floats")(B, H, W, C) * 4, dev)
                dkb = torch.empty((B, C, 3, 3), dtype=torch.float32, device=dev)
                _lib.check(_lib.fn("ossid_dw_bwd_k_nhwc")(x0.data_ptr(), dm.data_ptr(), B, H, W, C, ws.data_ptr(), dkb.data_ptr(),
                                                          _lib.stream()), "ossid_dw_bwd_k_nhwc")
                dk = dkb if ctx.k_shape[0] > 1 else dkb.sum(0, keepdim=True)
        return dx0, dk, r[0], r[1], None


def stem_tail(x0, k, bn):
    """Template modulation + training norm0 + ReLU + pool0 behind the stem convolution (StemTail)."""
    return StemTail.apply(x0, k, bn.weight, bn.bias, bn)


def stem_conv(img, conv):
    """Apply DenseNet's conv0 (7x7 / stride 2 / padding 3, 3 -> 64) through StemConv."""
    return StemConv.apply(img, conv.weight, conv.bias)


def dense_block_train(x, block):
    params = []
    for layer in block.values():
        params += [layer.norm1.weight, layer.norm1.bias, layer.conv1.weight, layer.norm2.weight, layer.norm2.bias,
                   layer.conv2.weight]
    return DenseBlockTrain.apply(x, block, *params)


def bn_relu_conv(x, bn, conv, relu=True, act_elu=False, want_stats=False, deciding=False):
    """Training-mode BatchNorm (+ReLU) in front of a convolution, folded into its input staging. deciding: the output
    goes on into a BatchNorm + ReLU (a DenseNet transition): exact-f32 launch, see FWD_DECIDING."""
    B, C, H, W = x.shape
    scale, shift = bn_fold(ColStats.apply(x), B * H * W, bn)
    with exact_forward(deciding):
        return fused_conv(x, conv, pre=(scale, shift), pre_relu=relu, act_elu=act_elu, want_stats=want_stats)


def bump_batches_tracked(module):
    """num_batches_tracked += 1 for every BatchNorm of `module` in ONE multi-tensor launch (the folded BatchNorms above
    update running_mean / running_var in their own kernel but not the counter)."""
    ts = [m.num_batches_tracked for m in module.modules()
          if isinstance(m, torch.nn.BatchNorm2d) and m.num_batches_tracked is not None]
    if ts:
        torch._foreach_add_(ts, 1)
