"""Plain-torch restatement of PointNet2SSG's TRAINING-mode arithmetic (SPEC.md 12), the yardstick of tests/test_pn2_train*.py.

Rows instead of NCHW between the layers: activations are [rows, channels] matrices, rows ordered (b, centre, sample). A layer is
z = X W^T and BatchNorm with the batch statistics of all rows (biased variance, eps 1e-5), evaluated by torch's own conv2d 1x1 /
linear and batch_norm on the layout the module would use, so that float64 rounding is the module's (tests/test_pn2_train.py);
ReLU is written as y * mask and max-pooling as gather(argmax). A padded sample of a ball-query group
is a repeat of the group's first sample; its pre-activations are taken from that row, so that repeats are equal bit for bit
(a BLAS gives equal rows at different places of a tile results that differ in the last bits, and "the first maximum" of
such a group would be noise). Mask and argmax are taken freely
(y > 0, the first maximum in sample order) or IMPOSED from outside, so a float32 implementation can be compared with
float64 under the decisions it actually took. Runs in any dtype under autograd. Channel order is torch's (xyz first).
"""
import torch
import torch.nn.functional as F

import ref_pointnet2 as ref

BN_EPS = 1e-5
LAYER_C = (64, 64, 128, 128, 128, 256, 256, 512, 1024, 512, 256)


def params_of(model, dtype, device="cpu"):
    """{'w': 12 x [cout, cin], 'gamma': 11, 'beta': 11, 'bias': [1]} as fresh leaves of dtype that require grad."""
    lin, bns = model.train_layers()

    def leaf(t):
        return t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
    return {"w": [leaf(m.weight.reshape(m.weight.shape[0], -1)) for m in lin], "gamma": [leaf(b.weight) for b in bns],
            "beta": [leaf(b.bias) for b in bns], "bias": leaf(lin[11].bias)}


def flat_params(p):
    return p["w"] + p["gamma"] + p["beta"] + [p["bias"]]


def ball_query(radius, nsample, xyz, new_xyz):
    """ref_pointnet2.ball_query, also for fewer than nsample points (its sorted list is then short): padded with the first
    hit to nsample entries all the same."""
    bq = ref.ball_query(radius, nsample, xyz, new_xyz)
    if bq.shape[-1] < nsample:
        n = xyz.shape[1]
        d = new_xyz[:, :, None, :] - xyz[:, None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        nhit = (d2 < radius * radius).sum(-1, keepdim=True)
        pad = bq[..., :1].expand(-1, -1, nsample - n)
        bq = torch.cat([torch.where(torch.arange(n).expand_as(bq) < nhit, bq, bq[..., :1].expand_as(bq)), pad], -1)
    return bq


def sample(point_x, npoint1, npoint2, radius1=0.2, radius2=0.4):
    """Sampling and grouping indices (SPEC.md 4.1) in point_x's own dtype: fps1 [B,np1], ball1 [B,np1,64], fps2, ball2."""
    xyz = point_x[..., 0:3].contiguous()
    fps1 = ref.furthest_point_sample(xyz, npoint1)
    xyz1 = xyz.gather(1, fps1[..., None].expand(-1, -1, 3))
    ball1 = ball_query(radius1, 64, xyz, xyz1)
    fps2 = ref.furthest_point_sample(xyz1, npoint2)
    xyz2 = xyz1.gather(1, fps2[..., None].expand(-1, -1, 3))
    ball2 = ball_query(radius2, 64, xyz1, xyz2)
    return {"fps1": fps1, "ball1": ball1, "fps2": fps2, "ball2": ball2}


def _take(x, idx):
    """x [B, n, C], idx [B, S, K] -> [B, S, K, C]"""
    B, S, K = idx.shape
    return x.gather(1, idx.reshape(B, S * K, 1).expand(-1, -1, x.shape[2])).reshape(B, S, K, x.shape[2])


def first_argmax(a):
    """a [G, S, C] -> the first index of the maximum along S, [G, C]"""
    S = a.shape[1]
    m = a.max(1, keepdim=True).values
    ar = torch.arange(S, device=a.device)[None, :, None].expand_as(a)
    return torch.where(a == m, ar, torch.full_like(ar, S)).min(1).values


def forward(p, point_x, idx, keep, p_drop, impose=None):
    """p: params_of(...); point_x [B, M, 8] (converted to the parameters' dtype); idx: sample(...); keep [B, 256] (0/1).
    impose: None, or {'relu': 11 x [rows, C] (non-zero = pass), 'argmax': 3 x [G, C]}.
    Returns scores [B, 1] and a record: 'relu' (11 bool), 'argmax' (3 long), 'y' (11 BatchNorm outputs), 'pool_in'
    (3 x [G, S, C] post-ReLU values), 'mean' / 'var' (11 batch statistics, biased variance), 'rows'."""
    dtype = p["bias"].dtype
    x = point_x.to(dtype)
    B = x.shape[0]
    rec = {"relu": [], "argmax": [], "y": [], "pool_in": [], "mean": [], "var": [], "rows": []}

    def layer(X, l, canon=None, shape=None):
        """shape (B, P, S): the rows are (b, j, s) and the layer runs as torch runs it on [B, K, P, S] -- conv2d 1x1 and
        batch_norm in NCHW -- so that its rounding is the module's (a float64 BatchNorm over the same values in another
        layout differs by 3e-15, which eleven layers amplify to the 1e-12 this restatement is pinned at)."""
        W, gamma, beta = p["w"][l], p["gamma"][l], p["beta"][l]
        if shape is None:
            z = F.linear(X, W)
            y = F.batch_norm(z, None, None, gamma, beta, True, 0.0, BN_EPS)
        else:
            Bq, P, S = shape
            z = F.conv2d(X.reshape(Bq, P, S, -1).permute(0, 3, 1, 2).contiguous(), W[:, :, None, None])
            z = z.permute(0, 2, 3, 1).reshape(-1, W.shape[0])
            if canon is not None:   # padded samples ARE their group's first sample: the same bits, whatever the BLAS does
                z = z[canon]        # with rows at different places of a tile
            y = F.batch_norm(z.reshape(Bq, P, S, -1).permute(0, 3, 1, 2).contiguous(), None, None, gamma, beta, True, 0.0, BN_EPS)
            y = y.permute(0, 2, 3, 1).reshape(-1, W.shape[0])
        with torch.no_grad():
            mean, var = z.mean(0), z.var(0, unbiased=False)
        mask = (y > 0) if impose is None else (impose["relu"][l].to(y.device) != 0)
        rec["relu"].append(mask.detach())
        rec["y"].append(y.detach())
        rec["mean"].append(mean)
        rec["var"].append(var)
        rec["rows"].append(z.shape[0])
        return y * mask.to(dtype)

    def pool(a, S, m):
        a = a.reshape(-1, S, a.shape[1])
        arg = first_argmax(a.detach()) if impose is None else impose["argmax"][m].to(a.device).reshape(a.shape[0], a.shape[2]).long()
        rec["argmax"].append(arg)
        rec["pool_in"].append(a.detach())
        return a.gather(1, arg[:, None, :]).squeeze(1)

    xyz, feats = x[..., 0:3], x[..., 3:]
    xyz1 = xyz.gather(1, idx["fps1"][..., None].expand(-1, -1, 3))
    xyz2 = xyz1.gather(1, idx["fps2"][..., None].expand(-1, -1, 3))
    np1, np2 = xyz1.shape[1], xyz2.shape[1]

    def canon_rows(ball):
        """row of (b, j, s) -> itself, or the row of (b, j, 0) where the sample is padding (a repeat of the first hit)"""
        rows = torch.arange(ball.numel(), device=ball.device).reshape(ball.shape)
        dup = (ball == ball[..., :1]) & (torch.arange(ball.shape[-1], device=ball.device) > 0)
        return torch.where(dup, rows[..., :1].expand_as(rows), rows).reshape(-1)

    c1, c2 = canon_rows(idx["ball1"]), canon_rows(idx["ball2"])
    g = torch.cat([_take(xyz, idx["ball1"]) - xyz1[:, :, None, :], _take(feats, idx["ball1"])], -1).reshape(-1, 8)
    s1 = (B, np1, 64)
    a = layer(g, 0, c1, s1)
    a = layer(a, 1, c1, s1)
    feat1 = pool(layer(a, 2, c1, s1), 64, 0).reshape(B, np1, 128)

    g = torch.cat([_take(xyz1, idx["ball2"]) - xyz2[:, :, None, :], _take(feat1, idx["ball2"])], -1).reshape(-1, 131)
    s2 = (B, np2, 64)
    a = layer(g, 3, c2, s2)
    a = layer(a, 4, c2, s2)
    feat2 = pool(layer(a, 5, c2, s2), 64, 1).reshape(B, np2, 256)

    g = torch.cat([xyz2, feat2], -1).reshape(-1, 259)
    s3 = (B, 1, np2)
    a = layer(g, 6, None, s3)
    a = layer(a, 7, None, s3)
    feat3 = pool(layer(a, 8, None, s3), np2, 2)

    a = layer(feat3, 9)
    a = layer(a, 10)
    a = a * (keep.to(dtype) * (1.0 / (1.0 - p_drop)))
    return a @ p["w"][11].t() + p["bias"], rec


def grads(p, scores, dscores):
    """The gradient of sum(scores * dscores) with respect to the 35 parameters, in flat_params order."""
    return torch.autograd.grad((scores * dscores.to(scores.dtype)).sum(), flat_params(p))


def make_inputs(B, M, seed):
    """The issue's inputs: xy uniform in [-0.5, 0.5]^2, z = 0, features N(0, 1); float32 [B, M, 8]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, M, 8)
    x[..., 0:2] = torch.rand(B, M, 2, generator=g) - 0.5
    x[..., 3:] = torch.randn(B, M, 5, generator=g)
    return x


def init_model(model, seed):
    """Random weights; BatchNorm gamma in [0.5, 1.5], beta ~ 0.2 N(0, 1); in place."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
    return model
