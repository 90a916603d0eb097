"""The cases of the scorer's training-kernel edge tests (csrc/pn2_train.hip, SPEC.md 12): shapes, input builders and a
restatement of the kernels' own chunk arithmetic (wgrad_split, stat_chunks). tests/test_pn2_train_edges.py asserts on the
host that every case lands on the edge it is named for, tests/test_pn2_train_edges_gpu.py runs them.

Nothing here touches the GPU."""
import functools

import numpy as np
import torch

import ref_pn2_train as rt

STAT_MAX_CHUNKS = 256


# ---- the kernels' chunk arithmetic, restated ----------------------------------------------------------------------------------
def wgrad_split(R):
    """(chunk, splits, rows in the last split) of linear_wgrad: at least 512 rows per split, at most 256 splits, the chunk
    a multiple of the 16-deep slice."""
    ch = max((R + 255) // 256, 512)
    ch = (ch + 15) // 16 * 16
    splits = max((R + ch - 1) // ch, 1)
    return ch, splits, R - (splits - 1) * ch


def stat_chunks(R):
    """(chunks, rows per chunk, rows in the last chunk) of colstats_kernel and bn_bwd_reduce_kernel."""
    n = min(max((R + 255) // 256, 1), STAT_MAX_CHUNKS)
    rpc = (R + n - 1) // n
    nchunk = (R + rpc - 1) // rpc
    return nchunk, rpc, R - (nchunk - 1) * rpc


def gemm_slices(K):
    """(16-deep slices, depth of the last one, accumulators in use) of one split of K in gemm_kernel."""
    s = (K + 15) // 16
    return s, K - (s - 1) * 16, min(s, 8)


# ---- 1, 2, 4: the three GEMM settings -------------------------------------------------------------------------------------------
GEMM_R = (1, 31, 32, 33, 63, 64, 65, 129)
GEMM_C = (1, 31, 33, 63, 64, 65, 129)
GEMM_KR = (1, 7, 8, 15, 16, 17, 127, 128, 129, 131, 259, 1024)


def _grid():
    """(R, C, Kr): every Kr twice, against the R and C lists walked at two offsets, so that every value stands in every role
    and meets neighbours on both sides of a tile edge; then the corners."""
    out = []
    for off_r, off_c in ((0, 0), (3, 5)):
        for i, kr in enumerate(GEMM_KR):
            out.append((GEMM_R[(i + off_r) % len(GEMM_R)], GEMM_C[(i + off_c) % len(GEMM_C)], kr))
    out += [(65, 65, 65), (129, 129, 129), (1, 129, 1), (129, 1, 1024), (1, 1, 1024)]
    seen, uniq = set(), []
    for t in out:
        if t not in seen:
            seen.add(t)
            uniq.append(t)
    return uniq


GEMM_GRID = _grid()
# ragged M, N and K at once, small and large: the subset held to float64 on real-valued inputs
GEMM_REAL = [(1, 1, 1), (33, 31, 7), (63, 65, 17), (65, 33, 127), (129, 63, 129), (31, 129, 131), (65, 65, 259), (33, 65, 1024)]
WGRAD_REAL_R = (544, 131073)


def kp_variants(Kr):
    """The padded widths a case runs at: none, the group kernel's (a multiple of 8), and an odd one."""
    return sorted({Kr, (Kr + 7) // 8 * 8, Kr + 9})


def gid(t):
    return "-".join(str(v) for v in t)


def int_matrix(rows, cols, seed, lo=-3, hi=3):
    """Small integers as float32: every product and every partial sum of them is exact in float32."""
    return torch.randint(lo, hi + 1, (rows, cols), generator=torch.Generator().manual_seed(seed)).float()


def gemm_operands(R, C, Kr, real=False):
    """X [R, Kr], W [C, Kr], dZ [R, C]."""
    if not real:
        return int_matrix(R, Kr, 3 * R + Kr), int_matrix(C, Kr, 5 * C + Kr + 1), int_matrix(R, C, 7 * R + C + 2)
    g = torch.Generator().manual_seed(R + Kr + C)
    return torch.randn(R, Kr, generator=g), torch.randn(C, Kr, generator=g) / Kr ** 0.5, torch.randn(R, C, generator=g)


def padded(X, Kp, fill):
    """X [R, Kr] in a [R, Kp] matrix whose pad columns hold `fill`."""
    out = torch.full((X.shape[0], Kp), float(fill))
    out[:, :X.shape[1]] = X
    return out


def exact(a, b):
    """The product of two integer-valued float32 matrices through int64, as float32."""
    return (a.long() @ b.long()).float()


# ---- 3: weight-gradient splits ---------------------------------------------------------------------------------------------------
WGRAD_R = (511, 512, 513, 544, 1040, 65537, 131072, 131073, 133120)
WGRAD_C, WGRAD_KR = 64, 8
# R: (chunk, splits, rows in the last split)
WGRAD_TABLE = {513: (512, 2, 1), 544: (512, 2, 32), 1040: (512, 3, 16), 65537: (512, 129, 1), 131073: (528, 249, 129),
               133120: (528, 253, 64)}

# ---- 5: BatchNorm statistics -----------------------------------------------------------------------------------------------------
STATS_R = (1, 2, 3, 5, 255, 257, 513, 544, 65536, 65537, 70001)
STATS_C = (1, 63, 64, 65, 1024)
# the widest C stays with the short matrices: 70001 x 64 floats is the largest operand
STATS_CASES = [(1, 1), (1, 1024), (2, 63), (2, 1024), (3, 64), (3, 1), (5, 65), (5, 1024), (255, 65), (255, 1024), (257, 63),
               (257, 1024), (513, 64), (513, 1024), (544, 65), (544, 1024), (65536, 64), (65537, 65), (65537, 1), (70001, 63),
               (70001, 64)]
# R: (chunks, rows per chunk, rows in the last chunk or None where the table leaves it open)
STATS_TABLE = {513: (3, 171, None), 544: (3, 182, 180), 65537: (256, 257, 2), 70001: (256, 274, 131)}


def stats_input(R, C):
    """Integers in [-8, 8]: the float64 sums of z and z^2 are exact."""
    return int_matrix(R, C, 11 * R + C, -8, 8)


def stats_expected(z):
    """mean, rstd, var as stats_finalize_kernel forms them, in numpy float64, each cast to float32."""
    a = z.numpy().astype(np.float64)
    R = a.shape[0]
    mean = a.sum(0) / R
    var = np.maximum((a * a).sum(0) / R - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    return mean.astype(np.float32), rstd.astype(np.float32), var.astype(np.float32)


# ---- 6: BatchNorm + ReLU + max-pool ----------------------------------------------------------------------------------------------
POOL_CASES = [(1, 1, 1), (3, 2, 63), (5, 32, 65), (7, 64, 129), (2, 65, 64)]


def pool_inputs(G, S, C):
    """Z [G, S, C], mean, rstd, gamma (positive), beta, and the groups made by hand: {'negative': g, 'repeated': g, 'last': g}
    as far as G has room. Group `negative` ends below zero in every row and channel, group `repeated` has one value above
    everything at s = 0 and again at s = S - 1, group `last` is `negative` with one positive row at s = S - 1."""
    g = torch.Generator().manual_seed(100 * G + 10 * S + C)
    Z = torch.randn(G, S, C, generator=g)
    mean, rstd = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g)
    low = mean - (1.0 + beta.abs() / gamma) / rstd                  # bn(low) = -gamma - |beta| + beta < 0, with room for rounding
    made = {}
    made["negative"] = 0
    Z[0] = low - torch.rand(S, C, generator=g)
    if G >= 2:
        made["repeated"] = 1
        Z[1, 0] = 50.0
        Z[1, S - 1] = 50.0
    if G >= 3:
        made["last"] = 2
        Z[2] = low - torch.rand(S, C, generator=g)
        Z[2, S - 1] = mean + 3.0 / rstd + beta.abs() / (gamma * rstd)
    return Z, mean, rstd, gamma, beta, made


def pool_expected(Z, mean, rstd, gamma, beta):
    """relu(bn(z)) in float32 torch by the kernel's two steps, its maximum over S and the first arg-max."""
    a = (((Z - mean) * rstd) * gamma + beta).clamp(min=0)
    return a, a.max(1).values, rt.first_argmax(a)


# ---- 7: ungroup --------------------------------------------------------------------------------------------------------------------
UNGROUP_N = (1, 3, 4, 5, 64)
UNGROUP_E = (1, 63, 64, 65, 130)
UNGROUP_CF = (1, 63, 64, 65, 255, 256, 257, 300)
# (B, E, n, Cf, kind): kind 'random' leaves the last target (n >= 3: the last two) without an entry, 'equal' sends every entry
# to one target, 'perm' is a permutation of the targets (E == n)
UNGROUP_CASES = [(1, 1, 1, 1, "perm"), (3, 63, 3, 63, "random"), (1, 64, 4, 64, "random"), (3, 65, 5, 65, "random"),
                 (1, 130, 64, 255, "random"), (3, 1, 3, 256, "random"), (1, 63, 4, 257, "equal"), (3, 64, 5, 300, "equal"),
                 (1, 65, 64, 1, "random"), (3, 130, 1, 63, "equal"), (1, 64, 64, 300, "perm"), (3, 64, 64, 257, "perm"),
                 (1, 130, 5, 256, "random"), (3, 65, 3, 255, "equal"), (1, 1, 5, 64, "equal"), (3, 130, 4, 65, "random")]


def ungroup_inputs(B, E, n, Cf, kind):
    """idx [B, E] long, dG [B, E, Cf] integer-valued float32."""
    g = torch.Generator().manual_seed(1000 * E + 10 * n + Cf + B)
    if kind == "equal":
        idx = torch.randint(0, n, (B, 1), generator=g).expand(B, E).contiguous()
    elif kind == "perm":
        assert E == n
        idx = torch.stack([torch.randperm(n, generator=g) for _ in range(B)])
    else:
        idx = torch.randint(0, max(n - (2 if n >= 3 else 1), 1), (B, E), generator=g)
    dG = torch.randint(-3, 4, (B, E, Cf), generator=g).float()
    return idx, dG


def ungroup_expected(idx, dG, n):
    B, E, Cf = dG.shape
    want = torch.zeros(B, n, Cf, dtype=torch.int64)
    for b in range(B):
        want[b].index_add_(0, idx[b], dG[b].long())
    return want.float()


# ---- whole model -------------------------------------------------------------------------------------------------------------------
# name: (B, M, npoint1, npoint2)
WHOLE = {"E1": (2, 32, 32, 32), "E2": (17, 256, 64, 32), "E3": (2, 640, 512, 128)}
RADIUS1, RADIUS2 = 0.2, 0.4


def mixed_density(B, M, seed=3):
    """rt.make_inputs with the first half of every set's points moved into a disc of radius 0.08 (uniform in area) about a
    centre of its own in [-0.3, 0.3]^2: balls in the disc overflow, balls outside it stay short."""
    x = rt.make_inputs(B, M, seed)
    g = torch.Generator().manual_seed(1000 + seed)
    h = M // 2
    centre = 0.6 * torch.rand(B, 1, 2, generator=g) - 0.3
    r = 0.08 * torch.sqrt(torch.rand(B, h, generator=g))
    phi = 2 * np.pi * torch.rand(B, h, generator=g)
    x[:, :h, 0:2] = centre + torch.stack([r * torch.cos(phi), r * torch.sin(phi)], -1)
    return x


def constant_input(B, M, seed=3):
    """Every point of every set is the one point (0.25, -0.125, 0.5) with one feature vector."""
    x = rt.make_inputs(1, 1, seed).expand(B, M, 8).clone()
    x[..., 0], x[..., 1], x[..., 2] = 0.25, -0.125, 0.5
    return x


WHOLE_INPUTS = {"E1": lambda B, M: rt.make_inputs(B, M, 3), "E2": mixed_density, "E3": mixed_density}


def hits(xyz, centres, radius):
    """[B, S] points of xyz within `radius` of each centre, by the ball query's own float32 expression."""
    d = centres[:, :, None, :] - xyz[:, None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return (d2 < radius * radius).sum(-1)


def ball_counts(x, idx):
    """Hits per ball at both levels, [B * npoint1] and [B * npoint2], on the restatement's sampling."""
    xyz = x[..., 0:3]
    xyz1 = xyz.gather(1, idx["fps1"][..., None].expand(-1, -1, 3))
    xyz2 = xyz1.gather(1, idx["fps2"][..., None].expand(-1, -1, 3))
    return hits(xyz, xyz1, RADIUS1).reshape(-1), hits(xyz1, xyz2, RADIUS2).reshape(-1)


@functools.lru_cache(maxsize=None)
def whole_inputs(name):
    """(x, restatement's sampling) of a whole-model case."""
    B, M, np1, np2 = WHOLE[name]
    x = WHOLE_INPUTS[name](B, M)
    return x, rt.sample(x, np1, np2, RADIUS1, RADIUS2)


def decisions_that_differ(free_a, free_b):
    """(decisions in all, decisions that differ, the worst margin in free_b's values of a decision taken as free_a took it)
    between two records of rt.forward."""
    total, differ, worst = 0, 0, 0.0
    for l in range(11):
        bad = free_a["relu"][l] != free_b["relu"][l]
        total += bad.numel()
        differ += int(bad.sum())
        if bad.any():
            worst = max(worst, float(free_b["y"][l][bad].abs().max()))
    for m in range(3):
        a = free_b["pool_in"][m]
        got = free_a["argmax"][m]
        bad = got != free_b["argmax"][m]
        total += bad.numel()
        differ += int(bad.sum())
        if bad.any():
            gap = a.max(1).values - a.gather(1, got[:, None, :]).squeeze(1)
            worst = max(worst, float(gap[bad].max()))
    return total, differ, worst
