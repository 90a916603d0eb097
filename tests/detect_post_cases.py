"""Inputs of the detection post-processing / AMSGrad edge tests (csrc/dtoid.hip: ossid_topk, _decode_clip_boxes, _nms,
_detect_post, _detect_emit, _gather_rows, _amsgrad_step), built once and shared by the CPU tests
(tests/test_detect_post_edges.py: the premises, the restatement against today's yardsticks) and the GPU tests
(tests/test_detect_post_edges_gpu.py: the entries against the restatement tests/ref_detect_post.py), in the manner of
tests/ppf_cases.py.

Every builder asserts that the edge a case is named after occurs and records the figures in case["premise"]: a case
cannot pass vacuously. A case is a dict: name, the arrays and scalars of the entry it drives, `want` (the restatement's
outputs) and `premise`. Per group: topk_cases(), decode_cases(), nms_cases(), post_cases(), emit_cases(), gather_cases(),
amsgrad_cases()."""
import functools

import numpy as np
import torch

import ref_detect_post as rd

f32, f64 = np.float32, np.float64
EINVAL = -22
TOPK_CHUNK, TOPK_BLOCKS, TOPK_CAP = 2048, 512, 2048      # csrc/dtoid.hip: elements per block, most blocks, largest k
NMS_LDS_MAX, NMS_MAX = 1024, 16384                       # boxes the LDS scan takes, boxes the entry takes
AMS_GRID = 2048 * 256                                    # float4 the AMSGrad grid covers in one trip

NAMES = {
    "topk": ("t_n1_k1", "t_n2_k2", "t_n63_k63", "t_n257_k1", "t_n2048_k2048", "t_n2049_k2048", "t_n5000_k2047",
             "t_n5000_k1025", "t_n5000_k1024", "t_n1048577_k1000", "t_low_bits_level3", "t_low_bits_level2", "t_specials",
             "t_bin_boundary_all_ties", "t_bin_boundary_one_tie", "t_tie_run_across_chunks"),
    "decode": ("d_r1_a1_frame", "d_r255_a1", "d_r256_a1", "d_r257_a1", "d_r85_a3"),
    "nms": ("n_on_threshold", "n_above_threshold", "n_below_threshold") +
           tuple("n_chain_w%d_%d" % (w, n) for w in (6, 8) for n in (64, 65, 1024, 1025, 16384)) +
           tuple("n_dense_%d" % n for n in (1, 64, 65, 1024, 1025)) + ("n_touching_1024", "n_touching_1025") +
           ("n_dead_block_256", "n_dead_block_1089") + tuple("n_kept_per_block_%d" % c for c in (1, 2, 3, 5)) +
           ("n_zero_area", "n_random_3000"),
    "post": tuple("p_%s_t%d_a%d_k%d" % (v, t, a, k) for t, a, k in ((1, 3, 3), (2, 5, 10), (3, 96, 64), (21, 288, 288))
                  for v in ("random", "equal", "placed") if not (v == "placed" and t == 1)),
    "emit": ("e_seg35_scalar", "e_seg48_float4"),
    "gather": ("g_row4", "g_row_grid_stride"),
    "amsgrad": ("a_n4_lr1e-2", "a_n4_product", "a_second_trip_lr1e-2", "a_second_trip_product"),
}


def by_name(group):
    return {c["name"]: c for c in BUILDERS[group]()}


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


# ---- top-k ----------------------------------------------------------------------------------------------------------------
def topk_blocks(n):
    """(blocks, chunk) of the gather: min(512, ceil(n / 2048)) blocks, each with a contiguous chunk"""
    blocks = min(TOPK_BLOCKS, -(-n // TOPK_CHUNK))
    return blocks, -(-n // blocks)


def cut_figures(x, k):
    """the cut of a top-k: threshold value, elements above it, ties, ties taken, and how many radix levels decide it"""
    key = rd.order_key(x)
    T = np.sort(key)[::-1][k - 1]
    gt, eq = int((key > T).sum()), int((key == T).sum())
    return dict(T_bits="0x%08x" % int(T), above=gt, ties=eq, need_ties=k - gt,
                in_top_bin=int((key >> 21 == T >> 21).sum()), in_mid_bin=int((key >> 10 == T >> 10).sum()))


def _topk_case(name, x, k, **premise):
    x = np.ascontiguousarray(x, dtype=f32)
    vals, idx = rd.topk(x, k)
    assert len(idx) == k and len(set(idx.tolist())) == k
    return dict(name=name, x=x, k=k, want=dict(values=vals, indices=idx), premise=dict(cut_figures(x, k), n=x.size, k=k, **premise))


@functools.lru_cache(None)
def topk_cases():
    out = []
    rng = np.random.default_rng(11)
    for n, k in ((1, 1), (2, 2), (63, 63), (257, 1), (2048, 2048), (2049, 2048), (5000, 2047), (5000, 1025), (5000, 1024)):
        x = np.round(rng.normal(size=n) * 16) / 16                  # 1/16 steps: tie runs everywhere, the cut inside one
        out.append(_topk_case("t_n%d_k%d" % (n, k), x, k))
    n = TOPK_BLOCKS * TOPK_CHUNK + 1
    c = _topk_case("t_n%d_k1000" % n, np.round(rng.normal(size=n) * 64) / 64, 1000)
    assert topk_blocks(n) == (512, 2049) and c["premise"]["ties"] > c["premise"]["need_ties"] >= 1
    out.append(c)
    # every key equal in its top 22 bits: only the third level tells the elements apart
    x = (1.0 + rng.integers(0, 1024, 5000) * 2.0 ** -23).astype(f32)
    c = _topk_case("t_low_bits_level3", x, 1000)
    assert len(np.unique(rd.order_key(x) >> 10)) == 1 and len(np.unique(rd.order_key(x))) > 900
    out.append(c)
    # ... in their top 11 bits only: the second and third level both decide
    x = (1.0 + rng.integers(0, 2 ** 21, 5000) * 2.0 ** -23).astype(f32)
    x[::5] = np.sort(x)[::-1][700]                                  # a run of 1000 ties with at most 700 above it: the cut is inside
    c = _topk_case("t_low_bits_level2", x, 1000)
    assert len(np.unique(rd.order_key(x) >> 21)) == 1 and len(np.unique(rd.order_key(x) >> 10)) > 1000
    assert 1 < c["premise"]["in_mid_bin"] < c["premise"]["in_top_bin"]
    out.append(c)
    # sign and exponent: negatives, both zeros, denormals of both signs, both infinities, positive quiet NaNs with payloads
    u = rng.integers(0, 2 ** 32, 1500, dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)      # no NaN or infinity by accident
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7F800000, 0xFF800000,
                        0x7FC00000, 0x7FC00001, 0x7FD2345F, 0x7FFFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0x7FC00001], np.uint32)
    u[rng.choice(1500, len(special), replace=False)] = special
    x = u.view(f32)
    c = _topk_case("t_specials", x, 1400)
    got = set(bits(c["want"]["values"]).view(np.uint32).tolist())
    assert set(special.tolist()) - got == {0xFF800000} and c["premise"]["above"] > 700    # all but -inf are in the answer
    v = c["want"]["values"].view(np.uint32)
    assert v[:5].tolist() == [0x7FFFFFFF, 0x7FD2345F, 0x7FC00001, 0x7FC00001, 0x7FC00000] and v[5] == 0x7F800000
    z = np.flatnonzero((v << 1) == 0)
    assert v[z].tolist() == [0, 0, 0x80000000, 0x80000000]          # +0.0 before -0.0
    c["premise"].update(nan=5, zeros=4, negatives=int((v >> 31).sum()))
    out.append(c)
    # the cut on a bin boundary: T = 2.0 opens a top-level bin (its key's low 21 bits are 0), the float below it closes one
    x = (1.0 + rng.random(4000)).astype(f32)
    x[x >= 2.0] = 1.5
    x[:40] = np.nextafter(f32(2.0), f32(0.0))
    pos = rng.permutation(4000)
    x[pos[:600]] = (2.0 + rng.random(600) * 1.5 + 2.0 ** -20).astype(f32)
    x[pos[600:650]] = 2.0
    assert int(rd.order_key(np.array([2.0], f32))[0]) & 0x1FFFFF == 0
    for nm, k in (("t_bin_boundary_all_ties", 650), ("t_bin_boundary_one_tie", 601)):
        c = _topk_case(nm, x, k)
        p = c["premise"]
        assert p["T_bits"] == "0xc0000000" and p["above"] == 600 and p["ties"] == 50 and p["need_ties"] == k - 600
        assert int((x >= 2.0).sum()) == 650 and int((x == np.nextafter(f32(2.0), f32(0.0))).sum()) > 0
        out.append(c)
    # a tie run across the blocks' chunks, the cut inside chunk 1
    n = 3 * TOPK_CHUNK + 5
    blocks, chunk = topk_blocks(n)
    x = (rng.random(n) * 0.5).astype(f32)
    gt = rng.choice(n, 300, replace=False)
    x[gt] = (2.0 + rng.random(300)).astype(f32)
    x[::7] = 1.0
    ties = np.flatnonzero(x == 1.0)
    per = np.bincount(ties // chunk, minlength=blocks)
    k = int((x > 1.0).sum() + per[0] + per[1] // 2)
    c = _topk_case("t_tie_run_across_chunks", x, k)
    taken = np.bincount(c["want"]["indices"][x[c["want"]["indices"]] == 1.0] // chunk, minlength=blocks)
    assert blocks >= 3 and taken[0] == per[0] and 0 < taken[1] < per[1] and not taken[2:].any() and per[2] > 0
    c["premise"].update(blocks=blocks, chunk=chunk, ties_per_chunk=per.tolist(), taken_per_chunk=taken.tolist())
    out.append(c)
    return out


# ---- decode + clip --------------------------------------------------------------------------------------------------------
IMG_W, IMG_H = 40.0, 32.0
FRAME = (0.0, 0.0, IMG_W, IMG_H)
# delta rows whose box is known in closed form on the anchor they are put on: name -> (delta, what the f64 box must show)
DECODE_SPECIALS = (
    ("left_of_frame", (-100.0, 0.0, 0.0, 0.0), lambda b: b[0] == 0.0 and b[2] < 0.0),
    ("above_frame", (0.0, -100.0, 0.0, 0.0), lambda b: b[1] == 0.0 and b[3] < 0.0),
    ("exp_overflow", (0.0, 0.0, 500.0, 0.0), lambda b: b[0] == 0.0 and b[2] == IMG_W),
    ("width_zero", (0.25, 0.0, -500.0, 0.0), lambda b: b[0] == b[2] and 0.0 < b[0] < IMG_W),
)


@functools.lru_cache(None)
def decode_cases():
    out = []
    rng = np.random.default_rng(12)
    for name, R, A in (("d_r1_a1_frame", 1, 1), ("d_r255_a1", 255, 1), ("d_r256_a1", 256, 1), ("d_r257_a1", 257, 1), ("d_r85_a3", 85, 3)):
        if A == 1:
            anchors = np.array([FRAME if R == 1 else (8.0, 6.0, 24.0, 22.0)], f32)
        else:
            anchors = np.array([FRAME, (8.0, 6.0, 24.0, 22.0), (7.0, 9.0, 7.0, 9.0)], f32)       # the third has no size
        deltas = (rng.normal(size=(R, A, 4)) * 0.5).astype(f32)
        flat = deltas.reshape(-1, 4)
        premise = dict(total=R * A, A=A)
        flat[0] = 0.0                                               # on the frame anchor: lands exactly on 0 and on img_w / img_h
        if R * A > 1:
            live = [i for i in range(1, R * A) if i % A != 2][:len(DECODE_SPECIALS)]       # anchors with a size
            for i, (_nm, d, _f) in zip(live, DECODE_SPECIALS):
                flat[i] = d
        want = rd.decode_clip(anchors, deltas, IMG_W, IMG_H)
        wf = want.reshape(-1, 4)
        if anchors[0].tolist() == list(FRAME):
            assert wf[0].tolist() == list(FRAME)
            premise["exact_frame"] = True
        if R * A > 1:
            for i, (nm, _d, f) in zip(live, DECODE_SPECIALS):
                assert f(wf[i]), (name, nm, wf[i])
                premise[nm] = wf[i].tolist()
        if A == 3:
            assert (wf[2::3, 0] == wf[2::3, 2]).all() and (wf[2::3, 0] == 7.0).all()       # anchor i % A, row after row
            premise["zero_size_anchor_rows"] = R
        assert np.isfinite(want).all()
        premise["total_mod_256"] = (R * A) % 256
        out.append(dict(name=name, anchors=anchors, deltas=deltas, want=want, premise=premise))
    return out


def decode_f32(anchors, deltas, img_w=IMG_W, img_h=IMG_H):
    """the float32 torch computation of the same boxes (oracle/dtoid_oracle.py), for the error yardstick"""
    from oracle import dtoid_oracle
    return dtoid_oracle.decode_clip_boxes(torch.from_numpy(np.asarray(anchors)), torch.from_numpy(np.asarray(deltas)), img_w, img_h).numpy()


# ---- NMS ------------------------------------------------------------------------------------------------------------------
def _nms_case(name, boxes, wants, **premise):
    """wants: {thr: keep list in closed form}; the coordinates are integers below 2^24, so intersection and union are exact
    in float32 and a correctly rounded quotient falls on the same side of a representable threshold as the float64 one."""
    boxes = np.ascontiguousarray(boxes, dtype=f32)
    assert np.array_equal(boxes, np.round(boxes)) and np.abs(boxes).max(initial=0) < 2 ** 24
    return dict(name=name, boxes=boxes, want={float(t): np.asarray(k, dtype=np.int64) for t, k in wants.items()},
                premise=dict(n=len(boxes), kept={float(t): len(k) for t, k in wants.items()}, **premise))


def _unit(slot):
    """disjoint unit boxes away from everything else, one per slot"""
    return (100.0 + 2 * slot, 10.0, 101.0 + 2 * slot, 11.0)


def random_boxes(n, seed):
    """the box recipe of test_nms_matches_greedy_oracle, with its exact duplicate and its tied scores"""
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand(n, 2, generator=g) * 200
    wh = torch.rand(n, 2, generator=g) * 60 + 2
    boxes = torch.cat([ctr - wh / 2, ctr + wh / 2], 1)
    scores = torch.rand(n, generator=g)
    boxes[5] = boxes[2]
    scores[7] = scores[3]
    return boxes.numpy(), scores.numpy()


RANDOM_NMS_SEED, RANDOM_NMS_GAP = 0, 2e-6


@functools.lru_cache(None)
def nms_cases():
    out = []
    for name, w2, keep in (("n_on_threshold", 32, [0, 1]), ("n_above_threshold", 33, [0]), ("n_below_threshold", 31, [0, 1])):
        b = np.array([(0, 0, 64, 1), (0, 0, w2, 1)], f32)
        out.append(_nms_case(name, b, {0.5: keep}, iou=float(rd.iou(b[0], b[1]))))
    assert out[0]["premise"]["iou"] == 0.5 and out[1]["premise"]["iou"] > 0.5 > out[2]["premise"]["iou"]
    for w, every in ((6, 2), (8, 3)):
        for n in (64, 65, 1024, 1025, 16384):
            i = np.arange(n, dtype=f64)
            b = np.stack([i, 0 * i, i + w, 0 * i + 1], 1)
            ious = [float(rd.iou(b[0], b[d])) for d in (1, 2, 3)]
            assert ious == ([5 / 7, 0.5, 3 / 9] if w == 6 else [7 / 9, 0.6, 5 / 11])
            out.append(_nms_case("n_chain_w%d_%d" % (w, n), b, {0.5: np.arange(0, n, every)}, iou_to_next_three=ious))
    for n in (1, 64, 65, 1024, 1025):
        b = np.tile(np.array([(0, 0, 4, 4)], f32), (n, 1))
        words = rd.suppression_words(b, 0.5)[0]
        full = np.uint64(2 ** 64 - 1)
        want_words = [full if 64 * w + 64 <= n else np.uint64((1 << (n - 64 * w)) - 1) for w in range(len(words))]
        want_words[0] &= ~np.uint64(1)
        assert words.tolist() == [int(q) for q in want_words] and (n < 64 or all((int(q) >> 31) & (int(q) >> 63) & 1 for q in words[:n // 64]))
        assert not rd.suppression_words(b, 1.0).any()
        out.append(_nms_case("n_dense_%d" % n, b, {0.5: [0], 1.0: np.arange(n)}, iou=float(rd.iou(b[0], b[0])), mask_words=len(words)))
    for n in (1024, 1025):
        i = np.arange(n, dtype=f64)
        b = np.stack([i, 0 * i, i + 1, 0 * i + 1], 1)               # each touches the next: intersection 0, IoU 0, not > 0
        assert float(rd.iou(b[0], b[1])) == 0.0
        out.append(_nms_case("n_touching_%d" % n, b, {0.5: np.arange(n), 0.0: np.arange(n)}))
    for n in (256, 1089):
        b = np.array([_unit(s) for s in range(n)], f32)
        b[64:128] = b[0]
        out.append(_nms_case("n_dead_block_%d" % n, b, {0.5: [i for i in range(n) if not 64 <= i < 128]}, dead="64..127"))
    # block 1 keeps c boxes, its first box is dead but its row would remove a box of word 15 that must stay; the last kept
    # box of blocks 0 and 1 is box 63 of its block and removes a box of word 15; bit 31 of block 1's removed word is set
    # while boxes 32.. of it live
    for c in (1, 2, 3, 5):
        n = 1024
        b = np.array([_unit(s) for s in range(n)], f32)
        b[0] = (0, 0, 6, 1)
        b[64] = (1, 0, 7, 1)                                        # dead: IoU 5/7 with box 0
        b[990] = (2, 0, 8, 1)                                       # IoU 5/7 with box 64, exactly 0.5 with box 0: stays
        b[65:127] = b[1]                                            # dead copies of a kept box of block 0 (bit 31 among them)
        alive = [127] + [96 + 3 * q for q in range(c - 1)]          # c live boxes of block 1, all in its upper half
        for a in alive:
            b[a] = _unit(a)
        b[1000], b[1023] = b[127], b[63]
        dead = set(range(64, 127)) - set(alive) | {1000, 1023}
        keep = [i for i in range(n) if i not in dead]
        assert np.array_equal(rd.nms_sorted(b, 0.5), keep) and 990 in keep and sum(64 <= i < 128 for i in keep) == c
        assert float(rd.iou(b[0], b[990])) == 0.5 and float(rd.iou(b[64], b[990])) == 5 / 7
        row64 = rd.suppression_words(b, 0.5)[64]
        assert (int(row64[15]) >> (990 - 960)) & 1                  # what a wrong fill row would remove
        out.append(_nms_case("n_kept_per_block_%d" % c, b, {0.5: keep}, kept_in_block_1=c, alive=sorted(alive)))
    b = np.array([(5, 5, 5, 5), (5, 5, 5, 5), (0, 0, 4, 4)], f32)
    assert np.isnan(rd.iou(b[0], b[1]))
    out.append(_nms_case("n_zero_area", b, {0.5: [0, 1, 2]}, iou="nan"))
    # random: the float32 and the float64 IoU take the same side of the threshold on every pair
    boxes, scores = random_boxes(3000, RANDOM_NMS_SEED)
    order = torch.sort(torch.from_numpy(scores), descending=True, stable=True).indices.numpy()
    sb = boxes[order]
    iu = np.triu_indices(3000, 1)
    i64 = rd.iou(sb[:, None], sb[None])[iu]
    b32 = sb.astype(f32)
    ar = (b32[:, 2] - b32[:, 0]) * (b32[:, 3] - b32[:, 1])
    inter = np.clip(np.minimum(b32[:, None, 2], b32[None, :, 2]) - np.maximum(b32[:, None, 0], b32[None, :, 0]), 0, None) * \
        np.clip(np.minimum(b32[:, None, 3], b32[None, :, 3]) - np.maximum(b32[:, None, 1], b32[None, :, 1]), 0, None)
    i32 = (inter / ((ar[:, None] + ar[None, :]) - inter))[iu]
    gap, err = float(np.abs(i64 - 0.5).min()), float(np.abs(i32.astype(f64) - i64).max())
    assert gap >= RANDOM_NMS_GAP and err < RANDOM_NMS_GAP / 4, (gap, err)
    keep = rd.nms_sorted(sb, 0.5)
    out.append(dict(name="n_random_3000", boxes=boxes, scores=scores, order=order, want={0.5: order[keep]},
                    premise=dict(n=3000, seed=RANDOM_NMS_SEED, min_gap_to_threshold=gap, max_f32_iou_error=err, kept=len(keep),
                                 pairs=len(i64), excluded_pairs=0)))
    return out


# ---- detect_post ----------------------------------------------------------------------------------------------------------
POST_W, POST_H, POST_THR, POST_GAP = 64.0, 48.0, 0.5, 1e-5


def _post_case(name, obj, decoy, anchors, deltas, k, **premise):
    n_t, A = obj.shape
    cls = np.stack([decoy, obj], -1).astype(f32)                    # [n_t, A, 2]: class 1 is the object column
    vals, idx, boxes, keep = rd.detect_post(obj.reshape(-1), k, anchors, deltas, POST_W, POST_H, POST_THR)
    iu = np.triu_indices(k, 1)
    gap = float(np.nanmin(np.abs(rd.iou(boxes[:, None], boxes[None])[iu] - POST_THR))) if k > 1 else 1.0
    assert gap >= POST_GAP, (name, gap)                             # far more than a float32 decode can move an IoU
    return dict(name=name, cls=cls, anchors=anchors, deltas=deltas, k=k, n_t=n_t, A=A,
                want=dict(values=vals, indices=idx, boxes=boxes, keep=keep),
                premise=dict(n=n_t * A, k=k, kept=len(keep), min_iou_gap=gap, templates=sorted(set((idx[keep] // A).tolist())), **premise))


@functools.lru_cache(None)
def post_cases():
    out = []
    for n_t, A, k in ((1, 3, 3), (2, 5, 10), (3, 96, 64), (21, 288, 288)):
        rng = np.random.default_rng(1000 * n_t + A)
        ctr = rng.random((A, 2)) * (POST_W, POST_H)
        wh = rng.random((A, 2)) * 20 + 4
        anchors = np.concatenate([ctr - wh / 2, ctr + wh / 2], 1).astype(f32)
        deltas = (rng.normal(size=(n_t, A, 4)) * 0.5).astype(f32)
        # the class-0 column must never be read: NaN, and values above every object score
        decoy = np.where(np.arange(n_t * A).reshape(n_t, A) % 2 == 0, np.nan, 1e9).astype(f32)
        tag = "t%d_a%d_k%d" % (n_t, A, k)
        obj = (np.round(rng.random((n_t, A)) * 64) / 64).astype(f32)              # quantised: ties, also at the cut
        c = _post_case("p_random_" + tag, obj, decoy, anchors, deltas, k)
        assert n_t * A < 100 or c["premise"]["kept"] < k           # the NMS stage has work to do
        out.append(c)
        c = _post_case("p_equal_" + tag, np.full((n_t, A), 0.375, f32), decoy, anchors, deltas, k)
        assert np.array_equal(c["want"]["indices"], np.arange(k)) and (k > A or c["premise"]["templates"] == [0])
        out.append(c)
        if n_t > 1:
            obj = (rng.random((n_t, A)) * 0.25).astype(f32)
            d2 = deltas.copy().reshape(-1, 4)
            at = [A - 1, A, n_t * A - 1]
            obj.reshape(-1)[at] = (0.9, 0.8, 0.7)
            d2[at] = 0.0
            d2[at[2], 0] = 15.0 if anchors[A - 1, 0] < POST_W / 2 else -15.0      # 1.5 widths aside of the same anchor's first box
            c = _post_case("p_placed_" + tag, obj, decoy, anchors, d2.reshape(n_t, A, 4), k)
            w = c["want"]
            assert w["indices"][:3].tolist() == at and w["keep"][:2].tolist() == [0, 1] and 2 in w["keep"]
            assert (w["indices"][:3] // A).tolist() == [0, 1, n_t - 1]
            c["premise"]["placed"] = at
            out.append(c)
    return out


# ---- detect_emit / gather_rows --------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def emit_cases():
    out = []
    rng = np.random.default_rng(14)
    n_t, A, k = 4, 5, 10
    for name, shape in (("e_seg35_scalar", (5, 7)), ("e_seg48_float4", (6, 8))):
        vals = np.sort(rng.random(k).astype(f32))[::-1].copy()
        idx = np.array([A - 1, A, n_t * A - 1, 0, 7, 12, 3, 16, 10, 6], np.int64)
        boxes = rng.random((k, 4)).astype(f32) * 50
        keep = np.array([0, 2, 3, 7, 9], np.int32)
        seg = (rng.normal(size=(n_t,) + shape) * 3).astype(f32)
        seg[:, 0, 0], seg[:, -1, -1], seg[:, 2, 3] = 100.0, -100.0, 0.0
        heat = rng.random((n_t, 3, 4)).astype(f32)
        heat[1, 0, 0], heat[3, 2, 3] = np.nan, -0.0                 # copies: the bits come through
        row = shape[0] * shape[1]
        assert (row % 4 != 0) == (name == "e_seg35_scalar")
        tmpl = (idx[keep] // A).tolist()
        assert tmpl == [0, 3, 0, 3, 1] and len(set(tmpl)) < len(tmpl)          # a template row is read more than once
        out.append(dict(name=name, vals=vals, idx=idx, boxes=boxes, keep=keep, n_keep=len(keep), A=A, k=k, seg=seg, heat=heat,
                        premise=dict(seg_row=row, heat_row=12, templates=tmpl, kept=len(keep))))
    return out


@functools.lru_cache(None)
def gather_cases():
    rng = np.random.default_rng(15)
    small = rng.normal(size=(5, 4)).astype(f32)
    small[1], small[4, 0] = (100.0, -100.0, 0.0, -0.0), np.nan
    row = 4 * (1024 * 256 + 3)                                      # more float4 than the 1024 x 256 threads of a row's grid
    big = rng.normal(size=(3, row)).astype(f32)
    big[:, -1], big[:, 0] = -100.0, 100.0
    return [dict(name="g_row4", src=small, idx=np.array([4, 4, 3, 1, 1, 0], np.int64), premise=dict(row=4, repeated=2, descending=True)),
            dict(name="g_row_grid_stride", src=big, idx=np.array([2, 0], np.int64), premise=dict(row=row, float4_past_grid=3))]


# ---- AMSGrad ---------------------------------------------------------------------------------------------------------------
AMS_SCHEDULE = (1.0, 1.0, 0.01, 0.01, 0.01)
AMS_PAD = 64
FLOOR = 2.0 ** -24


def hyper(lr, wd, betas=(0.9, 0.999), eps=1e-8):
    """The entry takes its hyper-parameters as C floats; every computation of a case gets those float32 values (as Python
    floats), so the device, the float32 torch run and the float64 restatement compute the same function of the same
    inputs. (Against the decimal 0.999 the float beta2 is 1.3e-8 off, which is 1.3e-5 of 1 - beta2.)"""
    q = lambda v: float(f32(v))
    return dict(lr=q(lr), wd=q(wd), betas=(q(betas[0]), q(betas[1])), eps=q(eps))


def amsgrad_f32(p0, grads, h, first_step=1):
    """torch.optim.Adam(amsgrad=True) in float32 on the CPU -> [(p, exp_avg, exp_avg_sq, max_exp_avg_sq) after every step]"""
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, dtype=f32)))
    opt = torch.optim.Adam([p], lr=h["lr"], betas=h["betas"], eps=h["eps"], weight_decay=h["wd"], amsgrad=True, foreach=False)
    if first_step != 1:
        opt.state[p] = dict(step=torch.tensor(float(first_step - 1)), exp_avg=torch.zeros_like(p.data),
                            exp_avg_sq=torch.zeros_like(p.data), max_exp_avg_sq=torch.zeros_like(p.data))
    out = []
    for g in grads:
        p.grad = torch.from_numpy(np.array(g, dtype=f32))
        opt.step()
        s = opt.state[p]
        out.append(tuple(t.detach().clone().numpy() for t in (p.data, s["exp_avg"], s["exp_avg_sq"], s["max_exp_avg_sq"])))
    return out


def rel_err(got, want64):
    return float(np.abs(np.asarray(got, dtype=f64) - want64).max()) / float(np.abs(want64).max())


def bound(e32):
    """the `_bounded` rule of tests/test_pn2_train_gpu.py with its floor: 4 x max(float32 torch's error, one rounding)"""
    return 4.0 * max(e32, FLOOR)


@functools.lru_cache(None)
def amsgrad_cases():
    out = []
    for name, n, lr, wd in (("a_n4_lr1e-2", 4, 1e-2, 1e-3), ("a_n4_product", 4, 1e-4, 1e-6),
                            ("a_second_trip_lr1e-2", 4 * AMS_GRID + 4, 1e-2, 1e-3), ("a_second_trip_product", 4 * AMS_GRID + 4, 1e-4, 1e-6)):
        rng = np.random.default_rng(16 + n % 97)
        h = hyper(lr, wd)
        p0 = (rng.normal(size=n) * 1e-4).astype(f32)      # small against the steps: p's own rounding does not drown what is compared
        g = rng.normal(size=n).astype(f32)
        grads = [(g * f32(s)).astype(f32) for s in AMS_SCHEDULE]
        want = rd.amsgrad(p0, grads, h["lr"], h["betas"], h["eps"], h["wd"])
        adam = rd.amsgrad(p0, grads, h["lr"], h["betas"], h["eps"], h["wd"], use_max=False)
        ref32 = amsgrad_f32(p0, grads, h)
        below = [float((w[2] < w[3]).mean()) for w in want]                    # where exp_avg_sq is under its running maximum
        assert below[:2] == [0.0, 0.0] and min(below[2:]) >= 0.99
        move = want[-1][0] - p0.astype(f64)
        tol = bound(rel_err(ref32[-1][0].astype(f64) - p0.astype(f64), move)) * float(np.abs(move).max())
        share = float((np.abs(adam[-1][0] - want[-1][0]) > 100.0 * tol).mean())
        assert share >= 0.9, (name, share)
        assert 4 * AMS_GRID < n or n == 4
        out.append(dict(name=name, n=n, p0=p0, grads=grads, hyper=h, want=want, ref32=ref32,
                        premise=dict(n=n, below_max_share_per_step=below, adam_differs_by_100_bounds_share=share,
                                     bound_on_move=tol, adam_max_difference=float(np.abs(adam[-1][0] - want[-1][0]).max()))))
    return out


BUILDERS = {"topk": topk_cases, "decode": decode_cases, "nms": nms_cases, "post": post_cases, "emit": emit_cases,
            "gather": gather_cases, "amsgrad": amsgrad_cases}
