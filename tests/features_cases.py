"""Inputs of the keypoint-feature edge tests (SPEC.md section 11, csrc/features.hip), built once and shared by the CPU
tests (tests/test_features_edges.py: the premises) and the GPU tests (tests/test_features_edges_gpu.py: detect, describe,
match and hypotheses through the C ABI against the restatement tests/ref_features.py), in the manner of tests/ppf_cases.py.
Every stage takes its input from caller memory, so each edge is built directly: pyramid buffers, keypoint lists, descriptor
arrays and match rows are written here and no case hopes that an image contains it.

Every builder asserts on the restatement's output that the edge the case is named after occurs, and records the figures in
case["premise"]: a case cannot pass vacuously. A case is a dict: name, the arrays and scalar arguments of the entry point
it drives, `want` (the restatement's outputs) and `premise`. Per stage: detect_cases(), describe_cases(), match_cases(),
hypotheses_cases()."""
import functools

import numpy as np

import ref_features as rf

f32 = np.float32
DNT = 256                                               # csrc/features.hip: flat indices per detect block
SCAN_THREADS = 1024                                     # feat_scan_kernel: one block per thread up to this many blocks
S_TILE, MT_ROWS, M_CHUNK = 128, 128, 2048               # the matcher's scene tile, staged model tile and model chunk
LEVEL_MAX = 255 * 64                                    # 11.1: a grey level with 6 fractional bits

NAMES = {
    "detect": ("d_ratio_10", "d_ratio_9p5", "d_ratio_10p5", "d_large_ratio_1", "d_large_ratio_10", "d_large_ratio_9p99",
               "d_contrast_192", "d_contrast_191", "d_minimum_s2", "d_plateau", "d_corners_s1", "d_corners_s2",
               "d_octaves_mask_depth", "d_random_full_range", "d_scan_1024", "d_scan_1025", "d_scan_2049", "d_scan_3150",
               "d_cap4096_exact", "d_cap4096_plus1", "d_cap1_exact", "d_cap1_plus1"),
    "describe": ("b_window_border", "b_sample_rule", "b_flat", "b_two_peaks", "b_full_range", "b_normalisation", "b_frames",
                 "b_frames_negative_fx", "b_frame_border_unreachable"),
    "match": tuple("m_scene%d_cap%d" % (n, c) for n in (1, 32, 33, 64, 65, 127, 128, 129, 257) for c in (n, 4096))
    + ("m_scene4096", "m_over_cap") + tuple("m_model%d" % k for k in (127, 128, 129, 2047, 2048, 2049, 4097, 65536))
    + ("m_ties_both", "m_ties_higher_only", "m_ties_lower_only", "m_ties_one_lane", "m_ties_one_lane_higher_only", "m_weights",
       "m_weight_farthest"),
    "hypotheses": ("h_n1", "h_n255", "h_n256", "h_n257", "h_magnitudes", "h_over_cap"),
}


def by_name(stage):
    return {c["name"]: c for c in STAGE_BUILDERS[stage]()}


# ---- pyramids -----------------------------------------------------------------------------------------------------------
def pyramid_words(H, W, octaves):
    """int32 words of the device pyramid buffer: the octaves back to back, then two scratch planes of the frame."""
    return sum(5 * h * w for h, w in rf.octave_sizes(H, W, octaves)) + 2 * H * W


def pyramid_buffer(levels, H, W, octaves):
    """list per octave of [5,Ho,Wo] -> the int32 buffer ossid_feat_detect / _describe read (scratch planes: a poison value)."""
    sizes = rf.octave_sizes(H, W, octaves)
    assert [tuple(l.shape) for l in levels] == [(5, h, w) for h, w in sizes]
    buf = np.full(pyramid_words(H, W, octaves), -(1 << 30), dtype=np.int32)
    off = 0
    for l in levels:
        buf[off:off + l.size] = np.asarray(l, dtype=np.int32).ravel()
        off += l.size
    return buf


def levels_from_differences(D):
    """D int64 [4,H,W], D[s] = L[s+1] - L[s] -> levels [5,H,W] by cumulative sums, shifted to be non-negative."""
    L = np.concatenate([np.zeros((1,) + D.shape[1:], dtype=np.int64), np.cumsum(D, axis=0)])
    return L - min(0, int(L.min()))


def flat_levels(H, W, octaves, value=0):
    return [np.full((5, h, w), value, dtype=np.int64) for h, w in rf.octave_sizes(H, W, octaves)]


def random_levels(H, W, octaves, seed, hi=LEVEL_MAX):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, hi + 1, (5, h, w), dtype=np.int64) for h, w in rf.octave_sizes(H, W, octaves)]


def hessian(levels, kps):
    """(tr, det4) of 11.2 at keypoint rows, Python integers (no width)."""
    out = []
    for o, s, y, x in np.asarray(kps).tolist():
        D = (levels[o][s + 1] - levels[o][s]).astype(object)
        dxx = D[y, x + 1] + D[y, x - 1] - 2 * D[y, x]
        dyy = D[y + 1, x] + D[y - 1, x] - 2 * D[y, x]
        dxy4 = D[y + 1, x + 1] + D[y - 1, x - 1] - D[y + 1, x - 1] - D[y - 1, x + 1]
        out.append((int(dxx + dyy), int(4 * dxx * dyy - dxy4 * dxy4)))
    return out


def detect_blocks(H, W, octaves):
    return -(-sum(2 * h * w for h, w in rf.octave_sizes(H, W, octaves)) // DNT)


def flat_index(kps, H, W, octaves):
    """detect's flat index of keypoint rows: octave o owns 2 Ho Wo indices, (s - 1, y, x) row-major."""
    sizes = rf.octave_sizes(H, W, octaves)
    base = np.concatenate([[0], np.cumsum([2 * h * w for h, w in sizes])])
    k = np.asarray(kps, dtype=np.int64).reshape(-1, 4)
    hw = np.array(sizes, dtype=np.int64)[k[:, 0]]
    return base[k[:, 0]] + ((k[:, 1] - 1) * hw[:, 0] + k[:, 2]) * hw[:, 1] + k[:, 3]


def _dcase(name, levels, H, W, octaves, depth=None, mask=None, cap=64, **premise):
    depth = np.ones((H, W), dtype=f32) if depth is None else np.asarray(depth, dtype=f32)
    mask = np.ones((H, W), dtype=np.uint8) if mask is None else np.asarray(mask).astype(np.uint8)
    want = rf.detect(levels, depth, mask)
    premise = dict(premise, keypoints=len(want), blocks=detect_blocks(H, W, octaves))
    return dict(name=name, levels=levels, H=H, W=W, octaves=octaves, depth=depth, mask=mask, contrast=rf.CONTRAST, cap=cap,
                want=want, premise=premise)


def _pattern(D, s, y, x, c, a, b):
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            D[s, y + dy, x + dx] = c - a * abs(dx) - b * abs(dy)


def _single(name, c, a, b, kept, s=1, H=12, W=16, y=5, x=7, tweak=None, **premise):
    D = np.zeros((4, H, W), dtype=np.int64)
    _pattern(D, s, y, x, c, a, b)
    if tweak is not None:
        tweak(D)
    L = levels_from_differences(D)
    assert np.array_equal(L[1:] - L[:-1], D)
    case = _dcase(name, [L], H, W, 1, **premise)
    assert case["want"].tolist() == ([[0, s, y, x]] if kept else []), (name, case["want"])
    tr, det4 = hessian([L], [[0, s, y, x]])[0]
    case["premise"].update(kept=kept, tr=tr, det4=det4, lhs=4 * rf.EDGE_R * tr * tr, rhs=(rf.EDGE_R + 1) ** 2 * det4)
    return case


@functools.lru_cache(maxsize=None)
def _dense(H, W, octaves, seed):
    """A random full-range pyramid and the restatement's keypoints under a full mask."""
    levels = random_levels(H, W, octaves, seed)
    return levels, rf.detect(levels, np.ones((H, W), dtype=f32), np.ones((H, W), dtype=bool))


def _mask_keeping(all_kps, H, W, target, seed, forced=()):
    """A mask that is set only at full-resolution pixels of the restatement's own keypoints, chosen (the `forced` rows first,
    then in seeded order) so that exactly `target` keypoints survive. Pixels that several keypoints share count for all."""
    pix = (all_kps[:, 2] << all_kps[:, 0]) * W + (all_kps[:, 3] << all_kps[:, 0])
    uniq, inv, cnt = np.unique(pix, return_inverse=True, return_counts=True)
    order = list(dict.fromkeys([int(inv[i]) for i in forced]))
    seen = set(order)
    order += [int(u) for u in np.random.default_rng(seed).permutation(len(uniq)) if int(u) not in seen]
    mask = np.zeros(H * W, dtype=np.uint8)
    have = 0
    for u in order:
        if have + cnt[u] <= target:
            mask[uniq[u]] = 1
            have += int(cnt[u])
        if have == target:
            break
    assert have == target
    return mask.reshape(H, W)


def _scan_case(name, H, W, octaves, seed, target, cap=rf.MAX_KEYPOINTS):
    levels, full = _dense(H, W, octaves, seed)
    nb = detect_blocks(H, W, octaves)
    per = -(-nb // SCAN_THREADS)                        # wg_scan_range: blocks per scanning thread
    blk = flat_index(full, H, W, octaves) // DNT
    last = np.flatnonzero(blk == nb - 1)
    assert len(last) > 0, "%s: the full-mask pyramid has no keypoint in the last block" % name
    # forced: one keypoint in the last block, and a run of keypoints in eight consecutive blocks across a segment border
    b0 = (nb // 2 // per) * per - 4
    run = [int(np.flatnonzero(blk == b)[0]) for b in range(b0, b0 + 8)]
    mask = _mask_keeping(full, H, W, target, seed, forced=[int(last[0])] + run)
    c = _dcase(name, levels, H, W, octaves, mask=mask, cap=cap)
    kb = flat_index(c["want"], H, W, octaves) // DNT
    per_block = np.bincount(kb, minlength=nb)
    total = sum(2 * h * w for h, w in rf.octave_sizes(H, W, octaves))
    p = c["premise"]
    p.update(blocks=nb, per_thread=per, empty_blocks=int((per_block == 0).sum()), most_in_a_block=int(per_block.max()),
             adjacent_blocks=int((np.diff(kb) == 1).sum()), adjacent_segments=int((np.diff(kb // per) == 1).sum()),
             in_last_block=int(per_block[nb - 1]), last_block_size=total - (nb - 1) * DNT, full_mask_keypoints=len(full))
    assert len(c["want"]) == target and p["empty_blocks"] > 0 and p["most_in_a_block"] >= 2 and p["adjacent_blocks"] > 0
    assert p["in_last_block"] >= 1 and (per == 1 or p["adjacent_segments"] > 0)
    return c


# the shapes of the scan cases: blocks exactly 1024 (one per scanning thread), exactly 1025 (the first segmented count),
# at least 2049, and the product's 480 x 640 x 3 = 3150. The first three end in a partial block that reaches row H - 2 of
# the last octave, so that it can hold a keypoint; 480 x 640 ends on a block border (its last block is full).
SCAN_SHAPES = {"d_scan_1024": (239, 417, 3, 1024), "d_scan_1025": (281, 355, 3, 1025), "d_scan_2049": (373, 535, 3, 2049),
               "d_scan_3150": (480, 640, 3, 3150)}


@functools.lru_cache(maxsize=None)
def detect_cases():
    out = []
    # 1-3, 8-10: the 3 x 3 pattern c - a |dx| - b |dy|: tr = -2 (a + b), det4 = 16 a b, kept iff 10 (a + b)^2 < 121 a b
    out.append(_single("d_ratio_10", 1000, 10, 1, False))
    out.append(_single("d_ratio_9p5", 1000, 19, 2, True))
    out.append(_single("d_ratio_10p5", 1000, 21, 2, False))
    assert out[0]["premise"]["lhs"] == out[0]["premise"]["rhs"]                      # exactly on the threshold: strict <
    # 4-7: the same decisions where 40 tr^2 does not fit 32 bits
    for name, a, b, kept in (("d_large_ratio_1", 4000, 4000, True), ("d_large_ratio_10", 7000, 700, False),
                             ("d_large_ratio_9p99", 6993, 700, True)):
        c = _single(name, 16000, a, b, kept)
        assert c["premise"]["lhs"] > 2 ** 31
        out.append(c)
    assert out[4]["premise"]["lhs"] == out[4]["premise"]["rhs"]
    out.append(_single("d_contrast_192", 192, 50, 50, True))
    out.append(_single("d_contrast_191", 191, 50, 50, False))
    out.append(_single("d_minimum_s2", -192, -50, -50, True, s=2))

    def plateau(D):
        D[1, 5, 8] = 1000                                # the right neighbour as high as the centre: neither is strict
    c = _single("d_plateau", 1000, 50, 50, False, tweak=plateau)
    assert c["levels"][0][2, 5, 7] - c["levels"][0][1, 5, 7] == c["levels"][0][2, 5, 8] - c["levels"][0][1, 5, 8] == 1000
    out.append(c)
    # 11, 12: the four corners of the interior, at each level
    H, W = 12, 16
    for s in (1, 2):
        D = np.zeros((4, H, W), dtype=np.int64)
        corners = [(1, 1), (1, W - 2), (H - 2, 1), (H - 2, W - 2)]
        for y, x in corners:
            _pattern(D, s, y, x, 1000, 50, 50)
        c = _dcase("d_corners_s%d" % s, [levels_from_differences(D)], H, W, 1, corners=corners)
        assert c["want"].tolist() == [[0, s, y, x] for y, x in corners]
        out.append(c)
    out.append(_octaves_mask_depth())
    # 14: full-range levels, compared in full
    levels, full = _dense(40, 56, 3, 14)
    c = _dcase("d_random_full_range", levels, 40, 56, 3, cap=rf.MAX_KEYPOINTS)
    hs = hessian(levels, c["want"])
    wide = sum(1 for tr, det4 in hs if 40 * tr * tr >= 2 ** 31 or 121 * det4 >= 2 ** 31)
    c["premise"].update(beyond_32_bits=wide, max_40_tr2=max(40 * tr * tr for tr, _d in hs),
                        octaves_hit=sorted(set(c["want"][:, 0].tolist())))
    assert len(c["want"]) >= 100 and wide >= 1 and c["premise"]["octaves_hit"] == [0, 1, 2]
    out.append(c)
    # the scan paths
    for name, (H, W, octaves, nb) in SCAN_SHAPES.items():
        assert detect_blocks(H, W, octaves) == nb
        c = _scan_case(name, H, W, octaves, seed=nb, target=3000)
        assert (c["premise"]["last_block_size"] < DNT) == (name != "d_scan_3150")
        out.append(c)
    # the cap: the true count exactly cap and cap + 1
    H, W, octaves, _nb = SCAN_SHAPES["d_scan_1024"]
    levels, full = _dense(H, W, octaves, 1024)
    for cap in (rf.MAX_KEYPOINTS, 1):
        for extra, tag in ((0, "exact"), (1, "plus1")):
            c = _dcase("d_cap%d_%s" % (cap, tag), levels, H, W, octaves, mask=_mask_keeping(full, H, W, cap + extra, cap), cap=cap)
            assert len(c["want"]) == cap + extra
            c["premise"]["over"] = extra
            out.append(c)
    return out


def _octaves_mask_depth():
    """13: patterns in octaves 1 and 2 of an odd-sized frame; the mask or the depth cleared at exactly (y << o, x << o) for
    five of every seven, at a neighbouring full-resolution pixel for one, untouched for one."""
    H, W, octaves = 37, 53, 3
    sizes = rf.octave_sizes(H, W, octaves)
    assert sizes == [(37, 53), (19, 27), (10, 14)]
    Ds = [np.zeros((4, h, w), dtype=np.int64) for h, w in sizes]
    depth, mask = np.ones((H, W), dtype=f32), np.ones((H, W), dtype=np.uint8)
    how = ("keep", "mask", "zero", "minus_zero", "negative", "nan", "neighbour")
    spots, k = [], 0
    for o in (1, 2):
        h, w = sizes[o]
        # the first and the last interior row and column come first, so the spacing rule never drops (h - 2, w - 2)
        for y in [1, h - 2] + list(range(5, h - 2, 4)):
            for x in [1, w - 2] + list(range(5, w - 2, 4)):
                if spots and any(so == o and abs(sy - y) < 4 and abs(sx - x) < 4 for so, _s, sy, sx, _t in spots):
                    continue
                s, t = 1 + k % 2, how[k % len(how)]
                _pattern(Ds[o], s, y, x, 1000, 50, 50)
                fy, fx = y << o, x << o
                if t == "mask":
                    mask[fy, fx] = 0
                elif t == "neighbour":                  # the pixels around the sampled one are cleared, the one itself is not
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            if (dy or dx) and 0 <= fy + dy < H and 0 <= fx + dx < W:
                                mask[fy + dy, fx + dx], depth[fy + dy, fx + dx] = 0, 0.0
                elif t != "keep":
                    depth[fy, fx] = dict(zero=0.0, minus_zero=-0.0, negative=-1.0, nan=np.nan)[t]
                spots.append((o, s, y, x, t))
                k += 1
    levels = flat_levels(H, W, 1) + [levels_from_differences(D) for D in Ds[1:]]
    c = _dcase("d_octaves_mask_depth", levels, H, W, octaves, depth=depth, mask=mask)
    kept = [(o, s, y, x) for o, s, y, x, t in spots if t in ("keep", "neighbour")]
    assert sorted(map(tuple, c["want"].tolist())) == sorted(kept)
    by = {t: sum(1 for sp in spots if sp[4] == t) for t in how}
    assert all(by[t] >= 2 for t in how) and {sp[0] for sp in spots} == {1, 2}
    assert np.signbit(depth[depth == 0]).any() and np.isnan(depth).any()
    corner = sorted({(o, y, x) for o, _s, y, x, _t in spots if y == sizes[o][0] - 2 and x == sizes[o][1] - 2})
    assert corner == [(1, 17, 25), (2, 8, 12)]          # the last interior pixel of both octaves carries a pattern
    c["premise"].update(spots=len(spots), per_treatment=by, last_interior_pixel=corner)
    return c


# ---- describe -----------------------------------------------------------------------------------------------------------
K_PLAIN = (300.0, 310.0, 60.5, 47.25)                  # fx, fy, cx, cy


def cam_matrix(k):
    return [[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]]


@functools.lru_cache(maxsize=None)
def smooth_levels(H, W, octaves, seed, amp=1500.0, waves=10):
    """Per octave one smooth random surface (a sum of plane waves, 7 to 40 pixels long) in all five levels: a gradient of
    every direction somewhere, and no flat spot."""
    rng = np.random.default_rng(seed)
    out = []
    for h, w in rf.octave_sizes(H, W, octaves):
        yy, xx = np.mgrid[0:h, 0:w]
        f = np.full((h, w), 8000.0)
        for _ in range(waves):
            k, a = 2 * np.pi / rng.uniform(7.0, 40.0), rng.uniform(0, 2 * np.pi)
            f += amp * rng.uniform(0.3, 1.0) * np.sin(k * (np.cos(a) * xx + np.sin(a) * yy) + rng.uniform(0, 2 * np.pi))
        L = np.clip(np.rint(f), 0, LEVEL_MAX).astype(np.int64)
        out.append(np.stack([L] * 5))
    return out


GARBAGE = np.array([[7, 9, -5, 10 ** 9], [-1, 0, 1 << 30, -(1 << 30)], [3, 3, 70000, 70000]], dtype=np.int64)


def _bcase(name, levels, H, W, octaves, kps, depth=None, K=K_PLAIN, **premise):
    """cap = n + 3: the rows behind count hold keypoints that must never be read."""
    depth = np.full((H, W), 0.5, dtype=f32) if depth is None else np.asarray(depth, dtype=f32)
    kps = np.asarray(kps, dtype=np.int64).reshape(-1, 4)
    bins, desc, frames, ok = rf.describe_rows(levels, depth, cam_matrix(K), kps)
    n = len(kps)
    rows = np.concatenate([kps, GARBAGE]).astype(np.int32)
    premise = dict(premise, rows=n, ok=int(ok.sum()), window_dropped=int((bins < 0).sum()),
                   later_dropped=int(((bins >= 0) & ~ok).sum()))
    return dict(name=name, levels=levels, H=H, W=W, octaves=octaves, depth=depth, K=tuple(f32(v) for v in K), kps=rows, n=n,
                cap=n + len(GARBAGE), want=dict(bins=bins, desc=desc, frames=frames, ok=ok), premise=premise)


def _window_border():
    H, W, octaves = 96, 128, 3
    levels = smooth_levels(H, W, octaves, 21)
    kps, inside = [], []
    for o, (h, w) in enumerate(rf.octave_sizes(H, W, octaves)):
        for s in (1, 2):
            m = rf.RHO[s - 1] + 1
            for y, x, dy, dx in ((h // 2, m, 0, -1), (h // 2, w - 1 - m, 0, 1), (m, w // 2, -1, 0), (h - 1 - m, w // 2, 1, 0)):
                kps += [(o, s, y, x), (o, s, y + dy, x + dx)]
                inside += [True, False]
    c = _bcase("b_window_border", levels, H, W, octaves, kps)
    w = c["want"]
    inside = np.array(inside)
    assert (w["bins"][inside] >= 0).all() and (w["bins"][~inside] == -1).all() and not w["ok"].any()
    assert not w["desc"].any() and not w["frames"].any() and len(kps) == 48
    return c


def _sample_rule():
    H, W = 64, 80
    levels = smooth_levels(H, W, 1, 22)
    kps, walks = [], []
    for s in (1, 2):
        m = rf.RHO[s - 1] + 1
        for side in range(4):
            walk = []
            for t in range(11):
                y, x = ((H // 2 + 3, m + t), (H // 2 - 2, W - 1 - m - t), (m + t, W // 2 + 5), (H - 1 - m - t, W // 2 - 7))[side]
                walk.append(len(kps))
                kps.append((0, s, y, x))
            walks.append(walk)
    c = _bcase("b_sample_rule", levels, H, W, 1, kps)
    w = c["want"]
    first = []
    for walk in walks:
        assert (w["bins"][walk] >= 0).all()             # the orientation window is inside everywhere: only 11.4 decides
        kept = np.flatnonzero(w["ok"][walk])
        assert len(kept) > 0 and kept[0] > 0, "a walk must start dropped and end kept"
        first.append(int(kept[0]))
    bins = sorted(set(w["bins"].tolist()))
    assert len(bins) >= 4
    c["premise"].update(first_kept_step=first, orientation_bins=bins)
    return c


def _flat():
    H, W = 48, 48
    levels = flat_levels(H, W, 1, 5000)
    c = _bcase("b_flat", levels, H, W, 1, [(0, 1, 24, 24), (0, 2, 23, 25)])
    assert c["want"]["bins"].tolist() == [0, 0] and not c["want"]["ok"].any()
    return c


def _two_peaks():
    H = W = 41
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    L = np.rint(3000.0 * np.exp(-(xx - 20) ** 2 / 18.0) + 500.0 * np.exp(-(yy - 20) ** 2 / 30.0)).astype(np.int64)
    levels = [np.stack([L] * 5)]
    gx, gy = rf.gradients(L)
    hs = rf.smoothed_histogram(gx, gy, 1, 20, 20)
    peaks = np.flatnonzero(hs == hs.max()).tolist()
    c = _bcase("b_two_peaks", levels, H, W, 1, [(0, 1, 20, 20)], tie_bins=peaks, peak=int(hs.max()))
    assert peaks == [0, 18] and c["want"]["bins"].tolist() == [0]
    return c


def _full_range():
    H, W, octaves = 64, 80, 2
    levels = random_levels(H, W, octaves, 25)
    kps = [(0, s, y, x) for s in (1, 2) for y in (20, 28, 36, 44) for x in (20, 30, 40, 50, 60)]
    kps += [(1, 1, 16, 14), (1, 1, 16, 20), (1, 1, 15, 25)]
    c = _bcase("b_full_range", levels, H, W, octaves, kps)
    g2 = 0
    for o, s, y, x in kps:
        gx, gy = rf.gradients(levels[o][s])
        r = rf.RHO[s - 1]
        g2 = max(g2, int((gx * gx + gy * gy)[y - r:y + r + 1, x - r:x + r + 1].max()))
    # a central difference of levels in [0, 16320] is at most 16320, so gx^2 + gy^2 <= 2 * 16320^2 = 532 684 800 < 2^30:
    # no legal level reaches 2^30. Asserted instead: beyond 2^28, far past the 2^24 up to which float32 holds the sum exactly
    c["premise"]["max_gradient_squared"] = g2
    assert 2 ** 28 <= g2 <= 2 * LEVEL_MAX ** 2 and c["premise"]["ok"] >= 20 and c["want"]["ok"][-3:].any()
    return c


def _normalisation():
    """A straight step edge through the keypoint: energy in a few bins, so 11.4's 0.2 sqrt(S) cap clips; one bright pixel at
    a corner sample: energy in one cell, so the quantised value passes 127.

    Without clipping a bin is at most 0.2 sqrt(S), so q <= 256 * 0.2 = 51.2: a value of 52 or more proves that the cap
    clipped. Without the 127 clamp sum q^2 is 256^2 up to rounding (each of 128 values moves by at most 1/2, and
    sum q <= sqrt(128) * 256, so by less than 2929): a row with a 127 whose sum falls short of 65536 - 2929 was clamped."""
    H, W = 48, 48
    found = {}
    for amp in (4000, 16000):
        for dy in range(-12, 13):
            for dx in range(-12, 13):
                if "clamped" in found or max(abs(dy), abs(dx)) < 8:
                    continue
                L = np.full((H, W), 100, dtype=np.int64)
                L[24 + dy, 24 + dx] += amp
                gx, gy = rf.gradients(L)
                b = rf.orientation(gx, gy, 1, 24, 24)
                d = rf.descriptor(L, gx, gy, 1, 24, 24, b)
                if d is not None and d.max() == 127 and int((d.astype(np.int64) ** 2).sum()) < 65536 - 2929:
                    found["clamped"] = (L, (dy, dx, amp))
    assert "clamped" in found, "no bright-pixel pattern gives a clamped descriptor value"
    Lc, where = found["clamped"]
    Le = np.full((H, W), 100, dtype=np.int64)
    Le[:, 24:] = 9000
    L = np.concatenate([Le, Lc], axis=1)                # one level 48 x 96: the edge row at x = 24, the pixel row at x = 72
    c = _bcase("b_normalisation", [np.stack([L] * 5)], H, 2 * W, 1, [(0, 1, 24, 24), (0, 1, 24, 72)], bright_pixel=where)
    d = c["want"]["desc"].astype(np.int64)
    assert c["want"]["ok"].all()
    c["premise"].update(edge_row_max=int(d[0].max()), pixel_row_max=int(d[1].max()), pixel_row_sum_q2=int((d[1] ** 2).sum()),
                        edge_row_sum_q2=int((d[0] ** 2).sum()))
    assert 52 <= d[0].max() < 127 and d[1].max() == 127 and (d[1] ** 2).sum() < 65536 - 2929
    return c


def _raw_normal_faces_camera(depth, K, o, s, y, x):
    """11.5's n before the flip, in float64 from the float32 back-projections: True when n . P > 0 (the flip is taken)."""
    fx, fy, cx, cy = (f32(v) for v in K)
    xf, yf, r = x << o, y << o, rf.FRAME_R[s - 1] << o

    def bp(px, py):
        z = depth[py, px]
        return np.array([(f32(px) - cx) * z / fx, (f32(py) - cy) * z / fy, z], dtype=f32).astype(np.float64)
    n = rf._cross(bp(xf + r, yf) - bp(xf - r, yf), bp(xf, yf + r) - bp(xf, yf - r))
    return bool(rf._dot3(n, bp(xf, yf)) > 0.0)


def tolerance_floats(Z=f32(0.5)):
    """The largest zn above Z and the smallest below it that 11.5's |f32(zn - Z)| <= f32(0.05) Z keeps, by nextafter."""
    tol = f32(f32(0.05) * Z)

    def kept(zn):
        return bool(np.abs(f32(f32(zn) - Z)) <= tol)
    hi = f32(Z + tol)
    while not kept(hi):
        hi = np.nextafter(hi, f32(0), dtype=f32)
    while kept(np.nextafter(hi, f32(1), dtype=f32)):
        hi = np.nextafter(hi, f32(1), dtype=f32)
    lo = f32(Z - tol)
    while not kept(lo):
        lo = np.nextafter(lo, f32(1), dtype=f32)
    while kept(np.nextafter(lo, f32(0), dtype=f32)):
        lo = np.nextafter(lo, f32(0), dtype=f32)
    return hi, np.nextafter(hi, f32(1), dtype=f32), lo, np.nextafter(lo, f32(0), dtype=f32)


def _frames(name, K):
    """11.5 on the plane Z = 0.5: every keypoint sits in its own 32 x 32 cell of the frame and has one neighbour (or its
    centre) altered; three cells carry a tilted patch instead."""
    H, W, octaves = 352, 512, 3
    levels = smooth_levels(H, W, octaves, 27)
    Z = f32(0.5)
    depth = np.full((H, W), Z, dtype=f32)
    hi, hi_out, lo, lo_out = tolerance_floats(Z)
    # full-resolution centres 64 apart (the largest baseline is 24): the octave-2 rows take the central ones, where the
    # descriptor window of a 88 x 128 octave fits
    cells = [(cy, cx) for cy in range(48, H - 47, 64) for cx in range(48, W - 47, 64)]
    kps, expect, what = [], [], []

    def cell(o):
        k = next(i for i, (cy, cx) in enumerate(cells) if o < 2 or (80 <= cy <= H - 80 and 80 <= cx <= W - 80))
        return cells.pop(k)

    def put(o, s, side, value, keep, label, centre=False):
        cy, cx = cell(o)
        r = rf.FRAME_R[s - 1] << o
        py, px = ((cy, cx + r), (cy, cx - r), (cy + r, cx), (cy - r, cx))[side]
        if centre:
            py, px = cy, cx
        if label.startswith("beside"):                  # the pixels next to the sampled neighbour, not the neighbour itself
            depth[py - 1:py + 2, px - 1:px + 2] = value
            depth[py, px] = Z
        else:
            depth[py, px] = value
        kps.append((o, s, cy >> o, cx >> o))
        expect.append(keep)
        what.append(label)
    put(0, 1, 0, hi, True, "largest kept above")
    put(0, 1, 1, hi_out, False, "one ulp above")
    put(0, 2, 2, lo, True, "smallest kept below")
    put(0, 2, 3, lo_out, False, "one ulp below")
    for side, (v, label) in enumerate(((0.0, "zero"), (-0.0, "minus zero"), (np.nan, "nan"), (-0.5, "negative"))):
        put(0, 1 + side % 2, side, v, False, label + " neighbour")
    put(0, 1, 0, np.inf, False, "infinite neighbour")
    put(0, 1, 0, 0.0, False, "zero centre", centre=True)
    put(0, 2, 0, np.nan, False, "nan centre", centre=True)
    for o in (1, 2):
        for s in (1, 2):
            for side in range(4):
                if (side + s + o) % 2:
                    put(o, s, side, 0.0, False, "zero neighbour at r << o, octave %d level %d side %d" % (o, s, side))
                else:
                    put(o, s, side, 0.0, True, "beside the neighbour, octave %d level %d side %d" % (o, s, side))
    for gx_, gy_ in ((0.002, 0.0), (-0.002, 0.001), (0.0, -0.002)):                 # tilted patches, within the tolerance
        cy, cx = cell(0)
        yy, xx = np.mgrid[cy - 12:cy + 13, cx - 12:cx + 13]
        depth[cy - 12:cy + 13, cx - 12:cx + 13] = (0.5 + gx_ * (xx - cx) + gy_ * (yy - cy)).astype(f32)
        kps.append((0, 2, cy, cx))
        expect.append(True)
        what.append("tilted %g %g" % (gx_, gy_))
    c = _bcase(name, levels, H, W, octaves, kps, depth=depth, K=K)
    ok = c["want"]["ok"]
    wrong = [what[i] for i in range(len(kps)) if bool(ok[i]) != expect[i]]
    assert not wrong, (name, wrong)
    flips = sorted({_raw_normal_faces_camera(depth, K, *kp) for kp, k in zip(kps, ok) if k})
    nP = [float(rf._dot3(F[:3, 2], F[:3, 3])) for F in c["want"]["frames"][ok]]
    assert all(v < 0 for v in nP)                       # after the rule every normal faces the camera
    c["premise"].update(tolerance=[float(v) for v in (hi, hi_out, lo, lo_out)], rows_by_label=dict(zip(what, ok.tolist())),
                        flip_taken=flips)
    return c


def _frame_border_unreachable():
    """11.5's border rule (xf - r < 0 ...) on its own: rf.frame keeps xf - r == 0 and xf + r == W - 1 and drops one pixel
    further, but a keypoint that close to the border has lost its orientation window (rho + 1 > r) before, at every
    octave: through ossid_feat_describe the rule cannot decide a row. The rows are run all the same; all are dropped."""
    H, W, octaves = 96, 128, 3
    levels = smooth_levels(H, W, octaves, 21)
    depth = np.full((H, W), 0.5, dtype=f32)
    kps, alone = [], []
    for o, (h, w) in enumerate(rf.octave_sizes(H, W, octaves)):
        for s in (1, 2):
            r = rf.FRAME_R[s - 1]
            xr = ((W - 1) >> o) - r                     # the last x with (x + r) << o <= W - 1
            for x in (r, r - 1, xr, xr + 1):
                if x + 1 > w - 1:
                    continue
                kps.append((o, s, h // 2, x))
                alone.append(rf.frame(depth, cam_matrix(K_PLAIN), o, s, h // 2, x, 3) is not None)
    c = _bcase("b_frame_border_unreachable", levels, H, W, octaves, kps, depth=depth)
    assert any(alone) and not all(alone) and (c["want"]["bins"] == -1).all() and not c["want"]["ok"].any()
    c["premise"].update(frame_alone_keeps=int(sum(alone)), frame_alone_drops=int(len(alone) - sum(alone)))
    return c


@functools.lru_cache(maxsize=None)
def describe_cases():
    a = _frames("b_frames", K_PLAIN)
    b = _frames("b_frames_negative_fx", (-300.0, 310.0, 60.5, 47.25))
    assert a["premise"]["flip_taken"] == [True] and b["premise"]["flip_taken"] == [False]
    return [_window_border(), _sample_rule(), _flat(), _two_peaks(), _full_range(), _normalisation(), a, b,
            _frame_border_unreachable()]


def smooth_frame(H, W, seed, n):
    """Blobs of many sizes on mid grey, as tests/test_features_gpu.py's _smooth: keypoints in every octave."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    f = np.full((H, W, 3), 120.0)
    for _ in range(n):
        cy, cx, sg = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.2, 7.0)
        f += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))[..., None] * rng.uniform(-100, 100, 3)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def full_size_frame():
    """The product size: a 480 x 640 frame of 120 blobs on a tilted plane with holes -> inputs and the restatement's trace."""
    H, W = 480, 640
    img = smooth_frame(H, W, 5, 120)
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (0.6 + 0.0002 * xx + 0.0001 * yy).astype(f32)
    depth[rng.random((H, W)) < 0.01] = 0.0
    mask = rng.random((H, W)) >= 0.01
    K = [[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]]
    tr = {}
    kps, bins, desc, frames, ok = rf.featurize(img, depth, mask, K, trace=tr)
    premise = dict(keypoints=len(kps), ok=int(ok.sum()), blocks=detect_blocks(H, W, 3), octaves_hit=sorted(set(kps[:, 0].tolist())))
    assert len(kps) >= 40 and ok.sum() >= 10 and premise["blocks"] == 3150 and premise["octaves_hit"] == [0, 1, 2]
    return dict(name="full_size", img=img, depth=depth, mask=mask, K=K, pyramid=tr["pyramid"],
                want=dict(kps=kps, bins=bins, desc=desc, frames=frames, ok=ok), premise=premise)


# ---- match --------------------------------------------------------------------------------------------------------------
def _mcase(name, A, ok, B, cap=None, count=None, **premise):
    """A i8 [n,128] scene rows, B i8 [Nm,128]; the rows behind n (up to cap) hold random descriptors with ok = 1."""
    n = len(A)
    cap = n if cap is None else cap
    rng = np.random.default_rng(n * 7 + len(B))
    rows = rng.integers(0, 128, (cap, 128)).astype(np.uint8)
    oks = np.ones(cap, dtype=np.uint8)
    rows[:n], oks[:n] = A.astype(np.uint8), np.asarray(ok).astype(np.uint8)
    best, d2, w = rf.match_matrix(A, ok, B)
    want = np.stack([best, d2, w], 1).astype(np.int32)
    assert 0 <= A.min() and A.max() <= 127 and 0 <= B.min() and B.max() <= 127
    premise = dict(premise, n=n, cap=cap, Nm=len(B), matched=int((best >= 0).sum()), weighted=int((w > 0).sum()))
    return dict(name=name, A=rows, ok=oks, n=n, cap=cap, count=np.array([n, 0] if count is None else count, dtype=np.int32),
                B=np.ascontiguousarray(B.astype(np.uint8)), want=want, premise=premise)


def _near_copies(rng, B, rows, n):
    """n scene rows: the first len(rows) are near-copies of the model rows `rows`, the rest random."""
    A = rng.integers(0, 128, (n, 128)).astype(np.int64)
    k = min(len(rows), n)
    A[:k] = np.clip(B[rows[:k]].astype(np.int64) + rng.integers(-3, 4, (k, 128)), 0, 127)
    return A.astype(np.int8)


def _delta(d2):
    """A difference vector of 128 entries in 0..127 whose squares sum to d2 exactly (greedy)."""
    v, k = np.zeros(128, dtype=np.int64), 0
    while d2 > 0:
        e = min(127, int(np.floor(np.sqrt(d2))))
        v[k], d2, k = e, d2 - e * e, k + 1
    return v


@functools.lru_cache(maxsize=None)
def match_cases():
    out = []
    rng = np.random.default_rng(70)
    B129 = rng.integers(0, 128, (129, 128)).astype(np.int8)
    # scene counts across the 32-column waves and the 128-row tiles
    for n in (1, 32, 33, 64, 65, 127, 128, 129, 257, 4096):
        A = _near_copies(rng, B129, rng.integers(0, 129, n // 2), n)
        ok = rng.random(n) < 0.8
        ok[0] = True
        prem = {}
        if n >= 64:
            ok[32:64] = False
            prem["wave_off"] = (32, 64)
        if n >= 257:
            ok[128:256] = False
            prem["tile_off"] = (128, 256)
        if n == 4096:
            ok[3 * S_TILE:4 * S_TILE], ok[-1] = False, True
        for cap in ((n, 4096) if n < 4096 else (n,)):
            c = _mcase("m_scene%d_cap%d" % (n, cap) if n < 4096 else "m_scene4096", A, ok, B129, cap=cap, **prem)
            assert n == 1 or 0 < c["premise"]["matched"] < n
            for a, b in prem.values():                  # a whole wave / a whole tile of dropped rows: (-1, 0, 0) each
                assert (c["want"][a:b] == np.array([-1, 0, 0])).all() and b - a in (32, S_TILE)
            out.append(c)
    A = _near_copies(rng, B129, rng.integers(0, 129, 20), 40)
    c = _mcase("m_over_cap", A, np.ones(40, bool), B129, cap=40, count=[41, 1])
    c["want"] = c["want"][:0]
    out.append(c)
    # model counts across the staged tiles and the chunks
    for Nm in (127, 128, 129, 2047, 2048, 2049, 4097, 65536):
        n = 33 if Nm == 65536 else 129
        B = rng.integers(0, 128, (Nm, 128)).astype(np.int8)
        last_tile, last_chunk = (Nm - 1) // MT_ROWS * MT_ROWS, (Nm - 1) // M_CHUNK * M_CHUNK
        take = np.concatenate([[Nm - 1, last_tile, last_chunk, max(0, last_tile - 1), max(0, last_chunk - 1), 0],
                               rng.integers(0, Nm, n // 2 - 6)])
        A = _near_copies(rng, B, take, n)
        c = _mcase("m_model%d" % Nm, A, rng.random(n) < 0.9, B, last_tile=last_tile, last_chunk=last_chunk)
        best = c["want"][:, 0]
        c["premise"]["best_in_last_tile"] = int((best >= last_tile).sum())
        c["premise"]["best_is_last_row"] = int((best == Nm - 1).sum())
        hit = c["want"][:len(take), 0][c["ok"][:len(take)] != 0]
        assert np.array_equal(hit, take[c["ok"][:len(take)] != 0]) and (best >= last_chunk).any()
        out.append(c)
    # ties at d2 = 1 between distinct model rows; decoys of d2 = 2 at lower indices. Across the lane halves (the merge of
    # the two keys decides): the lower row in lane half 1 and the higher in half 0 (4, 8), across a 32-row tile (31, 32),
    # a staged tile (127, 128) and a chunk (2047, 2048). In one lane (row & 4 equal: the strict < of the running minimum
    # decides): neighbouring registers (9, 10), two 32-row tiles (16, 48), two staged tiles (70, 198), (300, 1324)
    across = ((4, 8), (31, 32), (127, 128), (2047, 2048)), ((0, 3), (20, 21), (100, 101), (1000, 2000))
    one_lane = ((9, 10), (16, 48), (70, 198), (300, 1324)), ((0, 3), (11, 12), (60, 61), (250, 251))
    assert all((lo & 4) == (hi & 4) and hi // M_CHUNK == lo // M_CHUNK for lo, hi in one_lane[0])
    assert all((lo & 4) != (hi & 4) or hi // M_CHUNK != lo // M_CHUNK for lo, hi in across[0])
    for name, d_lo, d_hi, (pairs, decoys) in (("m_ties_both", 1, 1, across), ("m_ties_higher_only", 2, 1, across),
                                              ("m_ties_lower_only", 1, 2, across), ("m_ties_one_lane", 1, 1, one_lane),
                                              ("m_ties_one_lane_higher_only", 2, 1, one_lane)):
        B = rng.integers(0, 128, (2100, 128)).astype(np.int64)
        A = rng.integers(1, 126, (len(pairs), 128)).astype(np.int64)
        for q, ((lo, hi), dec) in enumerate(zip(pairs, decoys)):
            for row, d, at in ((lo, d_lo, 3), (hi, d_hi, 70)) + tuple((j, 2, 11 + 5 * k) for k, j in enumerate(dec)):
                B[row] = A[q]
                B[row, at:at + d] += 1                  # + 1 in d coordinates (other coordinates for every row): d2 = d
        c = _mcase(name, A.astype(np.int8), np.ones(len(pairs), bool), B.astype(np.int8), pairs=pairs)
        want_j = [lo if d_lo <= d_hi else hi for lo, hi in pairs]
        assert c["want"][:, 0].tolist() == want_j and (c["want"][:, 1] == 1).all() and (c["want"][:, 2] == 1024).all()
        d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(2)
        assert all(sorted(d2[q].tolist())[:4] == ([1, 1, 2, 2] if d_lo == d_hi else [1, 2, 2, 2]) for q in range(len(pairs)))
        out.append(c)
    # weights at the steps of 1024 - (d2 >> 6)
    targets, ws = (0, 63, 64, 65535, 65536), (1024, 1024, 1023, 1, 0)
    B = rng.integers(0, 128, (300, 128)).astype(np.int64)
    A = rng.integers(0, 128, (len(targets), 128)).astype(np.int64)
    A[:, :8] = 0
    rows = (5, 40, 131, 200, 299)
    for q, (t, row) in enumerate(zip(targets, rows)):
        B[row] = A[q] + _delta(t)
    c = _mcase("m_weights", A.astype(np.int8), np.ones(len(targets), bool), B.astype(np.int8), d2=targets)
    assert c["want"].tolist() == [[r, t, w] for r, t, w in zip(rows, targets, ws)]
    out.append(c)
    c = _mcase("m_weight_farthest", np.zeros((1, 128), np.int8), np.ones(1, bool), np.full((3, 128), 127, np.int8))
    assert c["want"].tolist() == [[0, 128 * 127 * 127, 0]]
    out.append(c)
    return out


# ---- hypotheses ---------------------------------------------------------------------------------------------------------
def random_rigid(rng, n, scale=1.0):
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3], T[:, :3, 3] = Q, rng.normal(size=(n, 3)) * scale
    return T


def hypotheses_want(match, Fs, Fm):
    """rf.candidate_poses on the rows 11.7 takes (0 <= j < Nm and w > 0); the rest are rejected: zero pose, zero peak."""
    j, w = match[:, 0].astype(np.int64), match[:, 2].astype(np.int64)
    take = (j >= 0) & (j < len(Fm)) & (w > 0)
    cand = rf.candidate_poses(Fs, Fm, np.where(take, j, 0), np.where(take, w, 0))
    peaks = np.zeros((len(match), 3), dtype=np.int32)
    peaks[take, 0], peaks[take, 2] = j[take], w[take]
    return cand, peaks, take


def _hcase(name, n, Nm, seed, Fs=None, Fm=None, count=None, **premise):
    rng = np.random.default_rng(seed)
    cap = n + 3
    Fs = random_rigid(rng, cap, 0.5) if Fs is None else Fs
    Fm = random_rigid(rng, Nm, 0.1) if Fm is None else Fm
    special = [(-1, 5), (Nm, 7), (Nm - 1, 1), (0, 0), (Nm // 2, 1024), (1, -3), (Nm + 1000, 1024), (0, 1)]
    match = np.zeros((cap, 3), dtype=np.int32)
    match[:, 0] = rng.integers(0, Nm, cap)
    match[:, 1] = rng.integers(0, 70000, cap)
    match[:, 2] = rng.integers(1, 1025, cap)
    for k, i in enumerate(list(range(0, n, 5)) + [n - 1]):                 # spread over the list, the last row among them
        match[i, 0], match[i, 2] = special[k % len(special)] if n > 1 else special[2]
    cand, peaks, take = hypotheses_want(match[:n], Fs[:n], Fm)
    premise = dict(premise, n=n, cap=cap, Nm=Nm, taken=int(take.sum()), rejected=int(n - take.sum()))
    return dict(name=name, match=match, Fs=Fs, Fm=Fm, n=n, cap=cap, Nm=Nm, want=dict(cand=cand, peaks=peaks),
                count=np.array([n, 0] if count is None else count, dtype=np.int32), premise=premise)


def _other_order(A, M):
    """F_s . F_m^-1 with each three-term sum taken as a0 b0 + (a1 b1 + a2 b2): 11.6 writes (a0 b0 + a1 b1) + a2 b2."""
    R, t = M[:3, :3], M[:3, 3]
    B = np.eye(4)
    B[:3, :3] = R.T
    for j in range(3):
        B[j, 3] = -(R[0, j] * t[0] + (R[1, j] * t[1] + R[2, j] * t[2]))
    out = np.eye(4)
    for a in range(3):
        for b in range(3):
            out[a, b] = A[a, 0] * B[0, b] + (A[a, 1] * B[1, b] + A[a, 2] * B[2, b])
        out[a, 3] = (A[a, 0] * B[0, 3] + (A[a, 1] * B[1, 3] + A[a, 2] * B[2, 3])) + A[a, 3]
    return out


@functools.lru_cache(maxsize=None)
def hypotheses_cases():
    out = []
    for n in (1, 255, 256, 257):
        c = _hcase("h_n%d" % n, n, 40, n)
        assert c["premise"]["taken"] >= 1 and (n == 1 or c["premise"]["rejected"] >= 4)
        if n > 1:
            m = c["match"][:n]
            assert {-1, 40, 39}.issubset(set(m[:, 0].tolist())) and {0, 1, 1024}.issubset(set(m[:, 2].tolist()))
        out.append(c)
    # entries from 1e-6 to 1e3 in both frames: the order of the sums and a fused multiply-add show in the bits
    rng = np.random.default_rng(77)
    n, Nm = 64, 16

    def wide(k):
        F = np.tile(np.eye(4), (k, 1, 1))
        F[:, :3, :] = rng.choice([-1.0, 1.0], (k, 3, 4)) * 10.0 ** rng.uniform(-6, 3, (k, 3, 4))
        return F
    c = _hcase("h_magnitudes", n, Nm, 78, Fs=wide(n + 3), Fm=wide(Nm))
    m, moved = c["match"], 0
    for i in range(n):
        if c["want"]["peaks"][i, 2] > 0:
            moved += int((_other_order(c["Fs"][i], c["Fm"][m[i, 0]]).view(np.int64) != c["want"]["cand"][i].view(np.int64)).any())
    c["premise"].update(rows_another_order_changes=moved, smallest=float(np.abs(c["Fs"][:, :3]).min()),
                        largest=float(np.abs(c["Fs"][:, :3]).max()))
    assert moved >= c["premise"]["taken"] // 2 > 0
    out.append(c)
    c = _hcase("h_over_cap", 30, 40, 5, count=[34, 1])
    out.append(c)
    return out


STAGE_BUILDERS = dict(detect=detect_cases, describe=describe_cases, match=match_cases, hypotheses=hypotheses_cases)
