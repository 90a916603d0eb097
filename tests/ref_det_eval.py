"""numpy restatement of SPEC.md section 10 (detection mAP), written from the SPEC text. Two forms of the status rule:
`status_claim_winner` (10.5 as stated: order-free) and `status_sequential` (the loop 10.5 is equivalent to: the detections of
a class one by one in rank order, marking ground truths as taken). Everything else -- IoU, claim, rank, curves, both APs --
is shared. f32 where the SPEC says f32, one operation per numpy call so that nothing is contracted."""
import numpy as np

F = np.float32
REC_THR = np.array([F(float(j) * 0.1) for j in range(11)], dtype=F)      # 10.1: t_j = f32((double) j * 0.1)
ST_FP, ST_TP, ST_IGNORED, ST_DUP = 0, 1, 2, 3


def iou(d, g):
    """10.2 for boxes f32 [...,4] against f32 [...,4] (broadcast)."""
    d, g = np.asarray(d, F), np.asarray(g, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.maximum(np.minimum(d[..., 2], g[..., 2]) - np.maximum(d[..., 0], g[..., 0]), F(0))
        h = np.maximum(np.minimum(d[..., 3], g[..., 3]) - np.maximum(d[..., 1], g[..., 1]), F(0))
        inter = w * h
        a = (d[..., 2] - d[..., 0]) * (d[..., 3] - d[..., 1])
        b = (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])
        return (inter / ((a + b) - inter)).astype(F)


def claim(det_box, det_cls, det_image, gt_box, gt_cls, gt_offset):
    """10.3 -> best_gt int32 [N], best_iou f32 [N]; vectorised over the detections, one step per ground-truth slot."""
    N = len(det_cls)
    best, biou = np.full(N, -1, np.int32), np.zeros(N, F)
    if N == 0 or len(gt_cls) == 0:
        return best, biou
    g0, g1 = gt_offset[det_image], gt_offset[det_image + 1]
    for j in range(int((g1 - g0).max())):
        g = g0 + j
        live = g < g1
        gs = np.where(live, g, 0)
        v = iou(det_box, gt_box[gs])
        take = live & (gt_cls[gs] == det_cls) & ~np.isnan(v) & ((best < 0) | (v > biou))
        best[take], biou[take] = g[take], v[take]
    return best, biou


def sort_key(score, cls):
    """10.4: ascending key = class, then score descending (-0 = +0); a stable sort keeps the input order among equals."""
    b = np.asarray(score, F).view(np.uint32).astype(np.uint64)
    b = np.where(b == 0x80000000, 0, b)
    m = np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000)
    return ((np.asarray(cls).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - m)).astype(np.int64)


def rank_order(score, cls, C):
    order = np.argsort(sort_key(score, cls), kind="stable").astype(np.int32)
    class_offset = np.concatenate([[0], np.cumsum(np.bincount(cls, minlength=C))]).astype(np.int32)
    return order, class_offset


def status_claim_winner(best, biou, order, difficult, thr):
    """10.5 -> u8 [N] by input index."""
    N = len(best)
    st = np.zeros(N, np.uint8)
    b = best[order]                                          # rank order
    hit = (b >= 0) & (biou[order] > F(thr))
    ign = hit & (difficult[np.where(b >= 0, b, 0)] != 0) if len(difficult) else np.zeros(N, bool)
    cl = hit & ~ign
    ranks = np.nonzero(cl)[0]
    _u, first = np.unique(b[ranks], return_index=True)         # the lowest rank of every claimed ground truth
    s = np.zeros(N, np.uint8)
    s[cl] = ST_DUP
    s[ranks[first]] = ST_TP
    s[ign] = ST_IGNORED
    st[order] = s
    return st


def status_sequential(det_box, det_cls, det_image, gt_box, gt_cls, gt_offset, difficult, order, thr):
    """The loop of the reference's algorithm (detections of a class in rank order, ground truths marked once detected), with
    10.3's NaN and tie rules."""
    N = len(det_cls)
    st = np.zeros(N, np.uint8)
    taken = np.zeros(len(gt_cls), bool)
    for n in order:
        cand = [g for g in range(gt_offset[det_image[n]], gt_offset[det_image[n] + 1]) if gt_cls[g] == det_cls[n]]
        bg, bv = -1, F(0)
        for g in cand:
            v = iou(det_box[n], gt_box[g])
            if not np.isnan(v) and (bg < 0 or v > bv):
                bg, bv = g, v
        if bg < 0 or not bv > F(thr):
            st[n] = ST_FP
        elif difficult[bg]:
            st[n] = ST_IGNORED
        elif not taken[bg]:
            st[n], taken[bg] = ST_TP, True
        else:
            st[n] = ST_DUP
    return st


def evaluate(det_box, det_score, det_cls, det_image, gt_box, gt_cls, gt_offset, difficult, C, iou_thr=(0.5,), sequential=False):
    """Everything 10.9 lists. Curves are in rank order, [T,N]."""
    det_box, gt_box = np.asarray(det_box, F).reshape(-1, 4), np.asarray(gt_box, F).reshape(-1, 4)
    det_score, det_cls, det_image = np.asarray(det_score, F), np.asarray(det_cls, np.int64), np.asarray(det_image, np.int64)
    gt_cls, gt_offset = np.asarray(gt_cls, np.int64), np.asarray(gt_offset, np.int64)
    difficult = np.zeros(len(gt_cls), np.uint8) if difficult is None else np.asarray(difficult, np.uint8)
    N, T = len(det_cls), len(iou_thr)
    best, biou = claim(det_box, det_cls, det_image, gt_box, gt_cls, gt_offset)
    order, class_offset = rank_order(det_score, det_cls, C)
    n_easy = np.bincount(gt_cls[difficult == 0], minlength=C).astype(np.int32)
    out = {"best_gt": best, "best_iou": biou, "order": order, "class_offset": class_offset, "n_easy": n_easy,
           "status": np.zeros((T, N), np.uint8), "ctp": np.zeros((T, N), np.int32), "cfp": np.zeros((T, N), np.int32),
           "prec": np.zeros((T, N), F), "rec": np.zeros((T, N), F), "env": np.zeros((T, N), F), "p11": np.zeros((T, C, 11), F),
           "ap11": np.zeros((T, C), F), "apa": np.zeros((T, C), np.float64), "map11": np.zeros(T, F), "mapa": np.zeros(T, np.float64)}
    for k, thr in enumerate(iou_thr):
        if sequential:
            st = status_sequential(det_box, det_cls, det_image, gt_box, gt_cls, gt_offset, difficult, order, thr)
        else:
            st = status_claim_winner(best, biou, order, difficult, thr)
        out["status"][k] = st
        sr = st[order]
        for c in range(C):
            a, b = class_offset[c], class_offset[c + 1]
            if a == b:
                continue
            ctp = np.cumsum(sr[a:b] == ST_TP, dtype=np.int32)
            cfp = np.cumsum((sr[a:b] == ST_FP) | (sr[a:b] == ST_DUP), dtype=np.int32)
            ft, ff = ctp.astype(F), cfp.astype(F)
            with np.errstate(invalid="ignore", divide="ignore"):
                prec = ft / ((ft + ff) + F(1e-10))
                rec = ft / F(n_easy[c])
            env = np.maximum.accumulate(prec[::-1])[::-1]
            out["ctp"][k, a:b], out["cfp"][k, a:b], out["prec"][k, a:b], out["rec"][k, a:b], out["env"][k, a:b] = ctp, cfp, prec, rec, env
            for j in range(11):
                m = rec >= REC_THR[j]
                out["p11"][k, c, j] = prec[m].max() if m.any() else F(0)
            if n_easy[c] > 0:
                out["apa"][k, c] = float(np.sum(env[sr[a:b] == ST_TP].astype(np.float64))) / float(n_easy[c])
        for c in range(C):
            s = out["p11"][k, c, 0]
            for j in range(1, 11):
                s = F(s + out["p11"][k, c, j])
            out["ap11"][k, c] = F(s / F(11.0))
        s = F(0)
        for c in range(C):
            s = F(s + out["ap11"][k, c])
        out["map11"][k] = F(s / F(C))
        out["mapa"][k] = float(np.sum(out["apa"][k])) / float(C)
    return out
