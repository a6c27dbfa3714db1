"""Plain numpy float64 restatement of the detection-AP rules (DESIGN.md "Detection AP on the device"): the yardstick of
tests/test_det_ap_host.py and tests/test_det_ap_gpu.py.  No third-party evaluator is involved: this file is the definition.

Python loops throughout; sums run in plain index order.  ``iou`` is the scalar definition; ``iou_matrix`` applies the same
operations in the same order elementwise (test_det_ap_host checks that the two agree bit for bit) and only saves time.

``match`` takes keyword switches that BREAK one rule each (``strict``, ``claim_ignored``, ``rematch_claimed``, ``tie_high``): the host
tier uses them to show that the hand cases notice each of those mistakes."""
import numpy as np


def iou(a, b):
    """float64 IoU of two xyxy boxes given as fp32 coordinates, no "+1" convention."""
    ax1, ay1, ax2, ay2 = (np.float64(np.float32(v)) for v in a)
    bx1, by1, bx2, by2 = (np.float64(np.float32(v)) for v in b)
    area_a = (ax2 - ax1) * (ay2 - ay1)
    area_b = (bx2 - bx1) * (by2 - by1)
    iw = max(np.float64(0.0), min(ax2, bx2) - max(ax1, bx1))
    ih = max(np.float64(0.0), min(ay2, by2) - max(ay1, by1))
    inter = iw * ih
    union = (area_a + area_b) - inter
    return inter / union if union > 0 else np.float64(0.0)


def iou_matrix(A, G):
    """[n,4] x [m,4] fp32 -> float64 [n,m], the operations of ``iou`` in the same order."""
    A = np.asarray(A, np.float32).astype(np.float64).reshape(-1, 4)
    G = np.asarray(G, np.float32).astype(np.float64).reshape(-1, 4)
    area_a = ((A[:, 2] - A[:, 0]) * (A[:, 3] - A[:, 1]))[:, None]
    area_b = ((G[:, 2] - G[:, 0]) * (G[:, 3] - G[:, 1]))[None, :]
    iw = np.maximum(0.0, np.minimum(A[:, None, 2], G[None, :, 2]) - np.maximum(A[:, None, 0], G[None, :, 0]))
    ih = np.maximum(0.0, np.minimum(A[:, None, 3], G[None, :, 3]) - np.maximum(A[:, None, 1], G[None, :, 1]))
    inter = iw * ih
    union = (area_a + area_b) - inter
    out = np.zeros_like(inter)
    np.divide(inter, union, out=out, where=union > 0)
    return out


def _best(v, tie_high):
    """Highest entry of ``v`` (IoU per candidate, -1 = not available; equal IoU: lowest position; ``tie_high``: the broken rule)
    -> (iou, position) or None."""
    if v.size == 0 or v.max() < 0:
        return None
    j = v.size - 1 - int(np.argmax(v[::-1])) if tie_high else int(np.argmax(v))       # argmax: the first maximum
    return v[j], j


def match(count, cls, sc, bx, gt_boxes, gt_cls, gt_off, thresholds, C, gt_ignore=None,
          strict=False, claim_ignored=False, rematch_claimed=False, tie_high=False):
    """-> (flags uint8 [B,K,T], matched_gt int32 [B,K,T], npos int64 [C])."""
    count, cls, sc = np.asarray(count), np.asarray(cls), np.asarray(sc, np.float32)
    B, K = sc.shape
    T = len(thresholds)
    gt_cls = np.asarray(gt_cls).reshape(-1)
    ign = np.zeros(gt_cls.shape[0], bool) if gt_ignore is None else np.asarray(gt_ignore).reshape(-1) != 0
    flags = np.full((B, K, T), 3, np.uint8)
    matched = np.full((B, K, T), -1, np.int32)
    npos = np.zeros(C, np.int64)
    for g in range(gt_cls.shape[0]):
        if not ign[g] and 0 <= gt_cls[g] < C:
            npos[gt_cls[g]] += 1
    for b in range(B):
        n = min(max(int(count[b]), 0), K)
        g0, g1 = int(gt_off[b]), int(gt_off[b + 1])
        M = iou_matrix(np.asarray(bx)[b, :n], np.asarray(gt_boxes).reshape(-1, 4)[g0:g1])
        for k in range(n):
            if not 0 <= cls[b, k] < C:
                flags[b, k, :] = 0
        for c in range(C):
            dets = sorted([k for k in range(n) if cls[b, k] == c], key=lambda k: (-float(sc[b, k]), k))
            if not dets:
                continue
            real = np.asarray([g - g0 for g in range(g0, g1) if gt_cls[g] == c and not ign[g]], np.int64)
            ignored = np.asarray([g - g0 for g in range(g0, g1) if gt_cls[g] == c and ign[g]], np.int64)
            for t, thr in enumerate(thresholds):
                claimed = np.zeros(real.size, bool)
                claimed_ign = np.zeros(ignored.size, bool)
                for k in dets:
                    v = M[k][real]
                    hit = _best(v if rematch_claimed else np.where(claimed, -1.0, v), tie_high)
                    if hit is not None and (hit[0] > thr if strict else hit[0] >= thr):
                        flags[b, k, t], matched[b, k, t] = 1, g0 + real[hit[1]]
                        claimed[hit[1]] = True
                        continue
                    hit = _best(np.where(claimed_ign, -1.0, M[k][ignored]), tie_high)
                    if hit is not None and (hit[0] > thr if strict else hit[0] >= thr):
                        flags[b, k, t], matched[b, k, t] = 2, g0 + ignored[hit[1]]
                        claimed_ign[hit[1]] = claim_ignored
                    else:
                        flags[b, k, t], matched[b, k, t] = 0, -1
    return flags, matched, npos


def order(cls, score):
    """Indices that order a pool by (class ascending, score descending, insertion order ascending)."""
    cls, score = np.asarray(cls), np.asarray(score, np.float32)
    return np.asarray(sorted(range(cls.shape[0]), key=lambda i: (int(cls[i]), -float(score[i]), i)), dtype=np.int64)


def segments(cls_sorted, C):
    cls_sorted = np.asarray(cls_sorted)
    seg = np.zeros(C + 1, np.int32)
    for c in range(C + 1):
        seg[c] = int(np.sum(cls_sorted < c))
    return seg


def ap(cls_sorted, flags_sorted, seg, npos, mode):
    """mode 0 / 1 / 2 -> (ap float64 [C,T], tp_cum, fp_cum int32 [N,T] (zero outside the segments), prec float64 [C,T,101]: the
    sampled precisions of modes 1 (first 11) and 2, else zeros)."""
    flags_sorted = np.asarray(flags_sorted)
    N, T = flags_sorted.shape
    C = len(npos)
    out = np.full((C, T), np.nan, np.float64)
    tp_cum = np.zeros((N, T), np.int32)
    fp_cum = np.zeros((N, T), np.int32)
    samples = np.zeros((C, T, 101), np.float64)
    for c in range(C):
        s0, s1 = int(seg[c]), int(seg[c + 1])
        for t in range(T):
            tp = fp = 0
            prec = []
            for i in range(s0, s1):
                ok = cls_sorted[i] == c
                tp += 1 if ok and flags_sorted[i, t] == 1 else 0
                fp += 1 if ok and flags_sorted[i, t] == 0 else 0
                tp_cum[i, t], fp_cum[i, t] = tp, fp
                prec.append(np.float64(tp) / np.float64(tp + fp) if tp + fp > 0 else np.float64(0.0))
            if npos[c] <= 0:
                continue
            env = list(prec)
            run = np.float64(0.0)
            for j in range(len(env) - 1, -1, -1):
                run = max(run, env[j])
                env[j] = run
            if mode == 0:
                s = np.float64(0.0)
                for j, i in enumerate(range(s0, s1)):
                    if cls_sorted[i] == c and flags_sorted[i, t] == 1:
                        s += env[j]
                out[c, t] = s / np.float64(npos[c])
            else:
                S = 10 if mode == 1 else 100
                s = np.float64(0.0)
                j = 0                                          # recall never falls: the first position reaching r only moves on
                for k in range(S + 1):
                    r = np.float64(k) / np.float64(S)
                    while j < s1 - s0 and not np.float64(tp_cum[s0 + j, t]) / np.float64(npos[c]) >= r:
                        j += 1
                    p = env[j] if j < s1 - s0 else np.float64(0.0)
                    samples[c, t, k] = p
                    s += p
                out[c, t] = s / np.float64(S + 1)
    return out, tp_cum, fp_cum, samples


MODES = {'area': 0, '11point': 1, '101point': 2}


def dataset(batches, thresholds, C, mode, **broken):
    """The whole metric for a list of batches ``(count, cls, sc, bx, gt_boxes, gt_cls, gt_off, gt_ignore)`` (numpy):
    -> {'ap' [C,T], 'map' [T], 'map_all', 'npos' [C]} with the means as plain index-order sums over the classes with GT."""
    pc, ps, pf = [], [], []
    npos = np.zeros(C, np.int64)
    for count, cls, sc, bx, gb, gc, go, gi in batches:
        f, _, n = match(count, cls, sc, bx, gb, gc, go, thresholds, C, gi, **broken)
        npos += n
        cls = np.asarray(cls)
        pc.append(np.where((f[..., 0] == 3) | (cls < 0) | (cls >= C), C, cls).reshape(-1))
        ps.append(np.asarray(sc, np.float32).reshape(-1))
        pf.append(f.reshape(-1, len(thresholds)))
    pc, ps, pf = np.concatenate(pc), np.concatenate(ps), np.concatenate(pf)
    o = order(pc, ps)
    a, _, _, _ = ap(pc[o], pf[o], segments(pc[o], C), npos, MODES.get(mode, mode))
    with_gt = [c for c in range(C) if npos[c] > 0]
    m = np.zeros(len(thresholds), np.float64)
    for t in range(len(thresholds)):
        s = 0.0
        for c in with_gt:
            s += float(a[c, t])
        m[t] = s / len(with_gt) if with_gt else np.nan
    s = 0.0
    for v in m:
        s += float(v)
    return {'ap': a, 'map': m, 'map_all': s / len(m), 'npos': npos}


# ---------------------------------------------------------------------------------------------------------------------
def hand_batch():
    """B=3, K=8, C=2, thresholds (0.5, 0.75), worked out by hand.  Image 0: a detection whose IoU is exactly 0.5 ([0,0,2,1] against
    [0,0,2,2]); a duplicate of one GT where the HIGHER-scored copy sits in the later slot; an ignored GT hit twice; two identical GT
    taken by two detections of equal score (lower slot first, lower GT index first); slot 7 past ``count`` holds garbage.  Image 1:
    GT but ``count == 0`` (all slots garbage).  Image 2: detections, no GT.
    -> (batch tuple as ``dataset`` takes it, thresholds, C, expected flags [3,8,2], expected matched_gt [3,8,2], expected npos [2])."""
    thr = (0.5, 0.75)
    gt_boxes = np.array([[0, 0, 2, 2], [10, 10, 20, 20], [30, 30, 40, 40], [50, 0, 54, 4], [50, 0, 54, 4],
                         [0, 0, 10, 10], [20, 20, 30, 30]], np.float32)
    gt_cls = np.array([0, 0, 1, 0, 0, 0, 1], np.int32)
    gt_ign = np.array([0, 0, 1, 0, 0, 0, 0], np.uint8)
    gt_off = np.array([0, 5, 7, 7], np.int32)
    count = np.array([7, 0, 3], np.int32)
    cls = np.zeros((3, 8), np.int64)
    sc = np.zeros((3, 8), np.float32)
    bx = np.zeros((3, 8, 4), np.float32)
    img0 = [(0, 0.9, [0, 0, 2, 1]), (0, 0.7, [10, 10, 20, 20]), (0, 0.8, [10, 10, 20, 20]), (1, 0.95, [30, 30, 40, 40]),
            (1, 0.6, [30, 30, 40, 38]), (0, 0.5, [50, 0, 54, 4]), (0, 0.5, [50, 0, 54, 4]), (1, 0.99, [0, 0, 2, 2])]
    for k, (c, s, box) in enumerate(img0):
        cls[0, k], sc[0, k], bx[0, k] = c, s, box
    cls[1, :], sc[1, :], bx[1, :] = 0, 0.9, [0, 0, 10, 10]                  # garbage behind count == 0
    img2 = [(0, 0.4, [0, 0, 5, 5]), (1, 0.3, [1, 1, 2, 2]), (0, 0.2, [3, 3, 9, 9])]
    for k, (c, s, box) in enumerate(img2):
        cls[2, k], sc[2, k], bx[2, k] = c, s, box
    cls[2, 3:], sc[2, 3:], bx[2, 3:] = 7, 1.5, [0, 0, 1, 1]
    flags = np.full((3, 8, 2), 3, np.uint8)
    matched = np.full((3, 8, 2), -1, np.int32)
    flags[0, :7] = [[1, 0], [0, 0], [1, 1], [2, 2], [2, 2], [1, 1], [1, 1]]
    matched[0, :7] = [[0, -1], [-1, -1], [1, 1], [2, 2], [2, 2], [3, 3], [4, 4]]
    flags[2, :3] = 0
    npos = np.array([5, 1], np.int64)
    return (count, cls, sc, bx, gt_boxes, gt_cls, gt_off, gt_ign), thr, 2, flags, matched, npos


def random_batch(seed, B, K, C, gt_counts, with_ignore, canvas=24.0):
    """Seeded batch with ties: box coordinates on a quarter-pixel lattice, scores on a 1/64 lattice, some GT duplicated exactly
    (equal IoU for any detection), detections = jittered copies of GT of their class plus clutter, slots past ``count`` garbage.
    ``gt_counts``: GT per image.  -> batch tuple as ``dataset`` takes it."""
    rs = np.random.RandomState(seed)

    def boxes(n):
        x1 = rs.randint(0, int(canvas * 4), n) / 4.0
        y1 = rs.randint(0, int(canvas * 4), n) / 4.0
        w = rs.randint(4, 40, n) / 4.0
        h = rs.randint(4, 40, n) / 4.0
        return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.float32)

    gb, gc, off = [], [], [0]
    for b in range(B):
        n = int(gt_counts[b])
        bb, cc = boxes(n), rs.randint(0, C, n).astype(np.int32)
        for i in range(1, n):                                  # exact duplicates (same class): IoU ties
            if rs.rand() < 0.25:
                j = rs.randint(0, i)
                bb[i], cc[i] = bb[j], cc[j]
        gb.append(bb); gc.append(cc); off.append(off[-1] + n)
    gt_boxes = np.concatenate(gb, 0) if gb else np.zeros((0, 4), np.float32)
    gt_cls = np.concatenate(gc, 0)
    gt_off = np.asarray(off, np.int32)
    gt_ign = (rs.rand(gt_cls.shape[0]) < 0.3).astype(np.uint8) if with_ignore else None
    count = rs.randint(0, K + 1, B).astype(np.int32)
    count[0] = K                                               # one full image
    cls = rs.randint(0, C, (B, K)).astype(np.int64)
    sc = (rs.randint(1, 65, (B, K)) / 64.0).astype(np.float32)
    bx = np.stack([boxes(K) for _ in range(B)], 0)
    for b in range(B):
        n = int(gt_counts[b])
        for k in range(K):
            if n and rs.rand() < 0.7:                          # a (possibly shifted) copy of a GT, usually of its class
                g = off[b] + rs.randint(0, n)
                shift = rs.randint(-2, 3, 4) / 4.0 if rs.rand() < 0.6 else np.zeros(4)
                cand = gt_boxes[g] + shift.astype(np.float32)
                if cand[2] > cand[0] and cand[3] > cand[1]:
                    bx[b, k] = cand
                if rs.rand() < 0.9:
                    cls[b, k] = gt_cls[g]
    return count, cls, sc, bx, gt_boxes, gt_cls, gt_off, gt_ign


def count_ties(batch, C):
    """(score ties, IoU ties) present in a batch: pairs of live detections of one image and class with equal scores; live detections
    whose highest IoU over the GT of their class is positive and reached by two GT."""
    count, cls, sc, bx, gb, gc, go, _ = batch
    s_ties = i_ties = 0
    for b in range(sc.shape[0]):
        n = int(count[b])
        seen = set()
        for k in range(n):
            key = (int(cls[b, k]), float(sc[b, k]))
            s_ties += key in seen
            seen.add(key)
        g0, g1 = int(go[b]), int(go[b + 1])
        if g1 > g0 and n:
            M = iou_matrix(bx[b, :n], gb[g0:g1])
            for k in range(n):
                v = M[k][gc[g0:g1] == cls[b, k]]
                i_ties += v.size > 1 and v.max() > 0 and int((v == v.max()).sum()) > 1
    return s_ties, i_ties
