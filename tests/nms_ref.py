"""Plain-numpy reference of the NMS modes ("NMS modes"; csrc/detect_wide.hip ``detect_nms_select_kernel``).

``soft_filter``: the rule for one image in fp32, op for op -- the candidates (top K of the anchors with score > score_thresh, score
descending, ties by lower anchor index), the groups (classes 0 .. C-1, or one group with ``agnostic``), and within a group: pick the
largest current score (tie: lower rank), stop when it is not above the threshold, emit, then update every remaining candidate with
u = inter / ((area_i + area_j) - inter): 'hard' drops it if u > nms_thresh, 'linear' multiplies its score by (1 - u) if u > nms_thresh,
'gaussian' multiplies every score by exp(-(u * u) / sigma) -- the weight being float64 ``exp`` of the fp32 argument, rounded to fp32.

``verify_replay``: the check for a device result in Gaussian mode, where the device's ``expf`` and numpy's ``exp`` may differ in the
last bit and two current scores within that distance may legitimately be picked in either order.  It replays the DEVICE's emitted
order with the scores in float64 (the IoU and the exponent's argument in fp32, exactly as the device forms them -- IEEE fp32
arithmetic is deterministic, only ``expf`` and the rounding of the product are not pinned) and checks the rule at every step.
The tolerance of a score that has received n decays is ``tol_n = (n + 1) * 3 * 2^-24``: per decay, 1 ulp (2^-23) for ``expf`` -- the
bound the HIP math API documentation gives for it; that document is not part of every ROCm installation, the figure is taken as
published -- plus half an ulp (2^-24) for the rounding of the product."""
import numpy as np

F = np.float32
MODES = ('hard', 'linear', 'gaussian')


def tol(n):
    return (np.asarray(n, np.float64) + 1.0) * 3.0 * 2.0 ** -24


def candidates(scores, K, score_thresh):
    """Anchor indices of the candidates in rank order."""
    scores = np.asarray(scores, F).reshape(-1)
    cand = np.nonzero(scores > F(score_thresh))[0]
    return cand[np.argsort(-scores[cand], kind='stable')][:int(K)]


def _groups(c, num_classes, agnostic):
    valid = (c >= 0) & (c < num_classes)
    if agnostic:
        return [np.nonzero(valid)[0]]
    return [np.nonzero(c == k)[0] for k in range(num_classes)]


def iou32(box, area, boxes, areas):
    """u of one box against many, fp32 op for op (the expression of detect_kernel)."""
    with np.errstate(divide='ignore', invalid='ignore'):
        w = np.maximum(F(0), np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0]))
        h = np.maximum(F(0), np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1]))
        inter = (w * h).astype(F)
        return (inter / ((area + areas) - inter)).astype(F)


def gauss_arg(u, sigma):
    """the fp32 argument of the Gaussian weight's exp"""
    with np.errstate(invalid='ignore'):
        return (-(u * u) / F(sigma)).astype(F)


def soft_filter(class_ids, scores, boxes, K, nms_thresh, score_thresh, num_classes, mode, sigma=0.5, agnostic=False):
    """-> dict(class_ids int64 [n], scores fp32 [n], boxes fp32 [n,4], anchor_idx int64 [n], decays int [n] (decays each emitted row
    received), total_decays (score updates in the image), lost (candidates of a group that were never emitted: suppressed in 'hard',
    decayed to the threshold or below in the soft modes)); n may be 0."""
    assert mode in MODES
    class_ids = np.asarray(class_ids).reshape(-1)
    scores = np.asarray(scores, F).reshape(-1)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    thr, nt = F(score_thresh), F(nms_thresh)
    order = candidates(scores, K, score_thresh)
    c, s0, b = class_ids[order], scores[order], boxes[order]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F)
    out, total, lost = [], 0, 0
    for m in _groups(c, num_classes, agnostic):
        cur = s0[m].copy()
        alive = np.ones(len(m), bool)
        ndec = np.zeros(len(m), np.int64)
        while alive.any():
            masked = np.where(alive & ~np.isnan(cur), cur, F(-np.inf))
            j = int(np.argmax(masked))                      # first maximum = lowest rank
            if not masked[j] > thr:
                break
            out.append((m[j], cur[j], ndec[j]))
            alive[j] = False
            rest = np.nonzero(alive)[0]
            if rest.size == 0:
                break
            u = iou32(b[m[j]], area[m[j]], b[m[rest]], area[m[rest]])
            if mode == 'gaussian':
                w = np.exp(gauss_arg(u, sigma).astype(np.float64)).astype(F)
                cur[rest] = (cur[rest] * w).astype(F)
                ndec[rest] += 1
                total += rest.size
            else:
                hit = rest[u > nt]
                if mode == 'hard':
                    alive[hit] = False
                    lost += hit.size
                else:
                    cur[hit] = (cur[hit] * (F(1) - u[u > nt])).astype(F)
                    ndec[hit] += 1
                    total += hit.size
        if mode != 'hard':
            lost += int(alive.sum())
    sel = np.array([o[0] for o in out], np.int64)
    return {'class_ids': c[sel].astype(np.int64), 'scores': np.array([o[1] for o in out], F), 'boxes': b[sel].reshape(-1, 4),
            'anchor_idx': order[sel].astype(np.int64), 'decays': np.array([o[2] for o in out], np.int64),
            'total_decays': total, 'lost': lost}


def verify_replay(rows, class_ids, scores, boxes, K, nms_thresh, score_thresh, num_classes, mode, sigma=0.5, agnostic=False):
    """``rows``: one image's emitted rows -- dict(class_ids [n], scores [n], boxes [n,4], anchor_idx [n]) in output order.
    AssertionError naming the first violated condition; returns the number of rows checked."""
    assert mode in MODES
    class_ids = np.asarray(class_ids).reshape(-1)
    scores = np.asarray(scores, F).reshape(-1)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    r_cls = np.asarray(rows['class_ids']).reshape(-1)
    r_sc = np.asarray(rows['scores'], F).reshape(-1)
    r_bx = np.asarray(rows['boxes'], F).reshape(-1, 4)
    r_idx = np.asarray(rows['anchor_idx']).reshape(-1).astype(np.int64)
    n = len(r_idx)
    assert len(r_cls) == n and len(r_sc) == n and len(r_bx) == n, 'row arrays of different lengths'
    thr, nt = float(F(score_thresh)), F(nms_thresh)
    order = candidates(scores, K, score_thresh)
    c, b = class_ids[order], boxes[order]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F)
    rank_of = {int(a): r for r, a in enumerate(order)}
    # classes, boxes and anchor indices are exact
    for i in range(n):
        a = int(r_idx[i])
        assert a in rank_of, f'row {i}: anchor {a} is not a candidate'
        assert int(r_cls[i]) == int(class_ids[a]), f'row {i}: class {int(r_cls[i])} != {int(class_ids[a])} of anchor {a}'
        assert np.array_equal(r_bx[i], boxes[a]), f'row {i}: box differs from anchor {a}\'s'
    pos = 0
    for gi, m in enumerate(_groups(c, num_classes, agnostic)):
        cur = scores[order][m].astype(np.float64)
        ndec = np.zeros(len(m), np.int64)
        alive = np.ones(len(m), bool)
        member = {int(r): j for j, r in enumerate(m)}
        while pos < n and (agnostic or int(r_cls[pos]) == gi):
            r = rank_of[int(r_idx[pos])]
            assert r in member, f'row {pos}: anchor {int(r_idx[pos])} is not a candidate of group {gi}'
            j = member[r]
            assert alive[j], f'row {pos}: anchor {int(r_idx[pos])} was emitted or dropped before'
            t = float(tol(ndec[j]))
            live = alive & ~np.isnan(cur)
            best = float(cur[live].max())
            assert cur[j] >= best * (1.0 - t), (f'row {pos}: current score {cur[j]!r} is not the largest remaining ({best!r}) '
                                                 f'within {t:.3g}')
            assert cur[j] > thr * (1.0 - t), f'row {pos}: current score {cur[j]!r} is not above the threshold {thr!r}'
            assert abs(float(r_sc[pos]) - cur[j]) <= t * abs(cur[j]), (f'row {pos}: score {float(r_sc[pos])!r} is not within {t:.3g} of '
                                                                     f'the replayed {cur[j]!r} ({int(ndec[j])} decays)')
            alive[j] = False
            rest = np.nonzero(alive)[0]
            if rest.size:
                u = iou32(b[m[j]], area[m[j]], b[m[rest]], area[m[rest]])
                if mode == 'gaussian':
                    cur[rest] = cur[rest] * np.exp(gauss_arg(u, sigma).astype(np.float64))
                    ndec[rest] += 1
                else:
                    hit = rest[u > nt]
                    if mode == 'hard':
                        alive[hit] = False
                    else:
                        cur[hit] = cur[hit] * (1.0 - u[u > nt].astype(np.float64))
                        ndec[hit] += 1
            pos += 1
        left = np.nonzero(alive & ~np.isnan(cur))[0]
        over = [int(order[m[j]]) for j in left if not cur[j] <= thr * (1.0 + float(tol(ndec[j])))]
        assert not over, f'group {gi}: anchors {over[:4]} are still above the threshold after its last row'
    assert pos == n, f'row {pos}: class {int(r_cls[pos])} is out of the groups\' order'
    return n


def make_case(seed, B, A, C, quant=None, one_class=None, size=(384, 1248)):
    """The generator of the GPU tests: box centres around 6 .. 12 cluster centres (12 px sigma), sides uniform in 40 .. 120 px, scores
    uniform in (0, 1) in fp32 (``quant``: rounded up to multiples of 1 / quant -- many exact ties), class ids uniform
    (``one_class``: all that class).  -> class_ids int64 [B,A], scores fp32 [B,A], boxes fp32 [B,A,4]."""
    rs = np.random.RandomState(seed)
    H, W = size
    cls = np.empty((B, A), np.int64); sc = np.empty((B, A), F); bx = np.empty((B, A, 4), F)
    for bi in range(B):
        nc = rs.randint(6, 13)
        centres = np.stack([rs.uniform(80, W - 80, nc), rs.uniform(80, H - 80, nc)], 1)
        pick = rs.randint(0, nc, A)
        cxy = centres[pick] + rs.normal(0, 12.0, (A, 2))
        wh = rs.uniform(40, 120, (A, 2))
        bx[bi] = np.concatenate([cxy - wh / 2, cxy + wh / 2], 1).astype(F)
        s = rs.uniform(0, 1, A).astype(F)
        s = np.clip(s, F(1e-6), F(1 - 1e-6))
        if quant:
            s = (np.ceil(s * quant) / quant).astype(F)
        sc[bi] = s
        cls[bi] = rs.randint(0, C, A) if one_class is None else one_class
    return cls, sc, bx
