"""Plain-numpy reference of box voting ("Box voting"; csrc/detect_wide.hip ``detn_vote``).  No torch.

``vote``: for one image, the candidates in rank order (``nms_ref.candidates``: the top K of the anchors with score > score_thresh, score
descending, ties by lower anchor index), and for every emitted anchor i -- the device's own ``anchor_idx`` rows, or a reference's -- the
voters V_i = { r eligible (class in 0 .. C-1) : class_r == class_i and (r == i or u(i, r) >= vote_iou) } with u = ``nms_ref.iou32`` (the
scan's fp32 expression; a NaN u compares false), then W = sum s_r and X_k = sum s_r * b_r[k] over V_i in ascending rank as Python floats
(float64; a product of two fp32 values is exact there) and the voted coordinate float32(X_k / W).  The weights are the original scores.
The result does not depend on the suppression rule or on the order of the ``anchor_idx`` rows: each row is computed on its own."""
import numpy as np

import nms_ref

F = np.float32


def vote(class_ids, scores, boxes, K, score_thresh, num_classes, anchor_idx, vote_iou, return_voters=False):
    """-> (boxes fp32 [n, 4], votes int32 [n]) for the n rows of ``anchor_idx``; with ``return_voters`` also the list of each row's
    voters as indices into the (pooled) anchors, ascending in rank."""
    class_ids = np.asarray(class_ids).reshape(-1)
    scores = np.asarray(scores, F).reshape(-1)
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    anchor_idx = np.asarray(anchor_idx).reshape(-1).astype(np.int64)
    order = nms_ref.candidates(scores, K, score_thresh)
    c, s, b = class_ids[order], scores[order], boxes[order]
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])).astype(F)
    eligible = (c >= 0) & (c < num_classes)
    rank_of = {int(a): r for r, a in enumerate(order)}
    thr = F(vote_iou)
    out = np.empty((len(anchor_idx), 4), F)
    votes = np.empty(len(anchor_idx), np.int32)
    voters = []
    for row, a in enumerate(anchor_idx):
        i = rank_of[int(a)]
        assert eligible[i], f'row {row}: anchor {int(a)} is not an eligible candidate'
        u = nms_ref.iou32(b[i], area[i], b, area)
        with np.errstate(invalid='ignore'):
            m = eligible & (c == c[i]) & (u >= thr)
        m[i] = True
        ranks = np.nonzero(m)[0]
        W, X = 0.0, [0.0, 0.0, 0.0, 0.0]
        for r in ranks:                                          # ascending rank, float64
            sr = float(s[r])
            W += sr
            for k in range(4):
                X[k] += sr * float(b[r, k])
        out[row] = [F(X[k] / W) for k in range(4)]
        votes[row] = len(ranks)
        voters.append(order[ranks])
    return (out, votes, voters) if return_voters else (out, votes)
