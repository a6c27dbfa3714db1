#!/usr/bin/env python
"""Box voting ("Box voting"): what the voting step costs inside the fused launch, against the same launch without
it and against the composition one would write by hand.  One JSON line on stdout and in --out.  Per shape four calls alternate in one
process on the same ``pred`` (same clocks, same caches):

  vote        : ``ops.detect_nms`` / ``ops.detect_views`` with ``vote_iou`` = 0.5 -- the voting select kernel, as ``Detector`` calls it;
  vote_counts : the same with ``return_votes=True`` -- the call also makes the zeroed int32 [B, K] tensor the kernel writes |V_i| to;
  plain       : the same call with ``vote_iou=None`` -- today's launch, the floor;
  composition : ``ops.decode`` of every row (the dense class / score / box tensors are written and read again; pooled: plus the fp32
                mapping in torch and the reshape that is the ``cat`` of an image's views), ``torch.topk`` of the thresholded scores for the
                K candidates, their pairwise IoU [B, K, K], the same-class / IoU >= vote_iou mask, the masked score-weighted mean in
                float64, then ``ops.filter_dense_nms`` on the dense tensors and a gather of the voted boxes of its rows.

Shapes: B = 20 images of 1248 x 384 (A = 16 848), 3 classes, K = 64, hard class-wise and Gaussian; the worst case for the walk -- K =
1024, one class, class-agnostic, score_thresh 0.05: 1024 candidates in one group, every emitted row walks 1024 ranks -- hard and Gaussian
(Gaussian emits the most rows); pooled V = 2 views of 10 images.  Inputs as tools/views_bench.py: KITTI anchors, seeded normal logits and
deltas, the confidence raised around twelve centres per row.  The composition's sums run in another order (a float64 matmul), so it is
compared with the launch within 1e-3 px on the rows both emit, not bit for bit.  Device events around each call after warm-up, medians
in microseconds; result buffers and workspaces are allocated once, outside the timed calls.

    python tools/box_vote_bench.py [--reps 200] [--out profiles/box_vote_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import ops  # noqa: E402

SIZE = (384, 1248)
NMS, VOTE = 0.4, 0.5

SHAPES = [
    dict(name='B20_K64_hard', B=20, V=1, C=3, K=64, thr=0.3, mode='hard', agnostic=False),
    dict(name='B20_K64_gaussian', B=20, V=1, C=3, K=64, thr=0.3, mode='gaussian', agnostic=False),
    dict(name='worst_K1024_one_class_agnostic_hard', B=20, V=1, C=1, K=1024, thr=0.05, mode='hard', agnostic=True),
    dict(name='worst_K1024_one_class_agnostic_gaussian', B=20, V=1, C=1, K=1024, thr=0.05, mode='gaussian', agnostic=True),
    dict(name='pooled_V2_B10_K64_hard', B=10, V=2, C=3, K=64, thr=0.3, mode='hard', agnostic=False),
]


def make_inputs(R, V, C, seed):
    cfg = sqd.make_cfg(num_classes=C, device='cpu')
    anc = cfg.anchors.astype(np.float32)
    A = anc.shape[0]
    rs = np.random.RandomState(seed)
    pred = np.empty((R, A, C + 5), np.float32)
    pred[..., :C] = rs.standard_normal((R, A, C)) * 2.0
    conf = rs.standard_normal((R, A)) * 1.0 - 2.0
    for r in range(R):
        for _ in range(12):
            cx, cy, rad = rs.uniform(0, SIZE[1]), rs.uniform(0, SIZE[0]), rs.uniform(20, 60)
            conf[r] += 4.0 * np.exp(-((anc[:, 0] - cx) ** 2 + (anc[:, 1] - cy) ** 2) / (2 * rad * rad))
    pred[..., C] = conf
    pred[..., C + 1:] = rs.standard_normal((R, A, 4)) * 0.3
    xf = np.zeros((R, 6), np.float32)
    for r in range(R):
        xf[r] = (1.0, 1.0, 0.0, 0.0, (r % V) % 2, SIZE[1] - 1)                     # (V = 2: the image and its mirror image)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(anc).cuda(), torch.from_numpy(xf).cuda(), A


def time_alternating(calls, reps, warmup=20):
    """{name: median microseconds} of the calls, alternating name by name."""
    for f in calls.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in calls}
    for r in range(reps):
        for k, f in calls.items():
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: float(np.median([a.elapsed_time(b) * 1e3 for a, b in v])) for k, v in ev.items()}


def hand_vote(ids, sc, bx, K, thr, vote_iou):
    """Voted box and voter count of each of the top-K candidates of dense [B, N] tensors -> (anchor [B, K], voted [B, K, 4] fp32,
    votes [B, K]); slots past the candidates have anchor -1."""
    s = torch.where(sc > thr, sc, torch.zeros_like(sc))
    top, at = torch.topk(s, min(K, s.shape[1]), dim=1)
    ok = top > 0
    b = torch.gather(bx, 1, at[..., None].expand(-1, -1, 4))
    c = torch.gather(ids, 1, at)
    area = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    iw = (torch.minimum(b[:, :, None, 2], b[:, None, :, 2]) - torch.maximum(b[:, :, None, 0], b[:, None, :, 0])).clamp_min(0)
    ih = (torch.minimum(b[:, :, None, 3], b[:, None, :, 3]) - torch.maximum(b[:, :, None, 1], b[:, None, :, 1])).clamp_min(0)
    inter = iw * ih
    u = inter / ((area[:, :, None] + area[:, None, :]) - inter)
    eye = torch.eye(u.shape[1], dtype=torch.bool, device=u.device)
    m = ((u >= vote_iou) | eye) & (c[:, :, None] == c[:, None, :]) & ok[:, None, :]
    w = m.double() * top.double()[:, None, :]
    voted = (torch.bmm(w, b.double()) / w.sum(2, keepdim=True).clamp_min(1e-300)).float()
    return torch.where(ok, at, torch.full_like(at, -1)), voted, m.sum(2).int()


def leg(shape, reps):
    dev = torch.device('cuda')
    B, V, C, K, thr, mode, agnostic = (shape[k] for k in ('B', 'V', 'C', 'K', 'thr', 'mode', 'agnostic'))
    R = B * V
    pred, anchors, xf, A = make_inputs(R, V, C, seed=len(shape['name']))
    kw = dict(nms_mode=mode, nms_agnostic=agnostic)
    ws = lambda rows, a: torch.empty(ops.det_workspace_words_wide(rows, a, K), device=dev, dtype=torch.int32)  # noqa: E731
    out_v, out_p, out_c = (ops._det_buffers(B, K, dev) + (ws(R, A),), ops._det_buffers(B, K, dev) + (ws(R, A),),
                           ops._det_buffers(B, K, dev) + (ws(B, V * A),))
    sy, sx, dy, dx, flip, mirror = (xf[:, i].reshape(-1, 1) for i in range(6))
    flipped = flip != 0
    if V == 1:
        def fused(out, **extra):
            return ops.detect_nms(pred, anchors, SIZE, C, K, NMS, thr, out=out, **kw, **extra)
    else:
        def fused(out, **extra):
            return ops.detect_views(pred, anchors, SIZE, C, V, xf, K, NMS, thr, out=out, **kw, **extra)

    def composition():
        ids, sc, bx = ops.decode(pred, anchors, SIZE, C)
        if V > 1:
            x1, y1 = bx[..., 0] / sx + dx, bx[..., 1] / sy + dy
            x2, y2 = bx[..., 2] / sx + dx, bx[..., 3] / sy + dy
            bx = torch.stack([torch.where(flipped, mirror - x2, x1), y1, torch.where(flipped, mirror - x1, x2), y2], -1)
            ids, sc, bx = ids.reshape(B, V * A), sc.reshape(B, V * A), bx.reshape(B, V * A, 4)
        at, voted, votes = hand_vote(ids, sc, bx, K, thr, VOTE)
        cnt, cls, s, box, idx = ops.filter_dense_nms(ids, sc, bx, C, K, NMS, thr, out=out_c, **kw)
        hit = (idx[:, :, None] == at[:, None, :])                                  # [B, K rows, K candidates]: a row's candidate slot
        slot = hit.int().argmax(2)
        return cnt, cls, s, torch.gather(voted, 1, slot[..., None].expand(-1, -1, 4)), idx, torch.gather(votes, 1, slot)

    calls = {'vote': lambda: fused(out_v, vote_iou=VOTE), 'vote_counts': lambda: fused(out_v, vote_iou=VOTE, return_votes=True),
             'plain': lambda: fused(out_p), 'composition': composition}
    got, plain, comp = calls['vote_counts'](), calls['plain'](), calls['composition']()
    torch.cuda.synchronize()
    counts = got[0].tolist()
    if sum(counts) == 0 or not torch.equal(got[0], plain[0]) or not torch.equal(got[0], comp[0]):
        raise SystemExit(f'box_vote_bench {shape["name"]}: the three calls disagree on the counts (or nothing was detected)')
    rows = torch.arange(K, device=dev)[None, :] < got[0][:, None]
    if not torch.equal(got[4][rows], plain[4][rows]) or not torch.equal(got[4][rows], comp[4][rows]):
        raise SystemExit(f'box_vote_bench {shape["name"]}: the three calls disagree on the emitted anchors')
    diff = (got[3][rows] - comp[3][rows]).abs().max(1).values
    close = float((diff <= 1e-3).float().mean())
    if close < 0.99:                                                               # (torch.topk may break a score tie at the K-th slot otherwise)
        raise SystemExit(f'box_vote_bench {shape["name"]}: only {close:.3f} of the voted rows agree with the hand composition')
    us = time_alternating(calls, reps)
    votes = got[5][rows].float()
    return dict(shape, A=A, us=us, emitted_per_image=float(got[0].float().mean()), mean_voters=float(votes.mean()), max_voters=int(votes.max()),
                rows_moved=float((got[3][rows] != plain[3][rows]).any(1).float().mean()), rows_within_1e_3_px_of_composition=close,
                vote_minus_plain_us=us['vote'] - us['plain'], vote_over_plain=us['vote'] / us['plain'],
                vote_over_composition=us['vote'] / us['composition'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'box_vote_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('box_vote_bench: needs a GPU')
    res = {'input_size': list(SIZE), 'nms_thresh': NMS, 'vote_iou': VOTE, 'reps': args.reps, 'unit': 'us per call (median, device events)',
           'legs': {s['name']: leg(s, args.reps) for s in SHAPES}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
