#!/usr/bin/env python
"""Pooled views ("Pooled views"): what the fused pooled detect costs against the hand composition it replaces and
against the unpooled floor.  One JSON line on stdout and in --out.  At B = 10 images x V = 2 and V = 4 views, 1248 x 384 (A = 16 848),
3 classes, K = 64, hard class-wise NMS, three calls alternate in one process on the same ``pred`` (same clocks, same caches):

  views       : ``ops.detect_views`` -- scoring launch on B*V rows + one pooled select launch per image;
  composition : ``ops.decode`` of the B*V rows + the fp32 mapping in torch (divide, add, mirror, where, stack) + the reshape that is
                the ``cat`` of an image's views + ``ops.filter_dense_nms`` on [B, V*A] -- the dense [B*V, A] class / score / box
                tensors and the mapped [B, V*A, 4] boxes are written and read again;
  unpooled    : ``ops.detect_nms`` on the same B*V rows, every row an image of its own -- no pooling, the floor.

Inputs: KITTI anchors, seeded normal logits and deltas, the confidence raised around twelve centres per row (as
tools/nms_modes_bench.py); view transforms of a flip / zoom TTA (scale 1 and 0.75, every second view mirrored).  Device events around
each call after warm-up, medians in microseconds; result buffers and workspaces are allocated once, outside the timed calls.

    python tools/views_bench.py [--reps 200] [--out profiles/views_bench.json]
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
B, C, K = 10, 3, 64
NMS, THR = 0.4, 0.3


def make_inputs(V, seed=0):
    cfg = sqd.make_cfg(num_classes=C, device='cpu')
    anc = cfg.anchors.astype(np.float32)
    A = anc.shape[0]
    rs = np.random.RandomState(seed)
    R = B * V
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
        v = r % V
        z = 1.0 if v < 2 else 0.75
        xf[r] = (z, z, -SIZE[0] * (1 - z) / (2 * z), -SIZE[1] * (1 - z) / (2 * z), v % 2, SIZE[1] - 1)
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


def leg(V, reps):
    dev = torch.device('cuda')
    pred, anchors, xf, A = make_inputs(V, seed=V)
    R = B * V
    out_v = ops._det_buffers(B, K, dev) + (torch.empty(ops.det_workspace_words_wide(R, A, K), device=dev, dtype=torch.int32),)
    out_c = ops._det_buffers(B, K, dev) + (torch.empty(ops.det_workspace_words_wide(B, V * A, K), device=dev, dtype=torch.int32),)
    out_u = ops._det_buffers(R, K, dev) + (torch.empty(ops.det_workspace_words_wide(R, A, K), device=dev, dtype=torch.int32),)
    sy, sx, dy, dx, flip, mirror = (xf[:, i].reshape(-1, 1) for i in range(6))
    flipped = flip != 0

    def composition():
        ids, sc, bx = ops.decode(pred, anchors, SIZE, C)
        x1, y1 = bx[..., 0] / sx + dx, bx[..., 1] / sy + dy
        x2, y2 = bx[..., 2] / sx + dx, bx[..., 3] / sy + dy
        mapped = torch.stack([torch.where(flipped, mirror - x2, x1), y1, torch.where(flipped, mirror - x1, x2), y2], -1)
        return ops.filter_dense_nms(ids.reshape(B, V * A), sc.reshape(B, V * A), mapped.reshape(B, V * A, 4), C, K, NMS, THR, out=out_c)

    calls = {'views': lambda: ops.detect_views(pred, anchors, SIZE, C, V, xf, K, NMS, THR, out=out_v),
             'composition': composition,
             'unpooled': lambda: ops.detect_nms(pred, anchors, SIZE, C, K, NMS, THR, out=out_u)}
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    counts = out_v[0].tolist()
    same = torch.equal(out_v[0], out_c[0]) and all(torch.equal(a[i, :n], b[i, :n]) for a, b in zip(out_v[1:5], out_c[1:5])
                                                   for i, n in enumerate(counts))
    if not same or sum(counts) == 0:
        raise SystemExit('views_bench: the pooled detect disagrees with the composition (or nothing was detected)')
    us = time_alternating(calls, reps)
    return {'V': V, 'A': A, 'rows': R, 'us': us, 'kept_per_image': float(out_v[0].float().mean()),
            'kept_per_row_unpooled': float(out_u[0].float().mean()), 'views_over_composition': us['views'] / us['composition'],
            'views_over_unpooled': us['views'] / us['unpooled']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'views_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('views_bench: needs a GPU')
    res = {'batch': B, 'num_classes': C, 'K': K, 'input_size': list(SIZE), 'nms_thresh': NMS, 'score_thresh': THR, 'reps': args.reps,
           'unit': 'us per call (median, device events)', 'legs': {f'V{V}': leg(V, args.reps) for V in (2, 4)}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
