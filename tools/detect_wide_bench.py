#!/usr/bin/env python
"""Fused detect, narrow against wide ("Wide fused detect"), one JSON line on stdout and in --out:

  narrow : ``ops.detect`` (detect_kernel, one launch) at the benchmarked parameters B = 20, A = 16 848, K = 64;
  wide   : ``ops.detect_wide`` (two launches) on the same inputs, the two alternating in one process -- what generality costs;
  grid   : ``ops.detect_wide`` at B = 20 for K in {64, 256, 1024} x A in {16 848, 32 400, 73 440}.

Device events around each call after warm-up, medians in microseconds.  Inputs: seeded normal logits (the sweep tests' 'normal'
distribution), default thresholds; result buffers and workspaces are allocated once, outside the timed calls.

    python tools/detect_wide_bench.py [--reps 200] [--out profiles/detect_wide_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squeezedet_pytorch_amd import ops  # noqa: E402

SIZE = (384, 1248)
B, C = 20, 3


def make_inputs(A, seed=0):
    rs = np.random.RandomState(seed)
    pred = np.empty((B, A, C + 5), np.float32)
    pred[..., :C + 1] = rs.standard_normal((B, A, C + 1)) * 1.5
    pred[..., C + 1:] = rs.standard_normal((B, A, 4)) * 0.3
    anchors = np.stack([rs.uniform(0, SIZE[1], A), rs.uniform(0, SIZE[0], A), rs.uniform(1, 120, A), rs.uniform(1, 120, A)], 1)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(anchors.astype(np.float32)).cuda()


def time_alternating(calls, reps, warmup=20):
    """{name: median microseconds} of the calls, alternating name by name (same clocks, same caches)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'detect_wide_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('detect_wide_bench: needs a GPU')
    dev = torch.device('cuda')
    res = {'batch': B, 'num_classes': C, 'reps': args.reps, 'nms_thresh': 0.4, 'score_thresh': 0.3, 'unit': 'us (median, device events)'}

    A = 16848
    pred, anchors = make_inputs(A)
    nb = ops._det_buffers(B, 64, dev, A)                                # the narrow workspace (eight scoring workgroups per image)
    wb = ops._det_buffers(B, 64, dev) + (torch.empty(ops.det_workspace_words_wide(B, A, 64), device=dev, dtype=torch.int32),)
    n = ops.detect(pred, anchors, SIZE, C, 64, 0.4, 0.3, out=nb)
    w = ops.detect_wide(pred, anchors, SIZE, C, 64, 0.4, 0.3, out=wb)
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(n, w))
    if not same:
        raise SystemExit('detect_wide_bench: wide and narrow results differ')
    us = time_alternating({'narrow': lambda: ops.detect(pred, anchors, SIZE, C, 64, 0.4, 0.3, out=nb),
                           'wide': lambda: ops.detect_wide(pred, anchors, SIZE, C, 64, 0.4, 0.3, out=wb)}, args.reps)
    res['A16848_K64'] = {'narrow_us': us['narrow'], 'wide_us': us['wide'], 'wide_over_narrow': us['wide'] / us['narrow'],
                         'kept_per_image': float(n[0].float().mean())}

    grid = {}
    for A in (16848, 32400, 73440):
        pred, anchors = make_inputs(A, seed=A)
        for K in (64, 256, 1024):
            bufs = ops._det_buffers(B, K, dev) + (torch.empty(ops.det_workspace_words_wide(B, A, K), device=dev, dtype=torch.int32),)
            f = lambda: ops.detect_wide(pred, anchors, SIZE, C, K, 0.4, 0.3, out=bufs)   # noqa: E731
            us = time_alternating({'wide': f}, args.reps)
            grid[f'A{A}_K{K}'] = {'wide_us': us['wide'], 'kept_per_image': float(bufs[0].float().mean())}
    res['wide_grid'] = grid
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
