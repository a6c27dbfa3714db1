#!/usr/bin/env python
"""Cost of the ignore regions at KITTI size ("Ignore regions and object-free images"), one JSON line on stdout
and in --out.  B = 20, A = 16 848 (24 x 78 x 9), ~40 positives per image:

  for C in {3, 80} and 0 / 8 / 300 ignore boxes per image: the masked loss forward (mean form) and backward against the unmasked
  sparse launches on the same operands, alternating in one process; and ``ops.anchor_ignore_mask`` on its own.  The masked launches
  read A / 8 bytes of bitmap per image more than the sparse ones.

Device events around each call after warm-up, enqueued behind a spin kernel so that they bracket device time only.  Nothing here
has a pass mark.

    python tools/ignore_regions_bench.py [--reps 100] [--out profiles/ignore_regions_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import _native as nat, ops  # noqa: E402
from many_class_bench import B, SIZE, WEIGHTS, make_inputs  # noqa: E402


def time_alternating(calls, reps, warmup=10, spin_us=600):
    """{name: median microseconds} of the calls, alternating name by name; every bracket is enqueued while the device still idles in
    a spin kernel, so the host time of the Python wrapper is not in the figure."""
    lib, stream = nat.lib(), nat.stream_handle()
    for f in calls.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            nat.check(lib.sqd_spin_us(spin_us, stream), 'sqd_spin_us')
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: float(np.median(v)) for k, v in ts.items()}


def ignore_boxes(n, seed):
    """n boxes per image, 40 .. 300 pixels wide and 30 .. 150 high, anywhere in the input -> (boxes [B n, 4], offsets [B+1])."""
    rs = np.random.RandomState(seed)
    w, h = rs.uniform(40, 300, (B, n)), rs.uniform(30, 150, (B, n))
    x, y = rs.uniform(0, SIZE[1] - 1 - w), rs.uniform(0, SIZE[0] - 1 - h)
    bx = np.stack([x, y, x + w, y + h], -1).astype(np.float32).reshape(-1, 4)
    return torch.from_numpy(bx).cuda(), torch.arange(B + 1, dtype=torch.int32, device='cuda') * n


def case(C, n, A, anchors, anchors64, reps):
    pred, gt = make_inputs(A, C, anchors, seed=C)
    sgt = ops.sparse_gt_from_dense(gt)
    total = int(sgt.anchor_idx.shape[0])
    gmean = torch.ones(1, device='cuda')
    boxes, offs = ignore_boxes(n, 100 + n)
    bitmap = ops.anchor_ignore_mask(boxes, offs, anchors64, 0.5)
    _, nobj, _ = ops.loss_sparse_mean_fwd(pred, sgt, anchors, SIZE, C, WEIGHTS)
    _, counts, _ = ops.loss_masked_mean_fwd(pred, sgt, bitmap, anchors, SIZE, C, WEIGHTS)
    us = time_alternating({'loss_sparse_fwd': lambda: ops.loss_sparse_mean_fwd(pred, sgt, anchors, SIZE, C, WEIGHTS),
                           'loss_masked_fwd': lambda: ops.loss_masked_mean_fwd(pred, sgt, bitmap, anchors, SIZE, C, WEIGHTS),
                           'loss_sparse_bwd': lambda: ops.loss_sparse_mean_bwd(pred, sgt, anchors, nobj, gmean, SIZE, C, WEIGHTS),
                           'loss_masked_bwd': lambda: ops.loss_masked_mean_bwd(pred, sgt, bitmap, anchors, counts, gmean, SIZE, C, WEIGHTS),
                           'anchor_ignore_mask': lambda: ops.anchor_ignore_mask(boxes, offs, anchors64, 0.5, out=bitmap)}, reps)
    ignored = float((counts[1] - (A - counts[0])).abs().mean())
    out = {'positives': total, 'ignore_boxes_per_image': n, 'ignored_anchors_per_image': ignored, 'bitmap_bytes_per_image': 4 * ops.ignore_words(A)}
    out.update({k + '_us': v for k, v in us.items()})
    return out


def as_called(cfg, anchors, anchors64, reps, warmup=30):
    """Host time of one eager ``Loss.mean_loss(pred, gt)`` + ``.backward()`` as a training step calls it (C = 3, sparse gt, without
    and with an ignore bitmap): wall clock around the two calls, the device drained before each, so the figure is the Python
    wrappers, the autograd node and the launches' enqueue, not device time; ``*_ops``: the same two launches through the
    ``ops.loss_*_mean_fwd`` / ``_bwd`` wrappers alone.  -> {name: {median_us, p10_us, p90_us}}."""
    import time
    from squeezedet_pytorch_amd.model import Loss
    C, A = 3, cfg.num_anchors
    loss_mod = Loss(cfg)
    pred, gt = make_inputs(A, C, anchors, seed=C)
    pred.requires_grad_(True)
    sgt = ops.sparse_gt_from_dense(gt)
    bitmap = ops.anchor_ignore_mask(*ignore_boxes(8, 108), anchors64, 0.5)
    def module_step(ignore):
        pred.grad = None
        mean, _ = loss_mod.mean_loss(pred, sgt, ignore)
        mean.backward()

    # the same two launches through the ops wrappers alone (no autograd node, no engine thread)
    p, gmean = pred.detach(), torch.ones(1, device='cuda')

    def sparse_ops():
        _, nobj, _ = ops.loss_sparse_mean_fwd(p, sgt, anchors, SIZE, C, WEIGHTS)
        ops.loss_sparse_mean_bwd(p, sgt, anchors, nobj, gmean, SIZE, C, WEIGHTS)

    def masked_ops():
        _, counts, _ = ops.loss_masked_mean_fwd(p, sgt, bitmap, anchors, SIZE, C, WEIGHTS)
        ops.loss_masked_mean_bwd(p, sgt, bitmap, anchors, counts, gmean, SIZE, C, WEIGHTS)

    out = {}
    for name, step in (('sparse', lambda: module_step(None)), ('masked', lambda: module_step(bitmap)),
                       ('sparse_ops', sparse_ops), ('masked_ops', masked_ops)):
        ts = []
        for i in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            ts.append((time.perf_counter() - t0) * 1e6)
        ts = np.asarray(ts[warmup:])
        out[name] = {'median_us': float(np.median(ts)), 'p10_us': float(np.percentile(ts, 10)), 'p90_us': float(np.percentile(ts, 90))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ignore_regions_bench.json'))
    ap.add_argument('--as-called', action='store_true', help='only the host time of Loss.mean_loss + backward as called (reps calls)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('ignore_regions_bench: needs a GPU')
    cfg = sqd.make_cfg(input_size=SIZE)
    anchors = torch.from_numpy(cfg.anchors).float().cuda()
    anchors64 = torch.from_numpy(np.asarray(cfg.anchors, np.float64)).cuda()
    A = cfg.num_anchors
    if args.as_called:
        line = json.dumps({'batch': B, 'anchors': A, 'reps': args.reps, 'unit': 'us (host wall clock per forward + backward)',
                           'as_called': as_called(cfg, anchors, anchors64, args.reps)})
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')
        print(line)
        return
    res = {'batch': B, 'anchors': A, 'reps': args.reps, 'overlap': 0.5, 'unit': 'us (median, device events behind a spin kernel)'}
    for C in (3, 80):
        res[f'C{C}'] = {f'boxes{n}': case(C, n, A, anchors, anchors64, args.reps) for n in (0, 8, 300)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
