#!/usr/bin/env python
"""Detection AP on the device (DESIGN.md "Detection AP on the device"): what the metric costs next to the inference step it follows.
One JSON line on stdout and in --out.

  match  : B = 20, K = 64, about 10 GT per image, T = 10 (COCO's thresholds), C in {3, 80}: the match launch alone (ops.det_match)
           and the whole ``DetectionAP.update`` (launch + the device-side appends to the pools), median microseconds.
  compute: ``DetectionAP.compute()`` after 250 such updates (5 000 images, 320 000 slots): the AP launch alone (device events) and the
           whole call (sorts, launch, the one copy; host clock around a synchronised call), for each C and for the 101-point and the
           area mode.

Device events around each call after warm-up, enqueued behind a spin kernel so that they bracket device time only; the host time
of a call is reported next to it.  The inputs are seeded copies of tests/det_ap_ref.py's random batches at these
sizes (detections = shifted copies of GT plus clutter).  Nothing here has a pass mark.

    python tools/det_ap_bench.py [--reps 200] [--out profiles/det_ap_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import det_ap_ref as ref  # noqa: E402
from squeezedet_pytorch_amd import _native as nat, metrics, ops  # noqa: E402

B, K, T = 20, 64, 10


def median_us(fn, reps, warm=20, spin_us=600):
    """Device time of ``fn``'s launches: (median, p10, p90) microseconds between two events that are enqueued while the device is still
    busy with a spin kernel, so the host time of the Python wrapper is not in the figure; and the host time per call (wall clock
    over ``reps`` un-synchronised calls)."""
    lib, stream = nat.lib(), nat.stream_handle()
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        nat.check(lib.sqd_spin_us(spin_us, stream), 'sqd_spin_us')
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    host = (time.perf_counter() - t0) * 1e6 / reps
    torch.cuda.synchronize()
    return {'device_us': float(np.median(ts)), 'p10': float(np.percentile(ts, 10)), 'p90': float(np.percentile(ts, 90)), 'host_us': host}


def batch_on_device(seed, C):
    rs = np.random.RandomState(seed)
    count, cls, sc, bx, gb, gc, go, gi = ref.random_batch(seed, B, K, C, rs.randint(6, 15, B), True, canvas=300.0)
    det = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (count, cls, sc, bx))
    return det, tuple(torch.from_numpy(a).cuda() for a in (gb, gc, go)), torch.from_numpy(gi).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--updates', type=int, default=250)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    out = {'B': B, 'K': K, 'T': T, 'reps': args.reps, 'images': args.updates * B, 'slots': args.updates * B * K, 'rows': []}
    for C in (3, 80):
        batches = [batch_on_device(100 + i, C) for i in range(8)]
        thr = ops.det_thresholds(metrics.COCO_THRESHOLDS, 'cuda')
        npos = torch.zeros(C, device='cuda', dtype=torch.int32)
        det, gt, ign = batches[0]
        row = {'C': C, 'gt_per_image': float(np.mean([float(g[2][-1]) / B for _, g, _ in batches]))}
        row['match_us'] = median_us(lambda: ops.det_match(det, *gt, thr, C, gt_ignore=ign, npos=npos), args.reps)
        for mode in ('101point', 'area'):
            met = metrics.DetectionAP(C, metrics.COCO_THRESHOLDS, mode)
            if mode == '101point':
                met.update(det, *gt, gt_ignore=ign)
                met._reserve(det[2].device, (2 * args.reps + 40) * B * K)          # (time the steady state, not a pool growth)
                row['update_us'] = median_us(lambda: met.update(det, *gt, gt_ignore=ign), args.reps)
                met.reset()
            for i in range(args.updates):
                d, g, ig = batches[i % len(batches)]
                met.update(d, *g, gt_ignore=ig)
            torch.cuda.synchronize()
            timer = ops.KernelTimer()
            ops.set_timer(timer)
            walls = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = met.compute()
                walls.append((time.perf_counter() - t0) * 1e6)
            torch.cuda.synchronize()
            ops.set_timer(None)
            launches = [r[4].elapsed_time(r[5]) * 1000.0 for r in timer.records if r[0] == 'det_ap']
            row[f'compute_{mode}_us'] = float(np.median(walls[2:]))
            row[f'ap_launch_{mode}_us'] = float(np.median(launches[2:]))
            row[f'map_all_{mode}'] = float(res['map_all'])
        out['rows'].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
