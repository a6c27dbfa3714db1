#!/usr/bin/env python
"""NMS modes ("NMS modes"): what Soft-NMS and class-agnostic NMS cost over the hard class-wise rule.  One JSON
line on stdout and in --out:

  select : per-call device time at B = 20, A = 16 848 for (K = 64, C = 3) and (K = 1024, C = 20) of the parent's hard wide path
           (``ops.detect_wide`` / ``ops.detect_many``: scoring launch + select launch) and of ``ops.detect_nms`` under every rule,
           all alternating in one process on the same inputs.  Every call shares the scoring launch, so a difference between two
           totals is the difference between their select launches.  At C = 3 the select launch of ``detect_nms`` is also timed alone
           (``keys_ready`` on the workspace the previous call filled: no scoring launch); the scoring launch is the hard rule's total
           minus its select launch, and the parent's select launch its total minus that.
  stream : the ``Detector.stream()`` step of the benchmarked shape (SqueezeDet, 20 x 384 x 1248, two lanes, captured) under
           ('hard'), ('gaussian') and ('hard', agnostic), the three taking turns for three rounds in one process.  The default
           rule launches the kernels it always launched (profiles/nms_modes_device_asm_diff.log: byte-identical), so its step
           against the parent's is a matter of run-to-run noise; bench.py's own line is the comparison.

Inputs of `select`: KITTI anchors, seeded normal logits and deltas, the confidence raised around twelve centres per image so that
the top K cluster as detections do (overlapping candidates: the scan has decays to compute).  Device events around each call after
warm-up, medians in microseconds; buffers and workspaces are allocated once, outside the timed calls.

    python tools/nms_modes_bench.py [--reps 200] [--steps 100] [--out profiles/nms_modes_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import ops, synthetic  # noqa: E402
from squeezedet_pytorch_amd.detector import Detector  # noqa: E402
from squeezedet_pytorch_amd.model import SqueezeDet  # noqa: E402

SIZE = (384, 1248)
B = 20
RULES = [('hard', False), ('linear', False), ('gaussian', False), ('hard', True), ('linear', True), ('gaussian', True)]


def make_inputs(C, seed=0):
    cfg = sqd.make_cfg(num_classes=C, device='cpu')
    anc = cfg.anchors.astype(np.float32)
    A = anc.shape[0]
    rs = np.random.RandomState(seed)
    pred = np.empty((B, A, C + 5), np.float32)
    pred[..., :C] = rs.standard_normal((B, A, C)) * 2.0
    conf = rs.standard_normal((B, A)) * 1.0 - 2.0
    for b in range(B):
        for _ in range(12):
            cx, cy, r = rs.uniform(0, SIZE[1]), rs.uniform(0, SIZE[0]), rs.uniform(20, 60)
            conf[b] += 4.0 * np.exp(-((anc[:, 0] - cx) ** 2 + (anc[:, 1] - cy) ** 2) / (2 * r * r))
    pred[..., C] = conf
    pred[..., C + 1:] = rs.standard_normal((B, A, 4)) * 0.3
    return torch.from_numpy(pred).cuda(), torch.from_numpy(anc).cuda(), A


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


def select_leg(C, K, reps, thr):
    dev = torch.device('cuda')
    pred, anchors, A = make_inputs(C, seed=C)
    old = ops.detect_wide if C <= 16 else ops.detect_many
    words = ops.det_workspace_words_wide(B, A, K)
    bufs = {k: ops._det_buffers(B, K, dev) + (torch.empty(words, device=dev, dtype=torch.int32),) for k in ['wide'] + RULES}
    calls = {'wide_hard_total': lambda: old(pred, anchors, SIZE, C, K, 0.4, thr, out=bufs['wide'])}
    for mode, agn in RULES:
        name = f'nms_{mode}' + ('_agnostic' if agn else '')
        calls[name + '_total'] = (lambda m=mode, a=agn: ops.detect_nms(pred, anchors, SIZE, C, K, 0.4, thr, out=bufs[(m, a)],
                                                                       nms_mode=m, nms_agnostic=a))
        if C <= 16:
            calls[name + '_select'] = (lambda m=mode, a=agn: ops.detect_nms(pred, anchors, SIZE, C, K, 0.4, thr, out=bufs[(m, a)],
                                                                            nms_mode=m, nms_agnostic=a, keys_ready=True))
    for f in calls.values():
        f()
    torch.cuda.synchronize()
    if not torch.equal(bufs['wide'][0], bufs[('hard', False)][0]):
        raise SystemExit('nms_modes_bench: the hard class-wise rule of detect_nms disagrees with the wide path')
    us = time_alternating(calls, reps)
    out = {'A': A, 'K': K, 'num_classes': C, 'score_thresh': thr, 'us': us,
           'kept_per_image': {('wide_hard' if k == 'wide' else f'{k[0]}' + ('_agnostic' if k[1] else '')): float(v[0].float().mean())
                              for k, v in bufs.items()}}
    if C <= 16:
        score = us['nms_hard_total'] - us['nms_hard_select']
        out['derived_us'] = {'score_launch': score, 'wide_hard_select': us['wide_hard_total'] - score}
        out['gaussian_select_over_wide_hard_select'] = us['nms_gaussian_select'] / out['derived_us']['wide_hard_select']
    out['gaussian_total_over_wide_hard_total'] = us['nms_gaussian_total'] / us['wide_hard_total']
    return out


def stream_leg(steps, rounds=3, lanes=2):
    cfg = sqd.make_cfg(input_size=SIZE, device='cuda:0', batch_size=B)
    model = SqueezeDet(cfg)
    model.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    det = Detector(model, cfg)
    x = synthetic.make_images(B, SIZE, seed=0).cuda()
    ex = det.stream(lanes=lanes)

    def run_lanes(n):
        last = None
        for _ in range(n):
            ex.submit_device(x)
            while ex.pending() > 2 * lanes - 1:
                last = ex.fetch()[1]
        for _t, last in ex.drain():
            pass
        return last
    rules = [('hard', False), ('gaussian', False), ('hard', True)]
    ms = {r: [] for r in rules}
    kept = {}
    for _ in range(rounds):
        for mode, agn in rules:
            cfg.nms_mode, cfg.nms_agnostic = mode, agn
            run_lanes(max(60, 3 * lanes + 2))                      # eager first use, capture, clocks back up (as bench.py)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = run_lanes(steps)
            torch.cuda.synchronize()
            ms[(mode, agn)].append((time.perf_counter() - t0) / steps * 1e3)
            kept[(mode, agn)] = float(np.mean(last.count))
    if ex.degraded:
        raise SystemExit('nms_modes_bench: a lane did not capture its step')
    name = lambda r: r[0] + ('_agnostic' if r[1] else '')      # noqa: E731
    return {'what': f'Detector.stream(): {lanes} lanes, captured, {B} x {SIZE[0]} x {SIZE[1]}, {steps} steps per window, {rounds} rounds taking turns',
            'ms_per_step_median': {name(r): float(np.median(v)) for r, v in ms.items()},
            'ms_per_step_rounds': {name(r): v for r, v in ms.items()},
            'kept_per_image': {name(r): v for r, v in kept.items()},
            'note': 'the default rule launches byte-identical kernels to the parent commit (profiles/nms_modes_device_asm_diff.log): a '
                    'difference of its step from the parent\'s is run-to-run noise; the spread of the rounds shows its size'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'nms_modes_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('nms_modes_bench: needs a GPU')
    res = {'batch': B, 'reps': args.reps, 'nms_thresh': 0.4, 'nms_sigma': 0.5, 'unit': 'us (median, device events) / ms per step (host clock)',
           'select': {'A16848_K64_C3': select_leg(3, 64, args.reps, 0.3), 'A16848_K1024_C20': select_leg(20, 1024, args.reps, 0.05)},
           'stream': stream_leg(args.steps)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
