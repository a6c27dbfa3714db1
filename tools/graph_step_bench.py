#!/usr/bin/env python
"""``Trainer.train_epoch`` with ``cfg.graph_step`` off and on ("The captured training step in the product"), one JSON line:
SqueezeDet bs=20 1248x384, fused optimizer, dropout on, over

  synthetic : a list of device-resident synthetic batches (four distinct ones in turn, 524 MB together -- more than the 256 MB
              Infinity Cache, so the staging copies read their source from HBM as they would with real data; no input cost);
  loader    : a ``TrainLoader`` (8 workers) on an in-memory uint8 dataset of KITTI-sized images.

The two modes run in ONE process, alternating (off, on, off per round: the off leg twice shows the spread), each on a model and an
optimizer of its own from the same state dict.  Round 0 warms every shape of both modes up (plans, workspaces, the capture) and is not
reported.  Every window is a host clock around an epoch that ends in a device synchronise; no profiler runs.  Afterwards a short pass of
the on mode with device events around the staging copies (wrapped around ``GraphedStep._stage`` here, not in the product) gives
their share of the step.

    python tools/graph_step_bench.py [--iters 200] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import synthetic  # noqa: E402
from augment_bench import MemKitti  # noqa: E402

SIZE = (384, 1248)
B = 20


def make_trainer(graph_step, workers):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, Trainer, find_base
    cfg = sqd.make_cfg(input_size=SIZE, device='cuda', batch_size=B, num_workers=workers, graph_step=graph_step)
    cfg.print_interval = 10 ** 9
    model = SqueezeDetWithLoss(cfg)
    model.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    model = model.cuda().train()
    base = find_base(model)
    opt = FusedClipSGD([p for p in model.parameters() if p.requires_grad], lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay,
                       max_norm=cfg.grad_norm, flat_grad=lambda: base.last_grad_flat)
    return Trainer(model, opt, torch.optim.lr_scheduler.StepLR(opt, 10 ** 6), cfg), cfg


def epoch_seconds(tr, loader):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train_epoch(1, loader)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('graph_step_bench: needs the GPU (a timing taken elsewhere says nothing)')
    torch.cuda.set_device(0)
    from squeezedet_pytorch_amd.train_data import TrainLoader
    torch.manual_seed(0)
    trainers = {'off': make_trainer(False, args.workers), 'on': make_trainer(True, args.workers)}
    cfg = trainers['off'][1]
    distinct = [{'image': synthetic.make_images(B, SIZE, seed=i).cuda(),
                 'gt': synthetic.make_gt(B, cfg.anchors, SIZE, cfg.num_classes, seed=10 + i).cuda(), 'image_meta': {}} for i in range(4)]
    synth = [distinct[i % 4] for i in range(args.iters)]
    ds = MemKitti(B * args.iters)
    inputs = {'synthetic': lambda mode, rnd: synth,
              'loader': lambda mode, rnd: TrainLoader(ds, trainers[mode][1], seed=rnd)}
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'input_size': list(SIZE), 'iters_per_window': args.iters,
           'rounds': args.rounds, 'workers': args.workers, 'legs': {}}
    for name, make in inputs.items():
        ms = {'off': [], 'on': []}
        for rnd in range(args.rounds + 1):                       # round 0: warm-up of every shape in both modes
            for mode in ('off', 'on', 'off'):
                sec = epoch_seconds(trainers[mode][0], make(mode, rnd))
                if rnd:
                    ms[mode].append(1e3 * sec / args.iters)
        off, on = float(np.median(ms['off'])), float(np.median(ms['on']))
        spread = (max(ms['off']) - min(ms['off'])) / off
        res['legs'][name] = {
            'off': {'ms_per_step': round(off, 4), 'img_per_s': round(1e3 * B / off, 1), 'windows_ms_per_step': [round(v, 4) for v in ms['off']]},
            'on': {'ms_per_step': round(on, 4), 'img_per_s': round(1e3 * B / on, 1), 'windows_ms_per_step': [round(v, 4) for v in ms['on']]},
            'off_spread_rel': round(spread, 4), 'on_over_off_time': round(on / off, 4),
            'on_faster_than_off_beyond_spread': bool(on < min(ms['off']) and (off - on) / off > spread),
        }
    # the staging copies' share of the captured step: device events around them, in a pass of its own (the events cost host time)
    gs = trainers['on'][0].graphed_step()
    events, stage = [], gs._stage

    def timed_stage(key, batch):                                 # (called on the step's stream: the events bracket the copies alone)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        out = stage(key, batch)
        ev[1].record()
        events.append(ev)
        return out
    gs._stage = timed_stage
    epoch_seconds(trainers['on'][0], synth[:40])
    del gs._stage
    stage_ms = [a.elapsed_time(b) for a, b in events]
    res['staging'] = {'median_ms_per_step': round(float(np.median(stage_ms)), 4), 'steps': len(stage_ms),
                      'share_of_on_step_synthetic': round(float(np.median(stage_ms)) / res['legs']['synthetic']['on']['ms_per_step'], 4),
                      'what': 'device-to-device copies of image [20,3,384,1248] and dense gt [20,16848,12] (131 MB) into the static buffers, four distinct '
                              'source batches in turn'}
    res['captures'] = gs.captures
    res['replays'] = gs.replays
    res['eager_steps_in_on_mode'] = gs.eager_steps
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
