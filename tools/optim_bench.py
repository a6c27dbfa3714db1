#!/usr/bin/env python
"""The optimizer launches alone ("AdamW and a weight EMA in the one-launch step"), one JSON line.

For the parameter sets of SqueezeDet (64 tensors) and SqueezeDet+, with device events around runs of back-to-back steps on a flat
gradient buffer, in ONE process and interleaved round by round:

  sgd        sqd_grad_sumsq + sqd_sgd_clip_step_chunked_dev                       (the existing kernel: 5 streams of the parameter size)
  sgd_ema    sqd_grad_sumsq + sqd_optim_begin + sqd_sgd_clip_step_chunked_ema     (7 streams)
  adamw      sqd_grad_sumsq + sqd_optim_begin + sqd_adamw_clip_step_chunked       (7 streams)
  adamw_ema  the same with the EMA                                                (9 streams)
  torch      clip_grad_norm_(foreach) + torch.optim.AdamW (fused if it runs here, else foreach) + torch._foreach_lerp_ for the EMA

The streams of a step launch: p and the states read and written, the gradient read (the norm launch reads the gradient once more: it
is counted in ``bytes_per_step`` and reported apart in ``step_launch_bytes``).  Each fused variant is also timed without its norm and
begin launches (``step_launch_us``), which is what ``step_launch_gb_per_s`` is computed from, and as 20 whole steps captured into one
hipGraph (``launches_replayed_us`` per step: the device time of all launches of a step, with no host in between; ``launches_us`` is
``optimizer.step()`` called back to back, host time included, as the torch sequence is timed).  With ``--whole-step`` the training step of
``cfg.graph_step`` at bs = 20 is timed as tools/graph_step_bench.py times it (host clock around ``Trainer.train_epoch`` on
device-resident synthetic batches) with SGD against AdamW + EMA, alternating.

    python tools/optim_bench.py [--iters 200] [--rounds 5] [--whole-step] [--out FILE]
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
from squeezedet_pytorch_amd import synthetic  # noqa: E402

STREAMS = {'sgd': 5, 'sgd_ema': 7, 'adamw': 7, 'adamw_ema': 9}


def param_sizes(arch):
    return [int(v.numel()) for v in synthetic.make_state_dict(arch, seed=1234).values()]


class Fused:
    """One fused variant on parameters and a flat gradient of its own; ``full()`` = every launch of a step, ``step_only()`` = the big one."""

    def __init__(self, kind, sizes, seed):
        from squeezedet_pytorch_amd.trainer import FusedClipAdamW, FusedClipSGD
        g = torch.Generator(device='cuda').manual_seed(seed)
        self.params = [torch.nn.Parameter(torch.randn(n, device='cuda', generator=g) * 0.05) for n in sizes]
        self.flat = torch.randn(sum(sizes), device='cuda', generator=g) * 0.01
        off = 0
        for p in self.params:
            p.grad = self.flat[off:off + p.numel()]; off += p.numel()
        ema = dict(ema_decay=0.999) if kind.endswith('_ema') else {}
        if kind.startswith('sgd'):
            self.opt = FusedClipSGD(self.params, lr=1e-3, momentum=0.9, weight_decay=1e-4, max_norm=5.0, flat_grad=lambda: self.flat, **ema)
            self.opt.hyper_on_device = True
        else:
            self.opt = FusedClipAdamW(self.params, lr=1e-4, weight_decay=1e-2, max_norm=5.0, flat_grad=lambda: self.flat, **ema)
        self.kind = kind
        self.opt.step()                                  # tables, workspaces, the hyper table

    def full(self):
        self.opt.step()

    def captured(self, steps=20):
        """``steps`` whole steps captured into one hipGraph: its replay time is the device time of the launches, no host in between."""
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(steps):
                self.opt.step()
        return g, steps

    def step_only(self):
        from squeezedet_pytorch_amd import _native as nat
        o, lib = self.opt, nat.lib()
        st = nat.stream_handle(self.flat.device)
        parts, norm = o._norm_ws[:-1], o._norm_ws[-1]
        args = (nat.ptr(o._table), nat.ptr(o._chunks), o._chunks.shape[0], nat.ptr(self.flat), nat.ptr(parts))
        derived = o._steps_dev[2:6].view(torch.float32) if o._steps_dev is not None else None
        if self.kind == 'sgd':
            nat.check(lib.sqd_sgd_clip_step_chunked_dev(*args, nat.ptr(norm), nat.ptr(o._hyper_dev), st), 'sgd')
        elif self.kind == 'sgd_ema':
            nat.check(lib.sqd_sgd_clip_step_chunked_ema(*args, nat.ptr(norm), nat.ptr(o._hyper_dev), nat.ptr(derived), st), 'sgd_ema')
        else:
            nat.check(lib.sqd_adamw_clip_step_chunked(*args, None, nat.ptr(norm), nat.ptr(o._hyper_dev), nat.ptr(derived),
                                                      int(self.kind == 'adamw_ema'), st), 'adamw')


class TorchAdamWEma:
    """What a user would otherwise write: clip_grad_norm_ + torch.optim.AdamW in its fastest mode here + a foreach lerp for the EMA."""

    def __init__(self, sizes, seed):
        g = torch.Generator(device='cuda').manual_seed(seed)
        self.params = [torch.nn.Parameter(torch.randn(n, device='cuda', generator=g) * 0.05) for n in sizes]
        for p in self.params:
            p.grad = torch.randn(p.numel(), device='cuda', generator=g) * 0.01
        self.ema = [p.detach().clone() for p in self.params]
        self.mode = None
        for mode in ('fused', 'foreach'):
            try:
                self.opt = torch.optim.AdamW(self.params, lr=1e-4, weight_decay=1e-2, **{mode: True})
                self.opt.step()
                torch.cuda.synchronize()
                self.mode = mode
                break
            except Exception:                            # (the fused implementation may be missing in this build)
                continue
        if self.mode is None:
            raise SystemExit('optim_bench: torch.optim.AdamW runs neither fused nor foreach here')

    def full(self):
        torch.nn.utils.clip_grad_norm_(self.params, 5.0, foreach=True)
        self.opt.step()
        with torch.no_grad():
            torch._foreach_lerp_(self.ema, [p.detach() for p in self.params], 1.0 - 0.999)


def time_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def bench_set(arch, iters, rounds):
    sizes = param_sizes(arch)
    total = sum(sizes)
    legs = {k: Fused(k, sizes, i) for i, k in enumerate(STREAMS)}
    tor = TorchAdamWEma(sizes, 9)
    graphs = {k: leg.captured() for k, leg in legs.items()}
    times = {k: {'full': [], 'step': [], 'graph': []} for k in legs}
    times['torch'] = {'full': []}
    for rnd in range(rounds + 1):                        # round 0 warms up and is not reported
        for k, leg in legs.items():
            f, s = time_us(leg.full, iters), time_us(leg.step_only, iters)
            g, n = graphs[k]
            r = time_us(g.replay, max(5, iters // n)) / n
            if rnd:
                times[k]['full'].append(f); times[k]['step'].append(s); times[k]['graph'].append(r)
        t = time_us(tor.full, max(10, iters // 4))
        if rnd:
            times['torch']['full'].append(t)
    out = {'tensors': len(sizes), 'floats': total, 'variants': {}}
    for k, n in STREAMS.items():
        full, step = float(np.median(times[k]['full'])), float(np.median(times[k]['step']))
        out['variants'][k] = {'streams': n, 'step_launch_bytes': 4 * n * total, 'bytes_per_step': 4 * (n + 1) * total,
                              'launches_us': round(full, 2), 'launches_replayed_us': round(float(np.median(times[k]['graph'])), 2),
                              'step_launch_us': round(step, 2),
                              'step_launch_gb_per_s': round(4 * n * total / step / 1e3, 1),
                              'windows_launches_us': [round(v, 2) for v in times[k]['full']]}
    t = float(np.median(times['torch']['full']))
    out['variants']['torch'] = {'what': f'clip_grad_norm_(foreach) + torch.optim.AdamW({tor.mode}) + torch._foreach_lerp_', 'launches_us': round(t, 2),
                                'windows_launches_us': [round(v, 2) for v in times['torch']['full']]}
    fused = out['variants']['adamw_ema']['launches_us']
    out['adamw_ema_fused_over_torch_time'] = round(fused / t, 4)
    out['fused_faster_than_torch'] = bool(max(times['adamw_ema']['full']) < min(times['torch']['full']))
    sgd_bw = out['variants']['sgd']['step_launch_gb_per_s']
    for k in ('sgd_ema', 'adamw', 'adamw_ema'):
        out['variants'][k]['gb_per_s_over_sgd'] = round(out['variants'][k]['step_launch_gb_per_s'] / sgd_bw, 3)
    return out


def whole_step(iters, rounds):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, FusedClipSGD, Trainer, find_base
    size, B = (384, 1248), 20

    def make(kind):
        cfg = sqd.make_cfg(input_size=size, device='cuda', batch_size=B, graph_step=True)
        cfg.print_interval = 10 ** 9
        model = SqueezeDetWithLoss(cfg)
        model.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
        model = model.cuda().train()
        base = find_base(model)
        params = [p for p in model.parameters() if p.requires_grad]
        if kind == 'sgd':
            opt = FusedClipSGD(params, lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay, max_norm=cfg.grad_norm,
                               flat_grad=lambda: base.last_grad_flat)
        else:
            opt = FusedClipAdamW(params, lr=1e-4, weight_decay=1e-2, max_norm=cfg.grad_norm, ema_decay=0.999,
                                 flat_grad=lambda: base.last_grad_flat)
        return Trainer(model, opt, torch.optim.lr_scheduler.StepLR(opt, 10 ** 6), cfg), cfg
    torch.manual_seed(0)
    trainers = {'sgd': make('sgd'), 'adamw_ema': make('adamw_ema')}
    cfg = trainers['sgd'][1]
    distinct = [{'image': synthetic.make_images(B, size, seed=i).cuda(),
                 'gt': synthetic.make_gt(B, cfg.anchors, size, cfg.num_classes, seed=10 + i).cuda(), 'image_meta': {}} for i in range(4)]
    synth = [distinct[i % 4] for i in range(iters)]
    ms = {k: [] for k in trainers}
    for rnd in range(rounds + 1):
        for k in ('sgd', 'adamw_ema', 'sgd'):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainers[k][0].train_epoch(1, synth)
            torch.cuda.synchronize()
            if rnd:
                ms[k].append(1e3 * (time.perf_counter() - t0) / iters)
    gs = {k: trainers[k][0].graphed_step() for k in trainers}
    return {'batch': B, 'input_size': list(size), 'iters_per_window': iters,
            'ms_per_step': {k: round(float(np.median(v)), 4) for k, v in ms.items()},
            'windows_ms_per_step': {k: [round(x, 4) for x in v] for k, v in ms.items()},
            'captures': {k: g.captures for k, g in gs.items()}, 'replays': {k: g.replays for k, g in gs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--whole-step', action='store_true')
    ap.add_argument('--step-iters', type=int, default=100)
    ap.add_argument('--step-rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_bench: needs the GPU (a timing taken elsewhere says nothing)')
    torch.cuda.set_device(0)
    res = {'device': torch.cuda.get_device_name(0), 'iters_per_window': args.iters, 'rounds': args.rounds,
           'sets': {arch: bench_set(arch, args.iters, args.rounds) for arch in ('squeezedet', 'squeezedetplus')}}
    if args.whole_step:
        res['whole_step'] = whole_step(args.step_iters, args.step_rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
