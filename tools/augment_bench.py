#!/usr/bin/env python
"""Training input pipeline measurements ("Training input on the GPU"), one JSON line on stdout:

  kernel  : the augmented preprocessing launch against the plain one on the same 20-image KITTI-sized uint8 batch (device events
            after warm-up, the two alternating in one process), both branches; and the colour-jitter call (statistics launches +
            colour launch) in its table form (saturation factor 1) and its per-tap form, against the augmented launch;
  loader  : TrainLoader throughput (img/s) over an in-memory uint8 dataset, num_workers 4 and 8;
  trainer : Trainer.run_epoch img/s fed by TrainLoader (8 workers) against the same Trainer over device-resident synthetic batches,
            and fed by the same loader with colour jitter on.

    python tools/augment_bench.py [--reps 200] [--iters 30] [--out FILE]
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
from squeezedet_pytorch_amd import _native as nat, augment, synthetic  # noqa: E402
from squeezedet_pytorch_amd.preprocess import KITTI_RGB_MEAN, KITTI_RGB_STD  # noqa: E402

SIZE = (384, 1248)
B = 20


def kitti_images(n, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, ((375, 1242), (370, 1224))[i % 2] + (3,), dtype=np.uint8) for i in range(n)]


def kitti_boxes(rs, h, w):
    m = int(rs.randint(3, 9))
    x1 = rs.uniform(0, w * 0.8, m); y1 = rs.uniform(h * 0.3, h * 0.7, m)
    b = np.stack([x1, y1, x1 + rs.uniform(20, 150, m), y1 + rs.uniform(20, 100, m)], 1).astype(np.float32)
    return rs.randint(0, 3, m).astype(np.int16), b


def bench_kernels(reps):
    images = kitti_images(B)
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes)
    pk = np.zeros(total, np.uint8)
    rng = np.random.RandomState(42)
    aug = augment.draw_augmentation(rng, sizes, [kitti_boxes(rng, h, w)[1] for h, w in sizes], 1.0, 0.5)
    augment.write_header(pk, offsets, sizes, aug)
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    dev = torch.from_numpy(pk).cuda()
    out = torch.empty(B, 3, SIZE[0], SIZE[1], device='cuda')
    side = torch.empty(B, 8, device='cuda', dtype=torch.int32)
    import ctypes
    base = dev.data_ptr()
    p = lambda off: ctypes.c_void_p(base + off)      # noqa: E731
    mean = (ctypes.c_float * 3)(*[float(v) for v in KITTI_RGB_MEAN])
    std = (ctypes.c_float * 3)(*[float(v) for v in KITTI_RGB_STD])
    st = nat.stream_handle()
    lib = nat.lib()
    # the same batch and draws with the colour header: factors with saturation 1 (table form) and with all three drawn (per-tap form)
    hdr_c, offsets_c, total_c = augment.pack_layout(sizes, color=True)
    crng = np.random.RandomState(43)
    dev_c = {}
    for name, jit in (('table', (0.4, 0.4, 0.)), ('pertap', (0.4, 0.4, 0.4))):
        pkc = np.zeros(total_c, np.uint8)
        augment.write_header(pkc, offsets_c, sizes, aug, augment.draw_color(crng, B, *jit))
        pkc[hdr_c:] = pk[hdr:]
        dev_c[name] = torch.from_numpy(pkc).cuda()
    sums = torch.empty(B, 3, 2, device='cuda', dtype=torch.int64)

    def color_call(name, forbid):                     # the statistics call (zeroing + sums launches), then the colour launch
        base_c = dev_c[name].data_ptr()
        q = lambda off: ctypes.c_void_p(base_c + off)      # noqa: E731

        def f():
            rc = lib.sqd_image_stats_u8(q(hdr_c), q(0), q(8 * B), nat.ptr(sums), B, st)
            if forbid:
                return rc or lib.sqd_preprocess_u8_padcrop_aug_color_fwd(q(hdr_c), q(0), q(8 * B), q(16 * B), q(28 * B), nat.ptr(sums), nat.ptr(out),
                                                                         None, nat.ptr(side), mean, std, B, SIZE[0], SIZE[1], st)
            return rc or lib.sqd_preprocess_u8_aug_color_fwd(q(hdr_c), q(0), q(8 * B), q(16 * B), q(28 * B), nat.ptr(sums), nat.ptr(out),
                                                             nat.ptr(side), mean, std, B, SIZE[0], SIZE[1], st)
        return f
    launches = {
        'plain_resize': lambda: lib.sqd_preprocess_u8_fwd(p(hdr), p(0), p(8 * B), nat.ptr(out), nat.ptr(side), mean, std, B, SIZE[0], SIZE[1], st),
        'aug_resize': lambda: lib.sqd_preprocess_u8_aug_fwd(p(hdr), p(0), p(8 * B), p(16 * B), nat.ptr(out), nat.ptr(side), mean, std, B,
                                                            SIZE[0], SIZE[1], st),
        'plain_padcrop': lambda: lib.sqd_preprocess_u8_padcrop_fwd(p(hdr), p(0), p(8 * B), nat.ptr(out), None, nat.ptr(side), mean, std, B,
                                                                   SIZE[0], SIZE[1], st),
        'aug_padcrop': lambda: lib.sqd_preprocess_u8_padcrop_aug_fwd(p(hdr), p(0), p(8 * B), p(16 * B), nat.ptr(out), None, nat.ptr(side),
                                                                     mean, std, B, SIZE[0], SIZE[1], st),
        'stats': lambda: lib.sqd_image_stats_u8(p(hdr), p(0), p(8 * B), nat.ptr(sums), B, st),
        'color_table_resize': color_call('table', False),
        'color_pertap_resize': color_call('pertap', False),
        'color_table_padcrop': color_call('table', True),
        'color_pertap_padcrop': color_call('pertap', True),
    }
    for f in launches.values():
        for _ in range(20):
            nat.check(f(), 'warm-up')
    torch.cuda.synchronize()
    times = {k: [] for k in launches}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(len(launches) * reps)]
    j = 0
    for _ in range(reps):                                   # alternate: plain, aug, plain, aug ... (same clocks, same caches)
        for k, f in launches.items():
            ev[j][0].record()
            f()
            ev[j][1].record()
            times[k].append(ev[j])
            j += 1
    torch.cuda.synchronize()
    us = {k: float(np.median([a.elapsed_time(b) * 1e3 for a, b in v])) for k, v in times.items()}
    pct = {k: [float(np.percentile([a.elapsed_time(b) * 1e3 for a, b in v], q)) for q in (10, 90)] for k, v in times.items()}
    return {'median_us': us, 'p10_p90_us': pct,
            'color_table_over_aug_resize': us['color_table_resize'] / us['aug_resize'],
            'color_pertap_over_aug_resize': us['color_pertap_resize'] / us['aug_resize'],
            'color_table_over_aug_padcrop': us['color_table_padcrop'] / us['aug_padcrop'],
            'color_pertap_over_aug_padcrop': us['color_pertap_padcrop'] / us['aug_padcrop'], 'aug_over_plain_resize': us['aug_resize'] / us['plain_resize'],
            'aug_over_plain_padcrop': us['aug_padcrop'] / us['plain_padcrop'], 'reps': reps, 'batch': B,
            'target_ratio': 1.15}


class MemKitti:
    """In-memory stand-in for the reference's KITTI dataset (decode speed is out of scope): uint8 pixels, KITTI sizes."""

    def __init__(self, n, distinct=40):
        self.n = n
        self.images = kitti_images(distinct, seed=1)
        rs = np.random.RandomState(2)
        self.ann = [kitti_boxes(rs, *im.shape[:2]) for im in self.images]
        self.rgb_mean, self.rgb_std = KITTI_RGB_MEAN.reshape(1, 1, 3), KITTI_RGB_STD.reshape(1, 1, 3)

    def __len__(self):
        return self.n

    def load_image(self, i):
        return self.images[i % len(self.images)], f'{i:06d}'

    def load_annotations(self, i):
        c, b = self.ann[i % len(self.ann)]
        return c.copy(), b.copy()


def bench_loader(workers, iters):
    from squeezedet_pytorch_amd.train_data import TrainLoader
    cfg = sqd.make_cfg(input_size=SIZE, device='cuda', batch_size=B, num_workers=workers)
    ld = TrainLoader(MemKitti(B * (iters + 3)), cfg, seed=1)
    it = iter(ld)
    for _ in range(3):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for b in it:
        n += b['image'].shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def bench_trainer(iters, workers=8):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, Trainer, find_base
    cfg = sqd.make_cfg(input_size=SIZE, device='cuda', batch_size=B, num_workers=workers)
    cfg.print_interval = 10 ** 9
    model = SqueezeDetWithLoss(cfg)
    model.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    model = model.cuda().train()
    base = find_base(model)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = FusedClipSGD(params, lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay, max_norm=cfg.grad_norm,
                       flat_grad=lambda: base.last_grad_flat)
    tr = Trainer(model, opt, torch.optim.lr_scheduler.StepLR(opt, 10 ** 6), cfg)
    x = synthetic.make_images(B, SIZE, seed=0).cuda()
    gt = synthetic.make_gt(B, cfg.anchors, SIZE, cfg.num_classes, seed=1).cuda()
    synth = [{'image': x, 'gt': gt, 'image_meta': {}}] * iters
    ds = MemKitti(B * iters)
    out = {}
    cfg_c = sqd.make_cfg(input_size=SIZE, device='cuda', batch_size=B, num_workers=workers, brightness_jitter=0.4, contrast_jitter=0.4,
                         saturation_jitter=0.4)
    runs = {}
    for rnd in range(4):                                   # round 0 warms the paths up; rounds 1-3 are measured, interleaved
        for name, make in (('synthetic', lambda: synth), ('loader', lambda: TrainLoader(ds, cfg, seed=rnd)),
                           ('loader_color', lambda: TrainLoader(ds, cfg_c, seed=rnd))):
            loader = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.run_epoch('train', 1, loader)
            torch.cuda.synchronize()
            if rnd:
                runs.setdefault(name, []).append(B * iters / (time.perf_counter() - t0))
    out = {k: float(np.median(v)) for k, v in runs.items()}
    return {'img_per_s': out, 'img_per_s_runs': runs, 'loader_over_synthetic': out['loader'] / out['synthetic'],
            'loader_color_over_loader': out['loader_color'] / out['loader'], 'workers': workers, 'iters': iters, 'target_ratio': 0.90}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default='kernel,loader,trainer')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    parts = args.only.split(',')
    res = {'device': torch.cuda.get_device_name(0)}
    if 'kernel' in parts:
        res['kernel'] = bench_kernels(args.reps)
    if 'loader' in parts:
        res['loader_img_per_s'] = {str(w): bench_loader(w, args.iters) for w in (4, 8)}
    if 'trainer' in parts:
        res['trainer'] = bench_trainer(args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
