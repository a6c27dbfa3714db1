#!/usr/bin/env python
"""Mosaic launch measurements ("Mosaic"), one JSON line on stdout (and, by default, profiles/mosaic_bench.json): 20 output
images of 384x1248 from uint8 sources of 375x1242, device events after warm-up, all launches alternating in one process:

  letterbox_aug / letterbox_aug_color   : the letterbox train entries (null window), the yardstick of this run;
  mosaic_one / mosaic_one_color         : the mosaic entries on 20 one-tile images (rectangle == the same centred window), 20 sources;
  mosaic_four / mosaic_four_color       : ... on 20 four-tile images around drawn centres with zooms in [0.5, 1], 80 sources.
The colour forms are timed with their statistics launch (sqd_image_stats_u8 over 20 or 80 sources), as the loader issues them.

Then the loader-fed Trainer, img/s of one epoch after a warm-up epoch, with mosaic_prob 0 and 1 on an in-memory dataset of such
images (--steps batches of 20), together with the host time to plan, pack and upload a batch.

    python tools/mosaic_bench.py [--reps 200] [--steps 12] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import _native as nat, augment, synthetic  # noqa: E402
from squeezedet_pytorch_amd.boxes import letterbox_window  # noqa: E402
from squeezedet_pytorch_amd.preprocess import KITTI_RGB_MEAN, KITTI_RGB_STD  # noqa: E402

SIZE = (384, 1248)
SRC = (375, 1242)
B = 20


def _upload(images, aug, tiles, color):
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes, True, tiles=len(tiles))
    pk = np.zeros(total, np.uint8)
    augment.write_header(pk, offsets, sizes, aug, color, tiles=tiles)
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    return torch.from_numpy(pk).cuda(), hdr


def bench(reps):
    rs = np.random.RandomState(0)
    images = [rs.randint(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(4 * B)]
    sizes = [im.shape[:2] for im in images]
    boxes = [np.array([[100., 150., 300., 250.]], np.float32)] * (4 * B)
    aug = augment.draw_augmentation(np.random.RandomState(42), sizes, boxes, 1.0, 0.5)
    color = augment.draw_color(np.random.RandomState(44), B, 0.4, 0.4, 0.4)
    drifted = [(h - a[0], w - a[1]) for (h, w), a in zip(sizes, aug)]
    one = np.stack([augment.one_tile(letterbox_window(drifted[b], SIZE), b) for b in range(B)])
    mz = augment.draw_mosaic(np.random.RandomState(45), B, 4 * B, SIZE, 1.0, (0.5, 1.0))
    four = np.stack([augment.mosaic_tiles(drifted[4 * b:4 * b + 4], mz['centre'][b], mz['scale'][b], SIZE, 4 * b) for b in range(B)])
    # the letterbox upload (colour header, null window), the one-tile and the four-tile mosaic uploads
    hdr_l, off_l, total_l = augment.pack_layout(sizes[:B], True)
    pk = np.zeros(total_l, np.uint8)
    augment.write_header(pk, off_l, sizes[:B], aug[:B], color)
    for im, off in zip(images[:B], off_l):
        pk[hdr_l + off:hdr_l + off + im.size] = im.reshape(-1)
    dev_l = torch.from_numpy(pk).cuda()
    dev_1, hdr_1 = _upload(images[:B], aug[:B], one, color)
    dev_4, hdr_4 = _upload(images, aug, four, color)
    out = torch.empty(B, 3, SIZE[0], SIZE[1], device='cuda')
    side = torch.empty(2, B, 2, device='cuda')
    sums = torch.empty(4 * B, 3, 2, dtype=torch.int64, device='cuda')
    mean = (ctypes.c_float * 3)(*[float(v) for v in KITTI_RGB_MEAN])
    std = (ctypes.c_float * 3)(*[float(v) for v in KITTI_RGB_STD])
    st, lib = nat.stream_handle(), nat.lib()
    H, W = SIZE
    o, sm = nat.ptr(out), nat.ptr(sums)

    def at(dev):
        base = dev.data_ptr()
        return lambda off: ctypes.c_void_p(base + off)

    pl, p1, p4 = at(dev_l), at(dev_1), at(dev_4)

    def mosaic(p, hdr, S, colour):
        t = augment.tiles_offset(S)
        if not colour:
            return lambda: lib.sqd_preprocess_u8_mosaic_aug_fwd(p(hdr), p(0), p(8 * S), p(16 * S), p(t), o, mean, std, B, S, H, W, st)
        return lambda: (lib.sqd_image_stats_u8(p(hdr), p(0), p(8 * S), sm, S, st) or
                        lib.sqd_preprocess_u8_mosaic_aug_color_fwd(p(hdr), p(0), p(8 * S), p(16 * S), p(t), p(t + 144 * B), sm, o, mean, std, B, S, H, W, st))

    launches = {
        'letterbox_aug': lambda: lib.sqd_preprocess_u8_letterbox_aug_fwd(pl(hdr_l), pl(0), pl(8 * B), pl(16 * B), None, o, nat.ptr(side[0]),
                                                                        nat.ptr(side[1]), mean, std, B, H, W, st),
        'letterbox_aug_color': lambda: (lib.sqd_image_stats_u8(pl(hdr_l), pl(0), pl(8 * B), sm, B, st) or
                                        lib.sqd_preprocess_u8_letterbox_aug_color_fwd(pl(hdr_l), pl(0), pl(8 * B), pl(16 * B), None, pl(28 * B), sm, o,
                                                                                      nat.ptr(side[0]), nat.ptr(side[1]), mean, std, B, H, W, st)),
        'mosaic_one': mosaic(p1, hdr_1, B, False), 'mosaic_one_color': mosaic(p1, hdr_1, B, True),
        'mosaic_four': mosaic(p4, hdr_4, 4 * B, False), 'mosaic_four_color': mosaic(p4, hdr_4, 4 * B, True),
    }
    for f in launches.values():
        for _ in range(20):
            nat.check(f(), 'warm-up')
    torch.cuda.synchronize()
    times = {k: [] for k in launches}
    for _ in range(reps):                                   # alternate (same clocks, same caches)
        for k, f in launches.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            times[k].append((a, b))
    torch.cuda.synchronize()
    us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in times.items()}
    med = {k: float(np.median(v)) for k, v in us.items()}
    return {'median_us': med, 'p10_p90_us': {k: [float(np.percentile(v, q)) for q in (10, 90)] for k, v in us.items()},
            'over_letterbox_aug': {k: med[k] / med['letterbox_aug'] for k in ('mosaic_one', 'mosaic_four')},
            'over_letterbox_aug_color': {k: med[k] / med['letterbox_aug_color'] for k in ('mosaic_one_color', 'mosaic_four_color')},
            'upload_bytes': {'letterbox': int(dev_l.numel()), 'mosaic_one': int(dev_1.numel()), 'mosaic_four': int(dev_4.numel())},
            'reps': reps, 'batch': B, 'source': list(SRC), 'canvas': list(SIZE)}


class _Dataset:
    def __init__(self, n):
        rs = np.random.RandomState(1)
        self.images = [rs.randint(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(n)]
        self.ann = []
        for _ in range(n):
            m = int(rs.randint(2, 7))
            x1, y1 = rs.uniform(0, SRC[1] * 0.7, m), rs.uniform(0, SRC[0] * 0.6, m)
            self.ann.append((rs.randint(0, 3, m).astype(np.int64),
                             np.stack([x1, y1, x1 + rs.uniform(30, 300, m), y1 + rs.uniform(30, 140, m)], 1).astype(np.float32)))
        self.rgb_mean, self.rgb_std = KITTI_RGB_MEAN, KITTI_RGB_STD

    def __len__(self):
        return len(self.images)

    def load_image(self, i):
        return self.images[i], f'{i:06d}'

    def image_size(self, i):
        return self.images[i].shape[:2]

    def load_annotations(self, i):
        return self.ann[i][0].copy(), self.ann[i][1].copy()


def trainer(steps):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import Trainer
    ds = _Dataset(B * steps)
    out = {}
    for prob in (0.0, 1.0):
        cfg = sqd.make_cfg(device='cuda', batch_size=B, letterbox=True, mosaic_prob=prob, sparse_gt=True)
        cfg.num_iters, cfg.print_interval = -1, 10 ** 6
        m = SqueezeDetWithLoss(cfg)
        m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234), strict=True)
        opt = torch.optim.SGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=1e-4)
        tr = Trainer(m.cuda(), opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
        loader = TrainLoader(ds, cfg, seed=1)
        tr.run_epoch('train', 1, loader)                    # warm-up: plans, pinned buffers, caches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = tr.run_epoch('train', 2, loader)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # the loader alone: host planning, packing and upload, no network behind it
        t0 = time.perf_counter()
        n = sum(b['image'].shape[0] for b in loader)
        torch.cuda.synchronize()
        dl = time.perf_counter() - t0
        out[f'mosaic_prob_{prob:g}'] = {'img_per_s': B * steps / dt, 'loader_only_img_per_s': n / dl, 'loss': float(stats['loss'])}
    out['mosaic_over_plain_img_per_s'] = out['mosaic_prob_1']['img_per_s'] / out['mosaic_prob_0']['img_per_s']
    out['steps'], out['batch'] = steps, B
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--steps', type=int, default=12)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mosaic_bench.json'))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'device': torch.cuda.get_device_name(0), 'kernel': bench(args.reps), 'trainer': trainer(args.steps)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
