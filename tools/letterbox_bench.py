#!/usr/bin/env python
"""Letterbox launch measurements ("Letterbox and zoom-out"), one JSON line on stdout: on 20 uint8 images of 375x1242
onto the 384x1248 canvas (window 377x1248: the kernel's own centred one), device events after warm-up, all launches alternating in
one process:

  plain_resize / letterbox          : sqd_preprocess_u8_fwd against sqd_preprocess_u8_letterbox_fwd;
  aug_resize / letterbox_aug        : sqd_preprocess_u8_aug_fwd against sqd_preprocess_u8_letterbox_aug_fwd (null window);
  letterbox_aug_zoom                : the same with host-given zoom-out windows (zoom_out = 0.5), for the cost of a mostly empty canvas.

    python tools/letterbox_bench.py [--reps 200] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squeezedet_pytorch_amd import _native as nat, augment  # noqa: E402
from squeezedet_pytorch_amd.boxes import letterbox_window  # noqa: E402
from squeezedet_pytorch_amd.preprocess import KITTI_RGB_MEAN, KITTI_RGB_STD  # noqa: E402

SIZE = (384, 1248)
SRC = (375, 1242)
B = 20


def bench(reps):
    rs = np.random.RandomState(0)
    images = [rs.randint(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(B)]
    sizes = [im.shape[:2] for im in images]
    rng = np.random.RandomState(42)
    boxes = [np.array([[100., 150., 300., 250.]], np.float32)] * B
    aug = augment.draw_augmentation(rng, sizes, boxes, 1.0, 0.5)
    wins = np.array([letterbox_window((h - a[0], w - a[1]), SIZE) for (h, w), a in zip(sizes, aug)], np.int32)
    zoom = augment.draw_zoom(np.random.RandomState(43), wins, SIZE, 0.5)
    hdr, offsets, total = augment.pack_layout(sizes, window=True)
    pk = np.zeros(total, np.uint8)
    augment.write_header(pk, offsets, sizes, aug, None, zoom)
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    dev = torch.from_numpy(pk).cuda()
    out = torch.empty(B, 3, SIZE[0], SIZE[1], device='cuda')
    scales = torch.empty(B, 2, device='cuda')
    shifts = torch.empty(B, 2, device='cuda')
    base = dev.data_ptr()
    p = lambda off: ctypes.c_void_p(base + off)      # noqa: E731
    mean = (ctypes.c_float * 3)(*[float(v) for v in KITTI_RGB_MEAN])
    std = (ctypes.c_float * 3)(*[float(v) for v in KITTI_RGB_STD])
    st = nat.stream_handle()
    lib = nat.lib()
    H, W = SIZE
    o, sc, sh = nat.ptr(out), nat.ptr(scales), nat.ptr(shifts)
    win = p(augment.window_offset(B))
    launches = {
        'plain_resize': lambda: lib.sqd_preprocess_u8_fwd(p(hdr), p(0), p(8 * B), o, sc, mean, std, B, H, W, st),
        'letterbox': lambda: lib.sqd_preprocess_u8_letterbox_fwd(p(hdr), p(0), p(8 * B), None, o, sc, sh, mean, std, B, H, W, st),
        'aug_resize': lambda: lib.sqd_preprocess_u8_aug_fwd(p(hdr), p(0), p(8 * B), p(16 * B), o, sc, mean, std, B, H, W, st),
        'letterbox_aug': lambda: lib.sqd_preprocess_u8_letterbox_aug_fwd(p(hdr), p(0), p(8 * B), p(16 * B), None, o, sc, sh, mean, std, B, H, W, st),
        'letterbox_aug_zoom': lambda: lib.sqd_preprocess_u8_letterbox_aug_fwd(p(hdr), p(0), p(8 * B), p(16 * B), win, o, sc, sh, mean, std, B, H, W, st),
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
            'letterbox_over_plain_resize': med['letterbox'] / med['plain_resize'],
            'letterbox_aug_over_aug_resize': med['letterbox_aug'] / med['aug_resize'],
            'letterbox_aug_zoom_over_aug_resize': med['letterbox_aug_zoom'] / med['aug_resize'],
            'reps': reps, 'batch': B, 'source': list(SRC), 'canvas': list(SIZE)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {'device': torch.cuda.get_device_name(0), 'kernel': bench(args.reps)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
