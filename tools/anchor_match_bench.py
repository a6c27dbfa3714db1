#!/usr/bin/env python
"""Cost of the IoU-threshold matcher at KITTI size ("IoU-threshold matching"), one JSON line on stdout and in
--out.  B = 20, A = 16 848 (24 x 78 x 9), the boxes of ``synthetic.make_gt_boxes`` (3..8 per image, 20..400 px):

  encode   : the sparse encode as it was (``ops.encode_gt`` alone) against encode + ``ops.anchor_match`` at match_iou 0.5 (band from
             0.4) and 0.7 (band from 0.6), and the matcher's two launches on their own; with the per-image positives, band and
             overflow seen
  loss     : the masked loss forward (mean form) and backward on the encoder's list (an all-zero bitmap) and on the matcher's lists
  trainer  : ``Trainer.run_epoch`` fed by ``TrainLoader`` on an in-memory dataset of input-sized images, ms per step with the
             feature off and on (the second of two epochs: wall clock around the epoch, the device drained at both ends)

Device events around each call after warm-up, enqueued behind a spin kernel so that they bracket device time only.  Nothing here has
a pass mark.

    python tools/anchor_match_bench.py [--reps 100] [--steps 10] [--out profiles/anchor_match_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import ops, synthetic  # noqa: E402
from squeezedet_pytorch_amd.annotations import pack_annotations  # noqa: E402
from ignore_regions_bench import time_alternating  # noqa: E402
from many_class_bench import B, SIZE, WEIGHTS  # noqa: E402

MATCH = {'iou0.5': (0.5, 0.4, 512), 'iou0.7': (0.7, 0.6, 512)}


def kernels(cfg, reps):
    A, C = cfg.num_anchors, cfg.num_classes
    anchors = torch.from_numpy(cfg.anchors).float().cuda()
    a64 = torch.from_numpy(np.asarray(cfg.anchors, np.float64)).cuda()
    cls_list, box_list = synthetic.make_gt_boxes(B, SIZE, num_classes=C, seed=1)
    bx, cl, offs = pack_annotations(cls_list, box_list)
    d_boxes, d_cls, d_offs = torch.from_numpy(bx).cuda(), torch.from_numpy(cl).cuda(), torch.from_numpy(offs).cuda()

    def encode():
        _, idx, deltas = ops.encode_gt(d_boxes, d_cls, d_offs, a64, C, dense=False)
        return ops.SparseGT(idx, d_boxes, deltas, d_cls, d_offs)
    base = encode()
    lists = {'encoder': (base, torch.zeros(B, ops.ignore_words(A), dtype=torch.int32, device='cuda'))}
    calls = {'encode_gt': encode}
    seen = {}
    for name, m in MATCH.items():
        sgt, bits, overflow = ops.anchor_match(base, a64, *m)
        lists[name] = (sgt, bits)
        pos = [int((sgt.anchor_idx[sgt.offsets[b]:sgt.offsets[b + 1]] < A).sum()) for b in range(B)]
        band = [bin(int(w) & 0xffffffff).count('1') for w in bits.cpu().numpy().reshape(-1)]
        band = np.asarray(band).reshape(B, -1).sum(1) - overflow.cpu().numpy()
        seen[name] = {'positives_per_image': {'mean': float(np.mean(pos)), 'max': int(max(pos))},
                      'band_per_image': {'mean': float(band.mean()), 'max': int(band.max())},
                      'overflow_per_image_max': int(overflow.max()), 'list_entries': int(sgt.anchor_idx.shape[0])}
        calls[f'encode_gt+match_{name}'] = lambda m=m: ops.anchor_match(encode(), a64, *m)
        calls[f'match_{name}'] = lambda m=m: ops.anchor_match(base, a64, *m)
    seen['encoder'] = {'positives_per_image': {'mean': float(np.mean(np.diff(offs))), 'max': int(np.diff(offs).max())},
                       'list_entries': int(base.anchor_idx.shape[0])}
    us = time_alternating(calls, reps)
    rs = np.random.RandomState(3)
    pred = torch.from_numpy((rs.standard_normal((B, A, C + 5)) * 0.5).astype(np.float32)).cuda()
    gmean = torch.ones(1, device='cuda')
    loss_calls = {}
    for name, (sgt, bits) in lists.items():
        _, counts, _ = ops.loss_masked_mean_fwd(pred, sgt, bits, anchors, SIZE, C, WEIGHTS)
        loss_calls[f'loss_masked_fwd_{name}'] = lambda s=sgt, b=bits: ops.loss_masked_mean_fwd(pred, s, b, anchors, SIZE, C, WEIGHTS)
        loss_calls[f'loss_masked_bwd_{name}'] = lambda s=sgt, b=bits, n=counts: ops.loss_masked_mean_bwd(pred, s, b, anchors, n, gmean, SIZE, C, WEIGHTS)
    us.update(time_alternating(loss_calls, reps))
    return {'median_us': us, 'seen': seen}


class _Dataset:
    """Input-sized uint8 images (eight distinct ones, reused) with the boxes of ``synthetic.make_gt_boxes``."""

    def __init__(self, n):
        rs = np.random.RandomState(1)
        self.images = [rs.randint(0, 256, SIZE + (3,), dtype=np.uint8) for _ in range(8)]
        self.n = n
        cls_list, box_list = synthetic.make_gt_boxes(n, SIZE, seed=2)
        self.ann = list(zip(cls_list, box_list))
        from squeezedet_pytorch_amd.augment import KITTI_RGB_MEAN, KITTI_RGB_STD
        self.rgb_mean, self.rgb_std = KITTI_RGB_MEAN, KITTI_RGB_STD

    def __len__(self):
        return self.n

    def load_image(self, i):
        return self.images[i % 8], f'{i:06d}'

    def image_size(self, i):
        return SIZE

    def load_annotations(self, i):
        return np.asarray(self.ann[i][0]).copy(), self.ann[i][1].copy()


def trainer(steps):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, Trainer
    ds = _Dataset(B * steps)
    out = {}
    for name, kw in (('off', {}), ('iou0.5', dict(match_iou=0.5, match_ignore_iou=0.4)), ('iou0.7', dict(match_iou=0.7, match_ignore_iou=0.6))):
        cfg = sqd.make_cfg(device='cuda', batch_size=B, sparse_gt=True, **kw)
        cfg.num_iters, cfg.print_interval, cfg.num_workers = -1, 10 ** 6, 8
        m = SqueezeDetWithLoss(cfg)
        m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234), strict=True)
        m = m.cuda()
        opt = FusedClipSGD(m.parameters(), lr=1e-4, momentum=0.9, weight_decay=1e-4, max_norm=cfg.grad_norm, flat_grad=lambda m=m: m.base.last_grad_flat)
        tr = Trainer(m, opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
        loader = TrainLoader(ds, cfg, seed=1)
        tr.run_epoch('train', 1, loader)                    # warm-up: plans, pinned buffers, caches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = tr.run_epoch('train', 2, loader)
        torch.cuda.synchronize()
        out[name] = {'ms_per_step': 1e3 * (time.perf_counter() - t0) / steps, 'loss': float(stats['loss'])}
    out['steps'], out['batch'] = steps, B
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'anchor_match_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('anchor_match_bench: needs a GPU')
    torch.cuda.set_device(0)
    cfg = sqd.make_cfg(input_size=SIZE)
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'anchors': cfg.num_anchors, 'reps': args.reps,
           'unit': 'us (median, device events behind a spin kernel); trainer: ms per step, wall clock',
           'match': {k: {'match_iou': v[0], 'match_ignore_iou': v[1], 'match_max_extra': v[2]} for k, v in MATCH.items()},
           'kernels': kernels(cfg, args.reps), 'trainer': trainer(args.steps)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
