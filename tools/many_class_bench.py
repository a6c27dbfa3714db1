#!/usr/bin/env python
"""The many-class head and the padded ConvDet at KITTI size ("Any class count"), one JSON line on stdout and
in --out.  B = 20, A = 16 848 (24 x 78 x 9):

  head   : for C in {16, 20, 80, 256} the dense decode, the fused detect (K = 64), the loss forward (mean form) and the loss backward
           on the many-class kernels (a 16-lane group per anchor row): median microseconds and achieved GB/s against the pred / gt /
           dpred bytes each launch has to move.  At C = 16 the <= 16-class kernels run on the same operands in the same process,
           alternating: they are the reference there.
  convdet: for 20 and 80 classes ConvDet's forward at its padded width followed by the pack launch, against the same convolution
           alone; the pack and the unpack launch on their own.
  sparse : for C in {3, 20, 80, 256} the dense ground truth against the sparse one (ops.SparseGT, DESIGN.md section 3 "Sparse ground
           truth"): the encoder with and without the dense write, the loss forward (mean form) and the loss backward on the kernels
           that serve C (ops.loss_fns) and on the sparse launches, same operands, alternating in one process.  GB/s of a sparse leg
           is against the sparse launch's own bytes (ops._sparse_fwd_bytes / _sparse_bwd_bytes).

Device events around each call after warm-up.  Nothing here has a pass mark.

    python tools/many_class_bench.py [--reps 100] [--sections head,convdet,sparse] [--out profiles/many_class_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import squeezedet_pytorch_amd as sqd  # noqa: E402
from squeezedet_pytorch_amd import ops  # noqa: E402
from squeezedet_pytorch_amd.model import _ConvParams  # noqa: E402

SIZE = (384, 1248)
B = 20
WEIGHTS = (1.0, 3.75, 100.0, 6.0)


def make_inputs(A, C, anchors, seed=0):
    """pred at the synthetic head's scales with one boosted class logit per anchor; gt with ~40 positives per image."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    pred = torch.randn(B, A, C + 5, device='cuda', generator=g)
    pred[..., :C + 1] *= 2.0
    pred[..., C] -= 2.0
    pred[..., C + 1:] *= 0.4
    boost = torch.randint(0, C, (B, A, 1), device='cuda', generator=g)
    pred.scatter_add_(2, boost, torch.full((B, A, 1), 6.0, device='cuda'))
    gt = torch.zeros(B, A, C + 9, device='cuda')
    rs = np.random.RandomState(seed)
    for b in range(B):
        idx = torch.from_numpy(rs.permutation(A)[:40]).cuda()
        a = anchors[idx]
        gt[b, idx, 0] = 1.0
        gt[b, idx, 1] = (a[:, 0] - a[:, 2] / 2).clamp(0, SIZE[1] - 1)
        gt[b, idx, 2] = (a[:, 1] - a[:, 3] / 2).clamp(0, SIZE[0] - 1)
        gt[b, idx, 3] = (a[:, 0] + a[:, 2] / 2).clamp(0, SIZE[1] - 1)
        gt[b, idx, 4] = (a[:, 1] + a[:, 3] / 2).clamp(0, SIZE[0] - 1)
        gt[b, idx, 5:9] = torch.from_numpy(rs.standard_normal((40, 4)).astype(np.float32) * 0.3).cuda()
        gt[b, idx, 9 + torch.from_numpy(rs.randint(0, C, 40)).cuda()] = 1.0
    return pred.contiguous(), gt


def time_alternating(calls, reps, warmup=10):
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


def head_case(C, A, anchors, reps):
    dev = anchors.device
    pred, gt = make_inputs(A, C, anchors, seed=C)
    gmean = torch.ones(1, device=dev)
    bufs = ops._det_buffers(B, 64, dev, A, 17)                          # (the wide workspace: the many-class detect's)
    _, nobj, _ = ops.loss_mean_fwd_many(pred, gt, anchors, SIZE, C, WEIGHTS)
    calls = {'decode': lambda: ops.decode_many(pred, anchors, SIZE, C),
             'detect': lambda: ops.detect_many(pred, anchors, SIZE, C, 64, 0.4, 0.3, out=bufs),
             'loss_fwd': lambda: ops.loss_mean_fwd_many(pred, gt, anchors, SIZE, C, WEIGHTS),
             'loss_bwd': lambda: ops.loss_mean_bwd_many(pred, gt, anchors, nobj, gmean, SIZE, C, WEIGHTS)}
    if C <= 16:
        nb = ops._det_buffers(B, 64, dev, A)
        calls.update({'narrow_decode': lambda: ops.decode(pred, anchors, SIZE, C),
                      'narrow_detect': lambda: ops.detect(pred, anchors, SIZE, C, 64, 0.4, 0.3, out=nb),
                      'narrow_loss_fwd': lambda: ops.loss_mean_fwd(pred, gt, anchors, SIZE, C, WEIGHTS),
                      'narrow_loss_bwd': lambda: ops.loss_mean_bwd(pred, gt, anchors, nobj, gmean, SIZE, C, WEIGHTS)})
    us = time_alternating(calls, reps)
    rows = B * A
    byts = {'decode': 4.0 * rows * (C + 5 + 7), 'detect': 4.0 * rows * (C + 5), 'loss_fwd': 4.0 * rows * (2 * C + 14),
            'loss_bwd': 4.0 * rows * (3 * C + 19)}
    out = {'kept_per_image': float(bufs[0].float().mean()), 'pred_MB': 4e-6 * rows * (C + 5)}
    for k, v in us.items():
        out[k + '_us'] = v
        out[k + '_GBps'] = byts[k.replace('narrow_', '')] / v * 1e-3
    return out


def sparse_case(C, A, anchors, anchors64, reps):
    dev = anchors.device
    pred, gt = make_inputs(A, C, anchors, seed=C)
    sgt = ops.sparse_gt_from_dense(gt)
    total = int(sgt.anchor_idx.shape[0])
    gmean = torch.ones(1, device=dev)
    _, mean_fwd, _, mean_bwd = ops.loss_fns(C)
    _, nobj, _ = ops.loss_sparse_mean_fwd(pred, sgt, anchors, SIZE, C, WEIGHTS)
    calls = {'encode_dense': lambda: ops.encode_gt(sgt.boxes, sgt.class_ids, sgt.offsets, anchors64, C),
             'encode_sparse': lambda: ops.encode_gt(sgt.boxes, sgt.class_ids, sgt.offsets, anchors64, C, dense=False),
             'loss_fwd_dense': lambda: mean_fwd(pred, gt, anchors, SIZE, C, WEIGHTS),
             'loss_fwd_sparse': lambda: ops.loss_sparse_mean_fwd(pred, sgt, anchors, SIZE, C, WEIGHTS),
             'loss_bwd_dense': lambda: mean_bwd(pred, gt, anchors, nobj, gmean, SIZE, C, WEIGHTS),
             'loss_bwd_sparse': lambda: ops.loss_sparse_mean_bwd(pred, sgt, anchors, nobj, gmean, SIZE, C, WEIGHTS)}
    us = time_alternating(calls, reps)
    rows = B * A
    byts = {'encode_dense': 4.0 * rows * (C + 9), 'loss_fwd_dense': 4.0 * rows * (2 * C + 14), 'loss_bwd_dense': 4.0 * rows * (3 * C + 19),
            'loss_fwd_sparse': ops._sparse_fwd_bytes(B, A, total, C), 'loss_bwd_sparse': ops._sparse_bwd_bytes(B, A, total, C)}
    out = {'positives': total, 'dense_path': ops.head_path(C), 'gt_MB': 4e-6 * rows * (C + 9), 'dpred_MB': 4e-6 * rows * (C + 5)}
    for k, v in us.items():
        out[k + '_us'] = v
        if k in byts:
            out[k + '_GBps'] = byts[k] / v * 1e-3
    return out


def convdet_case(C, reps):
    N, Npad = ops.convdet_width(9, C)
    conv = _ConvParams(768, Npad, 3, padding=1).cuda()
    torch.nn.init.normal_(conv.weight, std=0.002)
    torch.nn.init.zeros_(conv.bias)
    x = torch.randn(B, 24, 78, 768, device='cuda').relu_()
    scratch = torch.empty(B, 24, 78, Npad, device='cuda')
    pred = torch.empty(B, 24, 78, N, device='cuda')
    dpred = torch.randn(B, 24, 78, N, device='cuda')

    def conv_pack():
        conv.run_nhwc(x, out=scratch)
        ops.convdet_pack(scratch, N, out=pred)
    us = time_alternating({'conv_padded_width_alone': lambda: conv.run_nhwc(x, out=scratch), 'conv_plus_pack': conv_pack,
                           'pack': lambda: ops.convdet_pack(scratch, N, out=pred), 'unpack': lambda: ops.convdet_unpack(dpred, Npad)}, reps)
    out = {'N': N, 'Npad': Npad, 'pred_MB': 4e-6 * B * 24 * 78 * N}
    out.update({k + '_us': v for k, v in us.items()})
    out['pack_GBps'] = 8.0 * B * 24 * 78 * N / us['pack'] * 1e-3
    out['unpack_GBps'] = 4.0 * B * 24 * 78 * (N + Npad) / us['unpack'] * 1e-3
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--sections', default='head,convdet,sparse', help='comma-separated subset of head, convdet, sparse')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'many_class_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('many_class_bench: needs a GPU')
    cfg = sqd.make_cfg(input_size=SIZE)
    anchors = torch.from_numpy(cfg.anchors).float().cuda()
    A = cfg.num_anchors
    res = {'batch': B, 'anchors': A, 'reps': args.reps, 'keep_top_k': 64, 'unit': 'us (median, device events); GB/s against the algorithmic bytes'}
    sections = [x for x in args.sections.split(',') if x]
    if not sections or set(sections) - {'head', 'convdet', 'sparse'}:
        raise SystemExit(f'many_class_bench: --sections takes head, convdet, sparse; got {args.sections!r}')
    if 'head' in sections:
        res['head'] = {f'C{C}': head_case(C, A, anchors, args.reps) for C in (16, 20, 80, 256)}
    if 'convdet' in sections:
        res['convdet'] = {f'C{C}': convdet_case(C, args.reps) for C in (20, 80)}
    if 'sparse' in sections:
        anchors64 = torch.from_numpy(np.asarray(cfg.anchors, np.float64)).cuda()
        res['sparse'] = {f'C{C}': sparse_case(C, A, anchors, anchors64, args.reps) for C in (3, 20, 80, 256)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
