#!/usr/bin/env python
"""Do two builds give the same rows on every wide-family detect launch?  (A/B of a refactor of csrc/detect_wide.hip against its parent.)

    python tools/detect_bitwise.py > listing.txt        # once in each tree; the two listings must be identical

One line per case: the SHA-256 over (count, and the rows below count of class_ids, scores, boxes, anchor_idx) of every image.  The
grid is seeded: every wide-family ``ops`` function -- detect_wide / filter_dense_wide (C <= 16), detect_many / filter_dense_many,
detect_nms (and its keys_ready form at C <= 16) / filter_dense_nms, detect_views -- x C in {3, 20, 80} x K in {1, 64, 65, 200, 1024}
x A in {37, 16848} x the three modes x agnostic on and off x V in {1, 3} for the views form.  B = 2 images; random anchors on the
384 x 1248 canvas (wide boxes: every candidate overlaps others), every 16th pred row repeated in the next one (exact score ties),
scales and shifts on the pred forms, a mirrored and a half-scale view among the three."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from squeezedet_pytorch_amd import ops  # noqa: E402

SIZE = (384, 1248)
B = 2
CS, KS, AS, VS = (3, 20, 80), (1, 64, 65, 200, 1024), (37, 16848), (1, 3)
RULES = [(m, a) for m in ops.NMS_MODES for a in (False, True)]
NMS, SIGMA = 0.4, 0.5
XF = np.array([[1, 1, 0, 0, 0, 0], [1, 1, 0, 0, 1, SIZE[1] - 1], [0.5, 0.5, 3, -2, 0, 0]], np.float32)


def inputs(C, A, rows, seed):
    rs = np.random.RandomState(seed)
    pred = rs.standard_normal((rows, A, C + 5)).astype(np.float32)
    pred[..., :C] *= 3.0
    pred[..., C] += 1.0
    pred[..., C + 1:] *= 0.3
    pred[:, 1::16] = pred[:, 0:-1:16]
    anc = np.stack([rs.uniform(0, SIZE[1], A), rs.uniform(0, SIZE[0], A), rs.uniform(20, 300, A), rs.uniform(20, 200, A)], 1).astype(np.float32)
    return torch.from_numpy(pred).cuda(), torch.from_numpy(anc).cuda()


def digest(got):
    cnt = got[0].cpu().numpy()
    h = hashlib.sha256(cnt.tobytes())
    for b, n in enumerate(cnt):
        for t in got[1:]:
            h.update(t[b, :int(n)].contiguous().cpu().numpy().tobytes())
    return f'{h.hexdigest()} kept {cnt.tolist()}'


def main():
    if not torch.cuda.is_available():
        raise SystemExit('detect_bitwise: needs a GPU')
    seed = 0
    for C in CS:
        thr = 0.3 if C == 3 else 0.05
        for A in AS:
            seed += 1
            pred, anchors = inputs(C, A, B * max(VS), seed)
            rs = np.random.RandomState(1000 + seed)
            scales = torch.from_numpy((1.0 + rs.uniform(0.1, 0.9, (B, 2))).astype(np.float32)).cuda()
            shifts = torch.from_numpy(rs.randint(-9, 10, (B, 2)).astype(np.float32)).cuda()
            dense = (ops.decode if C <= 16 else ops.decode_many)(pred[:B], anchors, SIZE, C)
            for K in KS:
                tag = f'C{C} A{A} K{K}'
                pk = dict(scales=scales, shifts=shifts)
                hard = [('detect_many', lambda: ops.detect_many(pred[:B], anchors, SIZE, C, K, NMS, thr, **pk)),
                        ('filter_dense_many', lambda: ops.filter_dense_many(*dense, C, K, NMS, thr))]
                if C <= 16:
                    hard += [('detect_wide', lambda: ops.detect_wide(pred[:B], anchors, SIZE, C, K, NMS, thr, **pk)),
                             ('filter_dense_wide', lambda: ops.filter_dense_wide(*dense, C, K, NMS, thr))]
                for name, f in hard:
                    print(f'{name} {tag}: {digest(f())}')
                for mode, agn in RULES:
                    rule = dict(nms_mode=mode, nms_sigma=SIGMA, nms_agnostic=agn)
                    rtag = f'{tag} {mode}{" agnostic" if agn else ""}'
                    ws = torch.zeros(ops.det_workspace_words_wide(B, A, K), device='cuda', dtype=torch.int32)
                    out = ops._det_buffers(B, K, pred.device) + (ws,)
                    print(f'detect_nms {rtag}: {digest(ops.detect_nms(pred[:B], anchors, SIZE, C, K, NMS, thr, out=out, **pk, **rule))}')
                    if C <= 16:
                        out = ops._det_buffers(B, K, pred.device) + (ws,)
                        got = ops.detect_nms(pred[:B], anchors, SIZE, C, K, NMS, thr, out=out, keys_ready=True, **pk, **rule)
                        print(f'detect_nms keys_ready {rtag}: {digest(got)}')
                    print(f'filter_dense_nms {rtag}: {digest(ops.filter_dense_nms(*dense, C, K, NMS, thr, **rule))}')
                    for V in VS:
                        xf = torch.from_numpy(np.tile(XF[:V], (B, 1))).cuda()
                        got = ops.detect_views(pred[:B * V], anchors, SIZE, C, V, xf, K, NMS, thr, **rule)
                        print(f'detect_views V{V} {rtag}: {digest(got)}')
            sys.stdout.flush()


if __name__ == '__main__':
    main()
