#!/usr/bin/env python
"""Golden vectors for the training-phase input pipeline (``augment`` / ``train_data``): the REFERENCE's own
``BaseDataset.preprocess`` in the train phase (src/datasets/base.py:43-59: clip, whiten, drift, flip, then resize or crop_or_pad;
src/utils/image.py:9-124) and ``prepare_annotations`` (:61-76), imported read-only from /root/reference/src through a minimal
``BaseDataset`` subclass and run under ``np.random.seed``.  Build container only; output = data.

``cv2`` is absent here: a stub module stands in, whose ``resize`` is ``oracle.resize_linear_f32`` (the published INTER_LINEAR rule
restated).  The resize branch's bilinear weights therefore stay as unpinned against cv2 itself as they are for the eval path; the
draws, the drift / flip index arithmetic, the boxes, the targets and the whole crop_or_pad branch are the reference's.

Per case: the batch's image sizes and seeds (pixels are regenerated: ``image_of``), boxes and class ids in, the numpy seed, the
draws (dy, dx, flipped), the numpy RNG state after the batch, the transformed boxes, scales / padding / crops, the sparse rows of
the dense gt (and per image whether every anchor pick of the reference was uniquely determined), and the output images: whole
for small targets, for the (384, 1248) target pixel samples at fixed coordinates plus per-channel sums.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augment.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from squeezedet_pytorch_amd import boxes as host_boxes  # noqa: E402  (anchors only)

_cv2 = types.ModuleType("cv2")
_cv2.resize = lambda image, dsize: oracle.resize_linear_f32(image, (dsize[1], dsize[0]))
sys.modules.setdefault("cv2", _cv2)
sys.path.insert(0, "/root/reference/src")
_pkg = types.ModuleType("datasets")                # (a namespace package there; an installed ``datasets`` would shadow it)
_pkg.__path__ = ["/root/reference/src/datasets"]
sys.modules["datasets"] = _pkg
from datasets.base import BaseDataset  # noqa: E402

MEAN = np.array([93.877, 98.801, 95.923], dtype=np.float32).reshape(1, 1, 3)      # src/datasets/kitti.py:17-18
STD = np.array([78.782, 80.130, 81.200], dtype=np.float32).reshape(1, 1, 3)
NUM_CLASSES = 3
# sample coordinates of the full-size outputs (rows, columns): borders, tile edges, interior
SAMPLE_ROWS = np.array([0, 1, 3, 4, 100, 191, 192, 255, 256, 381, 382, 383])
SAMPLE_COLS = np.array([0, 1, 2, 127, 255, 256, 257, 511, 512, 623, 624, 1000, 1023, 1024, 1245, 1246, 1247])

# (numpy seed, [(h, w, image seed, box kind)], input size, drift_prob, flip_prob, forbid_resize)
# box kinds: 'rand' boxes inside the image; 'top' one box with y1 = 0 (randint upper bound 0); 'frac' x1, y1 fractional below 1;
# 'left' a box starting left of the image (clipped to x1 = 0).  (No image without boxes: the reference raises on one.)
CASES = [
    (7, [(375, 1242, 1, 'rand'), (370, 1224, 2, 'top'), (375, 1242, 3, 'frac'), (370, 1224, 4, 'left')], (384, 1248), 1.0, 0.5, False),
    (8, [(375, 1242, 5, 'rand'), (370, 1224, 6, 'frac'), (370, 1224, 7, 'rand')], (384, 1248), 1.0, 0.5, True),
    (9, [(61, 97, 8, 'rand'), (33, 47, 9, 'top'), (40, 29, 10, 'frac'), (120, 200, 11, 'left'), (47, 150, 12, 'rand')], (64, 96), 1.0, 0.5, False),
    (10, [(61, 97, 13, 'rand'), (33, 47, 14, 'frac'), (80, 130, 15, 'left'), (50, 101, 16, 'top')], (64, 96), 1.0, 0.5, True),
    (11, [(61, 97, 17, 'rand'), (52, 83, 18, 'top'), (45, 120, 19, 'rand'), (70, 70, 20, 'frac'), (64, 100, 21, 'rand'),
          (30, 60, 22, 'left')], (64, 96), 0.5, 0.5, False),
    (12, [(61, 97, 23, 'rand'), (52, 83, 24, 'frac'), (45, 120, 25, 'top'), (70, 70, 26, 'rand')], (64, 96), 0.5, 0.5, True),
]


def image_of(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def boxes_of(seed, h, w, kind):
    rs = np.random.RandomState(1000 + seed)
    n = int(rs.randint(2, 6))
    x1 = rs.uniform(w * 0.1, w * 0.7, n); y1 = rs.uniform(h * 0.15, h * 0.6, n)
    bw = rs.uniform(w * 0.05, w * 0.3, n); bh = rs.uniform(h * 0.1, h * 0.35, n)
    b = np.stack([x1, y1, x1 + bw, y1 + bh], 1)
    if kind == 'top':
        b[0, 1] = 0.
    elif kind == 'frac':
        b[0, 0], b[0, 1] = 0.625, 0.375
    elif kind == 'left':
        b[0, 0] = -7.5
    b = b.astype(np.float32)
    cls = rs.randint(0, NUM_CLASSES, n).astype(np.int16)
    return cls, b


class _Cfg:
    def __init__(self, drift_prob, flip_prob, forbid_resize):
        self.drift_prob, self.flip_prob, self.forbid_resize, self.debug = drift_prob, flip_prob, forbid_resize, 0


class _Dataset(BaseDataset):
    """The fields ``preprocess`` / ``prepare_annotations`` read (kitti.py:15-26, config.py:121-131)."""

    def __init__(self, cfg, input_size):
        super().__init__('train', cfg)
        self.input_size = input_size
        self.rgb_mean, self.rgb_std = MEAN, STD
        self.num_classes = NUM_CLASSES
        self.anchors = host_boxes.generate_anchors(tuple(x // 16 for x in input_size), input_size, host_boxes.KITTI_ANCHORS_SEED)
        self.num_anchors = self.anchors.shape[0]


def unique_picks(boxes, anchors):
    """Whether each anchor pick of compute_deltas (src/utils/boxes.py:98-121) was uniquely determined (no free anchor tied with it),
    replayed with the reference's arithmetic on the reference's taken-set sequence (as make_golden_gt.py)."""
    from utils.boxes import compute_overlaps, xywh_to_xyxy, xyxy_to_xywh
    axyxy = xywh_to_xyxy(anchors)
    bxywh = xyxy_to_xywh(boxes)
    taken = np.zeros(anchors.shape[0], bool)
    ok = True
    for i in range(boxes.shape[0]):
        ov = compute_overlaps(axyxy, boxes[i])
        free = ~taken
        best = ov[free].max()
        if best > 0:
            ok &= np.count_nonzero(ov[free] == best) == 1
            pick = np.nonzero(free & (ov == best))[0][0]
        else:
            d = np.sum((bxywh[i] - anchors) ** 2, axis=1)
            ok &= np.count_nonzero(d[free] == d[free].min()) == 1
            pick = np.nonzero(free & (d == d[free].min()))[0][0]
        taken[pick] = True
    return bool(ok)


def main():
    out = {'n': np.array(len(CASES)), 'mean': MEAN.reshape(3), 'std': STD.reshape(3),
           'sample_rows': SAMPLE_ROWS, 'sample_cols': SAMPLE_COLS}
    for c, (seed, imgs, input_size, drift_prob, flip_prob, forbid_resize) in enumerate(CASES):
        ds = _Dataset(_Cfg(drift_prob, flip_prob, forbid_resize), input_size)
        out[f'c{c}_cfg'] = np.array([seed, input_size[0], input_size[1], int(forbid_resize)], np.int64)
        out[f'c{c}_probs'] = np.array([drift_prob, flip_prob], np.float64)
        out[f'c{c}_images'] = np.array([(h, w, s) for h, w, s, _ in imgs], np.int32)
        np.random.seed(seed)
        aug = []
        for k, (h, w, s, kind) in enumerate(imgs):
            cls, boxes = boxes_of(s, h, w, kind)
            out[f'c{c}_i{k}_cls'] = cls; out[f'c{c}_i{k}_boxes_in'] = boxes.copy()
            image = image_of(s, h, w).astype(np.float32)                  # KITTI.load_image: imread(...).astype(np.float32)
            meta = {'index': k, 'image_id': f'{k:06d}', 'orig_size': np.array(image.shape, dtype=np.int32)}
            x, meta, tb = ds.preprocess(image, meta, boxes.copy())
            gt = ds.prepare_annotations(cls, tb)
            assert x.shape == (input_size[0], input_size[1], 3) and x.dtype == np.float32, (x.shape, x.dtype)
            aug.append([int(meta['drifts'][0]), int(meta['drifts'][1]), int(meta['flipped'])])
            assert np.array_equal(meta['drifted_size'][:2], [h - aug[-1][0], w - aug[-1][1]])
            out[f'c{c}_i{k}_boxes_out'] = tb
            if forbid_resize:
                out[f'c{c}_i{k}_padding'] = np.asarray(meta['padding']); out[f'c{c}_i{k}_crops'] = np.asarray(meta['crops'])
            else:
                out[f'c{c}_i{k}_scales'] = np.asarray(meta['scales'])
            rows = np.nonzero(gt[:, 0])[0].astype(np.int32)
            out[f'c{c}_i{k}_gt_idx'] = rows; out[f'c{c}_i{k}_gt_rows'] = gt[rows]
            out[f'c{c}_i{k}_unique'] = np.array(unique_picks(tb, ds.anchors))
            chw = np.ascontiguousarray(x.transpose(2, 0, 1))
            if input_size == (384, 1248):
                out[f'c{c}_i{k}_sample'] = chw[:, SAMPLE_ROWS][:, :, SAMPLE_COLS]
                out[f'c{c}_i{k}_sums'] = chw.astype(np.float64).sum(axis=(1, 2))
            else:
                out[f'c{c}_i{k}_image'] = chw
        st = np.random.get_state()
        out[f'c{c}_aug'] = np.array(aug, np.int32)
        out[f'c{c}_state_key'] = st[1]; out[f'c{c}_state_pos'] = np.array(st[2])
        print(f'case {c}: draws {aug}')
    path = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(path, **out)
    print('wrote augment.npz:', len(CASES), 'cases', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
