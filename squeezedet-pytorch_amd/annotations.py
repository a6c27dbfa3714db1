"""On-device GT encoding.

The reference builds the dense ``gt [A, C+9]`` tensor per image on the CPU inside DataLoader workers
(``BaseDataset.prepare_annotations`` src/datasets/base.py:61-76 -> ``compute_deltas`` src/utils/boxes.py:84-135: a Python
loop over boxes with an ``argsort`` over all 16848 anchors per box) and uploads 0.81 MB of fp32 per image.  Here only
the boxes and class ids are uploaded (a few hundred bytes) and one kernel assigns anchors, computes the regression
targets and writes the dense tensor for the whole batch.

Tie rule: among free anchors with exactly equal overlap (or distance) the LOWEST anchor index wins.  The reference
leaves such ties to ``np.argsort``'s unstable order (numpy-version and CPU dependent); exact ties are common (an
anchor shape lying inside a box has the same IoU at every grid position where it still lies inside).  The host
restatement ``boxes.compute_deltas`` keeps the reference's literal ``np.argsort`` call for anyone who needs the
same-machine behaviour.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

from . import ops

_anchor_cache = {}


def anchors_f64_on(anchors, device):
    """float64 [A,4] device copy of ``cfg.anchors`` (cached per (content hash, device))."""
    a = np.ascontiguousarray(np.asarray(anchors, dtype=np.float64))
    key = (a.shape, hashlib.sha1(a.tobytes()).hexdigest(), str(device))
    t = _anchor_cache.get(key)
    if t is None:
        t = torch.from_numpy(a).to(device)
        _anchor_cache[key] = t
    return t


def pack_annotations(class_ids_list, boxes_list):
    """Per-image lists -> (boxes [total,4] f32, class_ids [total] i32, box_offsets [B+1] i32) numpy, with the
    reference's input checks (xyxy_to_xywh asserts x1 < x2 and y1 < y2, src/utils/boxes.py:13-15)."""
    if len(class_ids_list) != len(boxes_list) or len(boxes_list) == 0:
        raise ValueError('pack_annotations: need one class-id array and one box array per image')
    offs = np.zeros(len(boxes_list) + 1, dtype=np.int32)
    bl, cl = [], []
    for i, (c, b) in enumerate(zip(class_ids_list, boxes_list)):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        c = np.asarray(c).reshape(-1)
        if c.shape[0] != b.shape[0]:
            raise ValueError(f'pack_annotations: image {i}: {c.shape[0]} class ids for {b.shape[0]} boxes')
        assert np.all(b[:, 0] < b[:, 2]) and np.all(b[:, 1] < b[:, 3]), 'boxes must satisfy x1 < x2 and y1 < y2'
        bl.append(b); cl.append(c.astype(np.int32))
        offs[i + 1] = offs[i] + b.shape[0]
    return np.concatenate(bl, 0) if bl else np.zeros((0, 4), np.float32), np.concatenate(cl, 0), offs


def ignore_overlap_of(cfg, who):
    """``cfg.ignore_overlap``: None (off), or a finite float in (0, 1] -- then ``cfg.sparse_gt`` must be set, because only the sparse
    loss has a masked form.  -> the overlap or None."""
    overlap = getattr(cfg, 'ignore_overlap', None)
    if overlap is None:
        return None
    overlap = ops.check_ignore_overlap(f'{who}: cfg.ignore_overlap', overlap)
    if not bool(getattr(cfg, 'sparse_gt', False)):
        raise ValueError(f'{who}: cfg.ignore_overlap needs cfg.sparse_gt (the dense loss has no masked form)')
    return overlap


def split_flagged(ann):
    """One ``dataset.load_annotations(i)`` result, ``(class_ids, boxes)`` or ``(class_ids, boxes, flags)`` (flags bool / uint8 [n],
    nonzero = ignore: KITTI ``DontCare``, VOC ``difficult``, COCO ``crowd``; the meaning of ``DetectionAP.update``'s ``gt_ignore``)
    -> (class ids of the unflagged boxes, unflagged boxes float32 [n,4], flagged boxes float32 [m,4])."""
    cls, boxes = ann[0], np.asarray(ann[1], np.float32).reshape(-1, 4)
    if len(ann) < 3 or ann[2] is None:
        return np.asarray(cls), boxes, np.zeros((0, 4), np.float32)
    cls = np.asarray(cls).reshape(-1)
    flags = np.asarray(ann[2]).reshape(-1) != 0
    if flags.shape[0] != boxes.shape[0] or cls.shape[0] != boxes.shape[0]:
        raise ValueError(f'load_annotations: {cls.shape[0]} class ids and {flags.shape[0]} flags for {boxes.shape[0]} boxes')
    return cls[~flags], boxes[~flags], boxes[flags]


def clip_ignore_boxes(boxes, input_size):
    """Ignore boxes in network-input coordinates clipped to [0, W-1] x [0, H-1]; the ones left without area (x2 <= x1 or y2 <= y1)
    are dropped.  -> float32 [m,4]."""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    H, W = int(input_size[0]), int(input_size[1])
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0., W - 1.)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0., H - 1.)
    return b[(b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1])]


def encode_ignore_boxes(ignore_boxes_list, anchors, overlap, device='cuda'):
    """Per-image lists of ignore boxes (xyxy, network-input coordinates) -> the anchor ignore bitmap int32 [B, ceil(A/32)] on
    ``device`` (``ops.anchor_ignore_mask``)."""
    bl = [np.asarray(b, np.float32).reshape(-1, 4) for b in ignore_boxes_list]
    if not bl:
        raise ValueError('encode_ignore_boxes: need one box array per image')
    offs = np.zeros(len(bl) + 1, dtype=np.int32)
    offs[1:] = np.cumsum([b.shape[0] for b in bl])
    if any(b.shape[0] > 65535 for b in bl):
        raise ValueError('encode_ignore_boxes: at most 65535 ignore boxes per image')
    dev = torch.device(device)
    d_boxes = torch.from_numpy(np.concatenate(bl, 0)).to(dev, non_blocking=True)
    d_offs = torch.from_numpy(offs).to(dev, non_blocking=True)
    return ops.anchor_ignore_mask(d_boxes, d_offs, anchors_f64_on(anchors, dev), overlap)


def encode_annotations(class_ids_list, boxes_list, anchors, num_classes, device='cuda', return_sparse=False, dense=True,
                       ignore_boxes_list=None, ignore_overlap=None, match=None, return_overflow=False):
    """Batch version of ``prepare_annotations``: lists (one entry per image) of class ids [n_i] and xyxy boxes
    [n_i,4] in network-input coordinates -> gt fp32 [B, A, num_classes+9] on ``device``.  With ``return_sparse``
    also returns (anchor_idx [total] i32, deltas [total,4] f32, box_offsets [B+1] i32), all on the device.
    ``dense=False``: -> an ``ops.SparseGT`` (the positives as a list, what ``ops.loss_sparse_*`` consume); the dense
    tensor is neither allocated nor written.  An image may have no boxes, and so may the whole batch (then no encoder launch
    runs and the ``SparseGT`` is empty).  ``ignore_boxes_list`` + ``ignore_overlap`` (both, with ``dense=False``): per-image ignore
    boxes -> (SparseGT, anchor ignore bitmap int32 [B, ceil(A/32)]), the operands of ``ops.loss_masked_*``.  ``match`` = (pos_iou,
    ign_iou, max_extra) (``config.check_match``; with ``dense=False``): the IoU-threshold matcher runs on the encoder's list
    (``ops.anchor_match``) -> (SparseGT with the extra positives, bitmap = band | overflow, ORed onto the region bitmap when both are
    given); ``return_overflow``: also the per-image overflow counts int32 [B] (a device tensor nothing waits on)."""
    if (ignore_boxes_list is None) != (ignore_overlap is None):
        raise ValueError('encode_annotations: ignore_boxes_list and ignore_overlap go together')
    if match is not None:
        if dense:
            raise ValueError('encode_annotations: match needs dense=False (the dense loss has no masked form)')
        from .boxes import check_match_thresholds
        match = check_match_thresholds('encode_annotations', *match)
    elif return_overflow:
        raise ValueError('encode_annotations: return_overflow goes with match')
    if ignore_boxes_list is not None:
        if dense:
            raise ValueError('encode_annotations: ignore regions need dense=False (the dense loss has no masked form)')
        if len(ignore_boxes_list) != len(boxes_list):
            raise ValueError('encode_annotations: need one ignore-box array per image')
        ignore_overlap = ops.check_ignore_overlap('encode_annotations', ignore_overlap)
    boxes, cls, offs = pack_annotations(class_ids_list, boxes_list)
    A = np.asarray(anchors).shape[0]
    if np.any(np.diff(offs) > A):
        raise IndexError('more boxes than anchors in one image')       # the reference indexes gt[num_anchors] here
    if cls.size and (cls.min() < 0 or cls.max() >= num_classes):
        raise IndexError('class id out of range')
    dev = torch.device(device)
    d_boxes = torch.from_numpy(boxes).to(dev, non_blocking=True)
    d_cls = torch.from_numpy(cls).to(dev, non_blocking=True)
    d_offs = torch.from_numpy(offs).to(dev, non_blocking=True)
    if not dense:
        _, idx, deltas = ops.encode_gt(d_boxes, d_cls, d_offs, anchors_f64_on(anchors, dev), num_classes, dense=False)
        sgt = ops.SparseGT(idx, d_boxes, deltas, d_cls, d_offs)
        if match is not None:
            regions = None if ignore_boxes_list is None else encode_ignore_boxes(ignore_boxes_list, anchors, ignore_overlap, dev)
            sgt, ignore, overflow = ops.anchor_match(sgt, anchors_f64_on(anchors, dev), *match, ignore=regions)
            return (sgt, ignore, overflow) if return_overflow else (sgt, ignore)
        if ignore_boxes_list is not None:
            return sgt, encode_ignore_boxes(ignore_boxes_list, anchors, ignore_overlap, dev)
        return sgt
    gt, idx, deltas = ops.encode_gt(d_boxes, d_cls, d_offs, anchors_f64_on(anchors, dev), num_classes)
    if return_sparse:
        return gt, idx, deltas, d_offs
    return gt
