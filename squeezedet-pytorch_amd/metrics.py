"""Detection AP for any class count (VOC / COCO style), computed on the device (csrc/det_eval.hip, DESIGN.md "Detection AP on the
device").  ``results.kitti_ap`` / ``results.evaluate`` stay the KITTI protocol (three classes, easy / moderate / hard, 41 points);
this module scores everything else:

* ``DetectionAP`` accumulates straight from ``Detector.detect_device``'s packed output and the ground truth that training already
  uploads (``annotations.pack_annotations`` / ``ops.SparseGT``): one match launch per batch, no host synchronisation, no copy;
  ``compute()`` orders the pool (torch stable sorts), runs the AP launch and copies the result out once.  Under a Soft-NMS rule
  (``cfg.nms_mode`` 'linear' / 'gaussian') ``detect_device``'s scores are the decayed ones: those are what the pool is ranked by.
* ``evaluate_results`` takes the host-side result dicts of ``Detector.detect_images`` / ``detect_dataset`` instead.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .annotations import pack_annotations

COCO_THRESHOLDS = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))      # 0.50:0.05:0.95, each the double nearest its decimal


def _mean(values):
    """Plain index-order float64 mean (NaN for an empty list)."""
    s = 0.0
    for v in values:
        s += float(v)
    return s / len(values) if len(values) else float('nan')


class DetectionAP(object):
    """Average precision per class and IoU threshold over a stream of batches.

    ``num_classes`` 1..256; ``iou_thresholds``: 1..16 floats; ``mode``: 'area' (area under the monotone precision envelope, VOC2010+),
    '11point' (VOC2007) or '101point' (COCO).  ``device``: where the pools live (default: the device of the first batch).  Matching
    rule, tie rules and the float64 IoU: ``ops.det_match``.  The pools hold, for every slot of every batch (``B * K`` per update), the
    class (or ``num_classes`` for an empty slot), the score and the per-threshold labels; they grow geometrically on the device."""

    def __init__(self, num_classes, iou_thresholds=(0.5,), mode='area', device=None):
        self.thresholds = tuple(float(t) for t in iou_thresholds)
        ops._check_det_eval_sizes('DetectionAP', len(self.thresholds), num_classes)
        if mode not in ops.AP_MODES:
            raise ValueError(f'DetectionAP: mode must be one of {sorted(ops.AP_MODES)}, got {mode!r}')
        self.num_classes = int(num_classes)
        self.mode = mode
        self.device = torch.device(device) if device is not None else None
        self.reset()

    @classmethod
    def coco(cls, num_classes, device=None):
        """IoU 0.50:0.05:0.95, 101 recall points."""
        return cls(num_classes, COCO_THRESHOLDS, '101point', device)

    @classmethod
    def voc07(cls, num_classes, device=None):
        """IoU 0.5, 11 recall points."""
        return cls(num_classes, (0.5,), '11point', device)

    def reset(self):
        self._n = 0
        self._cls = self._score = self._flags = self._npos = self._thr = None

    def _reserve(self, dev, extra):
        T = len(self.thresholds)
        cap = 0 if self._cls is None else self._cls.shape[0]
        need = self._n + extra
        if need > cap:
            cap = max(2 * cap, need)
            new = (torch.empty(cap, device=dev, dtype=torch.int32), torch.empty(cap, device=dev, dtype=torch.float32),
                   torch.empty(cap, T, device=dev, dtype=torch.uint8))
            if self._n:
                for dst, src in zip(new, (self._cls, self._score, self._flags)):
                    dst[:self._n] = src[:self._n]
            self._cls, self._score, self._flags = new

    def update(self, det, gt_boxes, gt_class_ids, gt_offsets, gt_ignore=None):
        """One batch: ``det`` = the tuple ``Detector.detect_device`` returns, the ground truth as ``annotations.pack_annotations``
        lays it out (device tensors, the coordinate frame of ``det``'s boxes), ``gt_ignore`` uint8 / bool [total] (VOC "difficult",
        COCO "crowd").  One launch and a few device-side copies; nothing waits, nothing leaves the device."""
        if len(det) < 4 or not isinstance(det[2], torch.Tensor):
            raise ValueError('DetectionAP.update: det must be (count, class_ids, scores, boxes, ...)')
        dev = det[2].device
        if self._npos is None:
            self.device = dev
            self._npos = torch.zeros(self.num_classes, device=dev, dtype=torch.int32)
            self._thr = ops.det_thresholds(self.thresholds, dev)
        elif dev != self._npos.device:
            raise ValueError(f'DetectionAP.update: the batch is on {dev}, the pools on {self._npos.device}')
        flags, _, _ = ops.det_match(det, gt_boxes, gt_class_ids, gt_offsets, self._thr, self.num_classes, gt_ignore=gt_ignore,
                                    npos=self._npos)
        B, K, _ = flags.shape
        self._reserve(dev, B * K)
        cls = det[1]
        C = self.num_classes
        empty = (flags[..., 0] == 3) | (cls < 0) | (cls >= C)
        n0, n1 = self._n, self._n + B * K
        self._cls[n0:n1] = torch.where(empty, torch.full_like(cls, C), cls).reshape(-1).to(torch.int32)
        self._score[n0:n1] = det[2].reshape(-1)
        self._flags[n0:n1] = flags.reshape(B * K, -1)
        self._n = n1

    def update_sparse(self, det, sgt):
        """``update`` with the ground truth of an ``ops.SparseGT`` (its ``boxes``, ``class_ids``, ``offsets``: network-input
        coordinates, matching ``detect_device`` without ``scales``)."""
        if not isinstance(sgt, ops.SparseGT):
            raise ValueError('DetectionAP.update_sparse: sgt must be an ops.SparseGT')
        self.update(det, sgt.boxes, sgt.class_ids, sgt.offsets)

    def compute(self):
        """-> {'ap': float64 [C,T] (NaN = class without GT), 'map': float64 [T] (mean over the classes with GT), 'map_all': mean of
        'map', 'npos': int64 [C], 'thresholds': tuple}.  Ordering by (class, score descending, insertion order) with torch stable
        sorts, one AP launch, one device-to-host copy."""
        if self._npos is None:
            raise RuntimeError('DetectionAP.compute: no batch has been added')
        C, T, n = self.num_classes, len(self.thresholds), self._n
        cls, score, flags = self._cls[:n], self._score[:n], self._flags[:n]
        by_score = torch.sort(score, descending=True, stable=True).indices
        by_class = torch.sort(cls[by_score], stable=True)
        perm = by_score[by_class.indices]
        seg = torch.searchsorted(by_class.values, torch.arange(C + 1, device=cls.device, dtype=torch.int32)).to(torch.int32)
        ap, _, _, _ = ops.det_ap(by_class.values, flags[perm], seg, self._npos, self.mode)
        host = torch.cat([ap.reshape(-1), self._npos.to(torch.float64)]).cpu().numpy()       # the one copy
        ap_h = host[:C * T].reshape(C, T).copy()
        npos = host[C * T:].astype(np.int64)
        with_gt = [c for c in range(C) if npos[c] > 0]
        m = np.array([_mean([ap_h[c, t] for c in with_gt]) for t in range(T)], dtype=np.float64)
        return {'ap': ap_h, 'map': m, 'map_all': _mean(m), 'npos': npos, 'thresholds': self.thresholds}


def pack_results(results):
    """Host-side result dicts (``Detector.detect_images`` / ``detect_dataset``: numpy ``class_ids`` / ``scores`` / ``boxes``; an
    image without detections has none of the keys) -> the packed detect form, numpy: (count int32 [B], class_ids int64 [B,K],
    scores fp32 [B,K], boxes fp32 [B,K,4]) with K = the largest count (at least 1); rows past an image's count are zero."""
    if len(results) == 0:
        raise ValueError('pack_results: need at least one image')
    counts = [0 if r.get('scores') is None else int(np.asarray(r['scores']).reshape(-1).shape[0]) for r in results]
    B, K = len(results), max(1, max(counts))
    if K > ops.DET_EVAL_MAX_K:
        raise ValueError(f'pack_results: {K} detections in one image, the limit is {ops.DET_EVAL_MAX_K}')
    cnt = np.asarray(counts, dtype=np.int32)
    cls = np.zeros((B, K), dtype=np.int64)
    sc = np.zeros((B, K), dtype=np.float32)
    bx = np.zeros((B, K, 4), dtype=np.float32)
    for b, (r, n) in enumerate(zip(results, counts)):
        if n == 0:
            continue
        c, s, x = np.asarray(r['class_ids']).reshape(-1), np.asarray(r['scores']).reshape(-1), np.asarray(r['boxes']).reshape(-1, 4)
        if c.shape[0] != n or x.shape[0] != n:
            raise ValueError(f'pack_results: image {b}: {c.shape[0]} class ids, {n} scores, {x.shape[0]} boxes')
        cls[b, :n], sc[b, :n], bx[b, :n] = c, s, x
    return cnt, cls, sc, bx


def evaluate_results(results, class_ids_list, boxes_list, num_classes, iou_thresholds=(0.5,), mode='area', ignore_list=None,
                     device='cuda'):
    """The metric for people who hold host-side results (the ``results.evaluate`` of datasets other than KITTI): ``results`` = the
    per-image dicts of ``Detector.detect_images`` / ``detect_dataset`` (original-image coordinates), ``class_ids_list`` /
    ``boxes_list`` = per image the GT class ids [n_i] and xyxy boxes [n_i,4] in the same coordinates, ``ignore_list`` = per image the
    ignore marks [n_i] or None.  Packs, uploads, and runs the two kernels of ``DetectionAP``; returns what ``compute()`` returns."""
    if len(results) != len(boxes_list):
        raise ValueError(f'evaluate_results: {len(results)} results for {len(boxes_list)} images of ground truth')
    dev = torch.device(device)
    det = tuple(torch.from_numpy(a).to(dev) for a in pack_results(results))
    boxes, cls, offs = pack_annotations(class_ids_list, boxes_list)
    ign = None
    if ignore_list is not None:
        ign = np.concatenate([np.asarray(i).reshape(-1) != 0 for i in ignore_list]).astype(np.uint8) if len(ignore_list) else None
        if ign is None or ign.shape[0] != cls.shape[0]:
            raise ValueError('evaluate_results: ignore_list must hold one mark per GT box')
        ign = torch.from_numpy(ign).to(dev)
    m = DetectionAP(num_classes, iou_thresholds, mode, dev)
    m.update(det, torch.from_numpy(boxes).to(dev), torch.from_numpy(cls).to(dev), torch.from_numpy(offs).to(dev), ign)
    return m.compute()
