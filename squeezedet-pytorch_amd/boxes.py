"""Host-side box utilities the hot path consumes as *inputs*: the anchor grid and the dense
GT tensor.  Mirrors the interface of the reference's ``src/utils/boxes.py`` /
``src/datasets/base.py`` (same names and argument meaning); numpy only.

Reference: ``generate_anchors`` src/utils/boxes.py:37-67, ``compute_deltas`` :84-135,
``boxes_postprocess`` :138-168, ``BaseDataset.prepare_annotations`` src/datasets/base.py:61-76.
"""
from __future__ import annotations

import numpy as np

EPSILON = 1e-10

# KITTI constants (src/datasets/kitti.py:15,26-31)
KITTI_INPUT_SIZE = (384, 1248)
KITTI_ANCHORS_SEED = np.array([[34, 30], [75, 45], [38, 90], [127, 68], [80, 174], [196, 97],
                               [194, 178], [283, 156], [381, 185]], dtype=np.float32)


def generate_anchors(grid_size, input_size, anchors_seed):
    """(grid_h*grid_w*N, 4) float64 anchors ``(cx, cy, w, h)``, ordered (y, x, k).

    Cell centres sit at ``input * (1/(2*grid) + i/grid)``; the expression is evaluated through
    ``linspace`` exactly as the reference does so the float64 values agree bit for bit."""
    anchors_seed = np.asarray(anchors_seed)
    assert anchors_seed.ndim == 2 and anchors_seed.shape[1] == 2
    grid_h, grid_w = grid_size
    in_h, in_w = input_size
    n = anchors_seed.shape[0]
    xs = in_w * (1 / (grid_w * 2) + np.linspace(0, 1, grid_w + 1)[:-1])
    ys = in_h * (1 / (grid_h * 2) + np.linspace(0, 1, grid_h + 1)[:-1])
    a = np.zeros((grid_h, grid_w, n, 4), dtype=np.float64)
    a[:, :, :, 0] = xs.reshape(1, grid_w, 1)
    a[:, :, :, 1] = ys.reshape(grid_h, 1, 1)
    a[:, :, :, 2:] = anchors_seed.reshape(1, 1, n, 2)
    return a.reshape(-1, 4)


def xyxy_to_xywh(boxes_xyxy):
    boxes_xyxy = np.asarray(boxes_xyxy)
    assert boxes_xyxy.ndim == 2
    assert np.all(boxes_xyxy[:, 0] < boxes_xyxy[:, 2]) and np.all(boxes_xyxy[:, 1] < boxes_xyxy[:, 3])
    out = np.empty_like(boxes_xyxy)
    out[:, 0] = (boxes_xyxy[:, 0] + boxes_xyxy[:, 2]) / 2.
    out[:, 1] = (boxes_xyxy[:, 1] + boxes_xyxy[:, 3]) / 2.
    out[:, 2] = boxes_xyxy[:, 2] - boxes_xyxy[:, 0] + 1.
    out[:, 3] = boxes_xyxy[:, 3] - boxes_xyxy[:, 1] + 1.
    return out


def xywh_to_xyxy(boxes_xywh):
    boxes_xywh = np.asarray(boxes_xywh)
    assert boxes_xywh.ndim == 2 and np.all(boxes_xywh > 0)
    half_w = 0.5 * (boxes_xywh[:, 2] - 1)
    half_h = 0.5 * (boxes_xywh[:, 3] - 1)
    return np.stack([boxes_xywh[:, 0] - half_w, boxes_xywh[:, 1] - half_h,
                     boxes_xywh[:, 0] + half_w, boxes_xywh[:, 1] + half_h], axis=1)


def _iou_one_to_many(boxes, box):
    w = np.maximum(np.minimum(boxes[:, 2], box[2]) - np.maximum(boxes[:, 0], box[0]), 0)
    h = np.maximum(np.minimum(boxes[:, 3], box[3]) - np.maximum(boxes[:, 1], box[1]), 0)
    inter = w * h
    union = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]) + \
            (box[2] - box[0]) * (box[3] - box[1]) - inter
    return inter / (union + EPSILON)


def compute_deltas(boxes_xyxy, anchors_xywh):
    """Assign every GT box a *distinct* anchor (best free IoU, else nearest free by squared
    (cx,cy,w,h) distance) and return (deltas float32 [n,4], anchor_indices int32 [n])."""
    boxes_xyxy = np.asarray(boxes_xyxy)
    num_anchors = anchors_xywh.shape[0]
    boxes_xywh = xyxy_to_xywh(boxes_xyxy)
    anchors_xyxy = xywh_to_xyxy(anchors_xywh)
    used = np.zeros(num_anchors, dtype=bool)
    indices = np.empty(boxes_xyxy.shape[0], dtype=np.int32)
    deltas = np.empty((boxes_xyxy.shape[0], 4), dtype=np.float32)
    for i in range(boxes_xyxy.shape[0]):
        iou = _iou_one_to_many(anchors_xyxy, boxes_xyxy[i])
        pick = -1
        for j in np.argsort(-iou):
            if iou[j] <= 0:
                break
            if not used[j]:
                pick = j
                break
        if pick < 0:
            d2 = np.sum((boxes_xywh[i] - anchors_xywh) ** 2, axis=1)
            for j in np.argsort(d2):
                if not used[j]:
                    pick = j
                    break
        used[pick] = True
        indices[i] = pick
        a = anchors_xywh[pick]
        deltas[i] = [(boxes_xywh[i, 0] - a[0]) / a[2], (boxes_xywh[i, 1] - a[1]) / a[3],
                     np.log(boxes_xywh[i, 2] / a[2]), np.log(boxes_xywh[i, 3] / a[3])]
    return deltas, indices


def prepare_annotations(class_ids, boxes, anchors, num_classes):
    """Dense GT ``[A, num_classes + 9]`` = ``[mask, x1,y1,x2,y2, dx,dy,dw,dh, one-hot]``."""
    deltas, anchor_indices = compute_deltas(boxes, anchors)
    gt = np.zeros((anchors.shape[0], num_classes + 9), dtype=np.float32)
    gt[anchor_indices, 0] = 1.
    gt[anchor_indices, 1:5] = boxes
    gt[anchor_indices, 5:9] = deltas
    gt[anchor_indices, 9 + np.asarray(class_ids)] = 1.
    return gt


def boxes_postprocess(boxes, image_meta):
    """Undo, in place, the geometric pre-processing recorded in ``image_meta`` so that ``boxes`` ([n,4] xyxy, network-input
    coordinates) land in original-image coordinates; returns ``boxes``.  Same transforms, order and float arithmetic as
    src/utils/boxes.py:138-168: un-scale (``scales`` = (sy, sx)), un-pad, un-crop (both (top, bottom, left, right)),
    mirror back if ``flipped``, un-drift (``drifts`` = (dy, dx)).  The eval path only ever carries ``scales`` and zero
    ``drifts``; the device path folds that division into the detect kernel."""
    xs, ys = boxes[:, 0::2], boxes[:, 1::2]            # strided views: (x1, x2) and (y1, y2) columns
    if 'scales' in image_meta:
        sy, sx = image_meta['scales'][0], image_meta['scales'][1]
        xs /= sx
        ys /= sy
    for key, sign in (('padding', -1.0), ('crops', 1.0)):
        if key in image_meta:
            top, left = image_meta[key][0], image_meta[key][2]
            xs += sign * left
            ys += sign * top
    if image_meta.get('flipped', False):
        size = image_meta['drifted_size'] if 'drifted_size' in image_meta else image_meta['orig_size']
        extent = boxes[:, 2] - boxes[:, 0] + 1.
        boxes[:, 0] = size[1] - 1 - boxes[:, 2]
        boxes[:, 2] = boxes[:, 0] + extent - 1.
    if 'drifts' in image_meta:
        dy, dx = image_meta['drifts'][0], image_meta['drifts'][1]
        xs += dx
        ys += dy
    return boxes


def pad_crop(size, target):
    """``crop_or_pad``'s integers for one axis (src/utils/image.py:99-115; ``preprocess_padcrop_body`` in csrc/preproc.hip evaluates the
    same): (pad front, pad back, crop front, crop back) -- a smaller image is padded, a larger one centre-cropped, floor half in front."""
    if size < target:
        return (target - size) // 2, (target - size) - (target - size) // 2, 0, 0
    if size > target:
        return 0, 0, (size - target) // 2, (size - target) - (size - target) // 2
    return 0, 0, 0, 0


def letterbox_window(size, canvas):
    """The centred letterbox window of an image of ``size`` = (Hd, Wd) on a ``canvas`` = (H, W): (top, left, h1, w1), the image
    scaled with its aspect ratio kept so that it just fits.  Integers only, the expressions ``preprocess_bilinear_body``
    (csrc/preproc.hip) evaluates in 64 bits: height-limited (``H * Wd <= W * Hd``) ``h1 = H, w1 = max(1, (Wd * H + Hd // 2) // Hd)``,
    else ``w1 = W, h1 = max(1, (Hd * W + Wd // 2) // Wd)``; ``top = (H - h1) // 2``, ``left = (W - w1) // 2``."""
    Hd, Wd = int(size[0]), int(size[1])
    H, W = int(canvas[0]), int(canvas[1])
    if Hd < 1 or Wd < 1 or H < 1 or W < 1:
        raise ValueError(f'letterbox_window: empty image {size} or canvas {canvas}')
    if H * Wd <= W * Hd:
        h1, w1 = H, max(1, (Wd * H + Hd // 2) // Hd)
    else:
        h1, w1 = max(1, (Hd * W + Wd // 2) // Wd), W
    return (H - h1) // 2, (W - w1) // 2, h1, w1


def letterbox_meta(size, window, canvas, overhang=False):
    """The ``image_meta`` entries of an image of ``size`` = (Hd, Wd) letterboxed into ``window`` = (top, left, h1, w1) of ``canvas``:
    ``scales`` float32 [2] = (h1 / Hd, w1 / Wd) (float64 division, then cast), ``padding`` float32 [4] = (top / sy, bottom / sy, left / sx,
    right / sx) -- the padding in original-image pixels, float32 divisions --, ``letterbox`` int32 [4] = the window.  With them
    ``boxes_postprocess`` (divide by ``scales``, then subtract ``padding``) undoes the transform unchanged.  ``overhang``: a mosaic tile's
    window, which may extend past the canvas (the padding on that side is then negative)."""
    top, left, h1, w1 = (int(v) for v in window)
    H, W = int(canvas[0]), int(canvas[1])
    if overhang:
        if h1 < 1 or w1 < 1:
            raise ValueError(f'letterbox_meta: empty window {(top, left, h1, w1)}')
    elif not (1 <= h1 <= H and 1 <= w1 <= W and 0 <= top <= H - h1 and 0 <= left <= W - w1):
        raise ValueError(f'letterbox_meta: window {(top, left, h1, w1)} outside the canvas {(H, W)}')
    scales = np.array([h1 / int(size[0]), w1 / int(size[1])], dtype=np.float32)
    pads = np.array([top, H - h1 - top, left, W - w1 - left], dtype=np.float32)
    return {'scales': scales, 'padding': pads / scales[[0, 0, 1, 1]], 'letterbox': np.array([top, left, h1, w1], np.int32)}


def anchor_ignore_mask(anchors, ign_boxes, overlap):
    """Which anchors of one image lie on an ignore region (KITTI ``DontCare``, VOC ``difficult``, COCO ``crowd``): anchors [A,4]
    (cx,cy,w,h), ign_boxes [n,4] xyxy float32 in network-input coordinates, overlap in (0, 1] -> bool [A].

    Anchor a is ignored iff ``area > 0`` and ``inter >= overlap * area`` for SOME box, with the corners ``compute_deltas`` uses
    (``x0 = cx - 0.5 (w - 1)``, ``x1 = cx + 0.5 (w - 1)``), ``inter`` the intersection with the box and ``area = (x1 - x0) (y1 - y0)``
    the ANCHOR's area: intersection over anchor area, the per-box maximum, not a sum.  (An IoU would never fire for a small anchor
    inside a large region.)  All float64 and no division: ``ops.anchor_ignore_mask`` gives the same bits."""
    overlap = float(overlap)
    if not (overlap > 0.0 and overlap <= 1.0):
        raise ValueError(f'anchor_ignore_mask: overlap must be in (0, 1], got {overlap!r}')
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 4)
    b = np.asarray(ign_boxes, dtype=np.float32).reshape(-1, 4).astype(np.float64)
    x0, y0 = a[:, 0] - 0.5 * (a[:, 2] - 1.0), a[:, 1] - 0.5 * (a[:, 3] - 1.0)
    x1, y1 = a[:, 0] + 0.5 * (a[:, 2] - 1.0), a[:, 1] + 0.5 * (a[:, 3] - 1.0)
    area = (x1 - x0) * (y1 - y0)
    need = overlap * area
    hit = np.zeros(a.shape[0], dtype=bool)
    for bx in b:
        lr = np.maximum(np.minimum(x1, bx[2]) - np.maximum(x0, bx[0]), 0.0)
        tb = np.maximum(np.minimum(y1, bx[3]) - np.maximum(y0, bx[1]), 0.0)
        hit |= lr * tb >= need
    return hit & (area > 0.0)


def check_match_thresholds(name, pos_iou, ign_iou, max_extra):
    """The matcher's arguments: finite floats with ``0 < ign_iou <= pos_iou <= 1`` (``ign_iou`` None: equal to ``pos_iou``, no band) and
    an int ``max_extra >= 0``.  -> (pos_iou, ign_iou, max_extra)."""
    try:
        pos = float(pos_iou)
        ign = pos if ign_iou is None else float(ign_iou)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: match thresholds must be numbers, got {pos_iou!r}, {ign_iou!r}') from None
    if not (0.0 < ign <= pos <= 1.0):                   # (NaN fails)
        raise ValueError(f'{name}: match thresholds must satisfy 0 < ignore <= pos <= 1, got pos {pos_iou!r}, ignore {ign_iou!r}')
    if isinstance(max_extra, (bool, np.bool_)) or not isinstance(max_extra, (int, np.integer)) or max_extra < 0:
        raise ValueError(f'{name}: max_extra must be an int >= 0, got {max_extra!r}')
    return pos, ign, int(max_extra)


def anchor_match(anchors, boxes_list, anchor_idx_list, pos_iou, ign_iou, max_extra, ignore=None):
    """IoU-threshold anchor matching on top of the greedy assignment, the host twin of ``ops.anchor_match`` (DESIGN.md section 3,
    "IoU-threshold matching").  anchors [A,4] (cx,cy,w,h); per image: boxes float32 [n,4] xyxy (the unflagged ones, input order) and
    the encoder's ``anchor_idx`` int [n] for them (the primaries; A = unassigned); ``ignore``: bool [B,A] or None.

    Per image, all overlap arithmetic float64: ``ov(i, j)`` is ``compute_deltas``' overlap (the box area a float32 product, widened
    afterwards; ``inter / (union + 1e-10)``).  For every anchor j that is no primary of the image: ``m = max_i ov(i, j)``, ``i*`` the
    lowest box index attaining it; ``m >= pos_iou``: an extra positive of box ``i*``; else ``m >= ign_iou``: a band anchor; else a
    negative.  An image without boxes has neither; a primary is never re-assigned.  The first ``max_extra`` extras by ascending anchor
    index are kept, the rest are overflow.

    -> (anchor_idx int32 [T], box_idx int64 [T], deltas float32 [T,4], offsets int32 [B+1], ignore bool [B,A], overflow int32 [B]) with
    T = total + B * max_extra and ``offsets[b] = box_offsets[b] + b * max_extra``.  Image b's segment: its primaries in box order, the
    kept extras in ascending anchor order, padding (``anchor_idx`` A, ``box_idx`` -1, zero deltas).  ``box_idx`` indexes the concatenated
    boxes; ``deltas`` are ``compute_deltas``' expression for every entry with an anchor (zero for an unassigned primary); ``ignore`` =
    the given bits | band | overflow."""
    pos_iou, ign_iou, max_extra = check_match_thresholds('anchor_match', pos_iou, ign_iou, max_extra)
    a = np.asarray(anchors, dtype=np.float64).reshape(-1, 4)
    A, B = a.shape[0], len(boxes_list)
    if B == 0 or len(anchor_idx_list) != B:
        raise ValueError('anchor_match: need one box array and one anchor_idx array per image')
    x0, y0 = a[:, 0] - 0.5 * (a[:, 2] - 1.0), a[:, 1] - 0.5 * (a[:, 3] - 1.0)
    x1, y1 = a[:, 0] + 0.5 * (a[:, 2] - 1.0), a[:, 1] + 0.5 * (a[:, 3] - 1.0)
    aarea = (x1 - x0) * (y1 - y0)
    ign_out = np.zeros((B, A), dtype=bool) if ignore is None else np.array(ignore, dtype=bool).reshape(B, A)
    overflow = np.zeros(B, np.int32)
    offsets = np.zeros(B + 1, np.int32)
    idx_out, box_out, delta_out = [], [], []
    first = 0
    for b in range(B):
        bx = np.asarray(boxes_list[b], dtype=np.float32).reshape(-1, 4)
        prim = np.asarray(anchor_idx_list[b]).reshape(-1).astype(np.int64)
        n = bx.shape[0]
        if prim.shape[0] != n:
            raise ValueError(f'anchor_match: image {b}: {prim.shape[0]} anchor indices for {n} boxes')
        barea = ((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])).astype(np.float64)      # float32 product, widened afterwards
        b64 = bx.astype(np.float64)
        m, best = np.full(A, -1.0), np.full(A, -1, np.int64)
        for i in range(n):                              # strict >: ties stay with the lowest box index
            lr = np.maximum(np.minimum(x1, b64[i, 2]) - np.maximum(x0, b64[i, 0]), 0.0)
            tb = np.maximum(np.minimum(y1, b64[i, 3]) - np.maximum(y0, b64[i, 1]), 0.0)
            inter = lr * tb
            ov = inter / ((aarea + barea[i] - inter) + 1e-10)
            better = ov > m
            m[better], best[better] = ov[better], i
        scored = best >= 0
        scored[prim[(prim >= 0) & (prim < A)]] = False
        extra = scored & (m >= pos_iou)
        band = scored & ~extra & (m >= ign_iou)
        ex = np.nonzero(extra)[0]
        kept, over = ex[:max_extra], ex[max_extra:]
        overflow[b] = over.shape[0]
        ign_out[b] |= band
        ign_out[b, over] = True
        seg_idx = np.concatenate([prim, kept, np.full(max_extra - kept.shape[0], A, np.int64)])
        seg_box = np.concatenate([np.arange(n, dtype=np.int64), best[kept], np.full(max_extra - kept.shape[0], -1, np.int64)])
        d = np.zeros((seg_idx.shape[0], 4), np.float32)
        for k in np.nonzero((seg_idx >= 0) & (seg_idx < A) & (seg_box >= 0))[0]:
            q, an = bx[seg_box[k]], a[seg_idx[k]]
            bcx, bcy = (q[0] + q[2]) / np.float32(2), (q[1] + q[3]) / np.float32(2)           # float32, as xyxy_to_xywh
            bw, bh = q[2] - q[0] + np.float32(1), q[3] - q[1] + np.float32(1)
            d[k] = [(np.float64(bcx) - an[0]) / an[2], (np.float64(bcy) - an[1]) / an[3],
                    np.log(np.float64(bw) / an[2]), np.log(np.float64(bh) / an[3])]
        idx_out.append(seg_idx.astype(np.int32))
        box_out.append(np.where(seg_box >= 0, seg_box + first, -1))
        delta_out.append(d)
        first += n
        offsets[b + 1] = offsets[b] + seg_idx.shape[0]
    return np.concatenate(idx_out), np.concatenate(box_out), np.concatenate(delta_out, 0), offsets, ign_out, overflow


def pack_ignore_bits(mask):
    """bool [..., A] -> int32 [..., ceil(A/32)]: anchor a in bit ``a & 31`` of word ``a >> 5`` (the layout of
    ``ops.anchor_ignore_mask``); the bits at and past A are 0."""
    mask = np.asarray(mask, dtype=bool)
    A = mask.shape[-1]
    pad = -A % 32
    m = np.concatenate([mask, np.zeros(mask.shape[:-1] + (pad,), dtype=bool)], -1) if pad else mask
    by = np.packbits(m, axis=-1, bitorder='little')
    return np.ascontiguousarray(by).view('<u4').view(np.int32) if by.size else np.zeros(mask.shape[:-1] + (0,), np.int32)


def unpack_ignore_bits(words, A):
    """int32 [..., ceil(A/32)] -> bool [..., A] (the inverse of ``pack_ignore_bits``)."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.int32)).view(np.uint8)
    return np.unpackbits(w, axis=-1, bitorder='little')[..., :A].astype(bool)
