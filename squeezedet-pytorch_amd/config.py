"""The ``cfg`` fields the hot path reads, with the reference's defaults.

The reference threads one mutable ``argparse.Namespace`` through every layer
(src/utils/config.py:5-131, src/utils/misc.py:14).  This module does not rebuild its CLI;
it only produces a namespace carrying exactly the fields the model / detector / trainer read
(SURVEY.md section 8b), so the mirrored classes accept either this or the reference's own cfg.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .boxes import KITTI_ANCHORS_SEED, KITTI_INPUT_SIZE, generate_anchors

MAX_CLASSES = 256                # ops.HEAD_MANY_MAX_CLASSES (this module imports no kernels)


def check_geometry(cfg, who):
    """The input geometry of ``cfg``: (letterbox, zoom_out).  ``letterbox`` excludes ``forbid_resize``; ``zoom_out`` is a finite
    amount in [0, 1) and needs ``letterbox``."""
    letterbox = bool(getattr(cfg, 'letterbox', False))
    if letterbox and bool(getattr(cfg, 'forbid_resize', False)):
        raise ValueError(f'{who}: letterbox and forbid_resize are two different input geometries, set one')
    try:
        zoom = float(getattr(cfg, 'zoom_out', 0.))
    except (TypeError, ValueError):
        raise ValueError(f'{who}: zoom_out must be a number in [0, 1), got {getattr(cfg, "zoom_out")!r}') from None
    if not (np.isfinite(zoom) and 0. <= zoom < 1.):
        raise ValueError(f'{who}: zoom_out must be finite and in [0, 1), got {zoom!r}')
    if zoom > 0 and not letterbox:
        raise ValueError(f'{who}: zoom_out shrinks the letterbox window, it needs letterbox=True')
    return letterbox, zoom


def check_mosaic(cfg, who):
    """The mosaic augmentation of ``cfg`` (DESIGN.md 6b "Mosaic"): (mosaic_prob, (lo, hi), mosaic_min_visible).  ``mosaic_prob`` is finite and
    in [0, 1]; ``mosaic_scale`` = (lo, hi) with 0 < lo <= hi <= 2; ``mosaic_min_visible`` in [0, 1].  ``mosaic_prob > 0`` needs ``letterbox=True``
    (which excludes ``forbid_resize``).  A cfg without the fields means off: (0.0, (0.5, 1.0), 0.25)."""
    def number(name, default):
        v = getattr(cfg, name, default)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v):
            raise ValueError(f'{who}: {name} must be a finite number, got {v!r}')
        return float(v)
    prob = number('mosaic_prob', 0.)
    if not 0. <= prob <= 1.:
        raise ValueError(f'{who}: mosaic_prob must be in [0, 1], got {prob!r}')
    scale = getattr(cfg, 'mosaic_scale', (0.5, 1.0))
    try:
        lo, hi = (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: mosaic_scale must be a (lo, hi) pair, got {scale!r}') from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0. < lo <= hi <= 2.):
        raise ValueError(f'{who}: mosaic_scale must satisfy 0 < lo <= hi <= 2, got {scale!r}')
    vis = number('mosaic_min_visible', 0.25)
    if not 0. <= vis <= 1.:
        raise ValueError(f'{who}: mosaic_min_visible must be in [0, 1], got {vis!r}')
    if prob > 0:
        if bool(getattr(cfg, 'forbid_resize', False)):
            raise ValueError(f'{who}: mosaic composes letterbox windows, it excludes forbid_resize')
        if not bool(getattr(cfg, 'letterbox', False)):
            raise ValueError(f'{who}: mosaic composes letterbox windows, it needs letterbox=True')
    return prob, (lo, hi), vis


def check_match(cfg, who):
    """The IoU-threshold matcher of ``cfg`` ("IoU-threshold matching"): None (``match_iou`` None or absent: off),
    or (match_iou, match_ignore_iou, match_max_extra) -- finite floats with ``0 < ignore <= pos <= 1`` (``match_ignore_iou`` None: equal
    to ``match_iou``, no band) and an int ``match_max_extra >= 0`` (default 512).  ``match_iou`` needs ``sparse_gt``: only the sparse loss
    has a masked form.  The other two fields are checked whenever they are there, whether the matcher is on or off."""
    pos = getattr(cfg, 'match_iou', None)
    ign = getattr(cfg, 'match_ignore_iou', None)
    extra = getattr(cfg, 'match_max_extra', 512)

    def number(name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.floating, np.integer)) or not np.isfinite(v):
            raise ValueError(f'{who}: {name} must be a finite number in (0, 1], got {v!r}')
        return float(v)
    if isinstance(extra, (bool, np.bool_)) or not isinstance(extra, (int, np.integer)) or extra < 0:
        raise ValueError(f'{who}: match_max_extra must be an int >= 0, got {extra!r}')
    if ign is not None and not 0. < number('match_ignore_iou', ign) <= 1.:
        raise ValueError(f'{who}: match_ignore_iou must be in (0, 1], got {ign!r}')
    if pos is None:
        if ign is not None:
            raise ValueError(f'{who}: match_ignore_iou is the lower edge of match_iou\'s band, it needs match_iou')
        return None
    pos = number('match_iou', pos)
    ign = pos if ign is None else float(ign)
    if not 0. < ign <= pos <= 1.:
        raise ValueError(f'{who}: the match thresholds must satisfy 0 < match_ignore_iou <= match_iou <= 1, got match_iou {pos!r}, '
                         f'match_ignore_iou {ign!r}')
    if not bool(getattr(cfg, 'sparse_gt', False)):
        raise ValueError(f'{who}: match_iou needs sparse_gt (the band and the overflow leave the loss through the masked launches, '
                         'which the dense loss does not have)')
    return pos, ign, int(extra)


KITTI_CLASS_NAMES = ('Car', 'Pedestrian', 'Cyclist')
BBOX_LOSSES = ('l2', 'iou', 'giou', 'diou', 'ciou')      # ops.BOX_LOSSES


def check_bbox_loss(kind, who):
    """``cfg.bbox_loss``: one of the five names."""
    if not isinstance(kind, str) or kind not in BBOX_LOSSES:
        raise ValueError(f'{who}: bbox_loss must be one of {BBOX_LOSSES}, got {kind!r}')
    return kind


NMS_MODES = ('hard', 'linear', 'gaussian')               # ops.NMS_MODES; the index is the C ABI's nms_mode


def check_nms(cfg, who):
    """The suppression rule of ``cfg``: (nms_mode, nms_sigma, nms_agnostic).  ``nms_mode`` is one of the three names, ``nms_sigma`` a
    finite float > 0 (the Gaussian mode's only reader, checked in every mode), ``nms_agnostic`` a bool.  A cfg without the fields
    (the reference's own namespace) means ('hard', 0.5, False)."""
    mode = getattr(cfg, 'nms_mode', 'hard')
    if not isinstance(mode, str) or mode not in NMS_MODES:
        raise ValueError(f'{who}: nms_mode must be one of {NMS_MODES}, got {mode!r}')
    sigma = getattr(cfg, 'nms_sigma', 0.5)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.floating, np.integer)) or not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f'{who}: nms_sigma must be a finite number > 0, got {sigma!r}')
    agnostic = getattr(cfg, 'nms_agnostic', False)
    if not isinstance(agnostic, (bool, np.bool_)):
        raise ValueError(f'{who}: nms_agnostic must be a bool, got {agnostic!r}')
    return mode, float(sigma), bool(agnostic)


def check_box_vote(cfg, who):
    """``cfg.box_vote_iou`` (DESIGN.md section 3 "Box voting"): None -- or a cfg without the field -- means off; else a finite number in
    (0, 1], not a bool: every detection's box becomes the score-weighted mean of the same-class candidates that overlap it by that IoU.
    -> None or the float."""
    v = getattr(cfg, 'box_vote_iou', None)
    if v is None:
        return None
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.floating, np.integer)) or not (np.isfinite(v) and 0 < v <= 1):
        raise ValueError(f'{who}: box_vote_iou must be None or a finite number in (0, 1], got {v!r}')
    return float(v)


def check_tta(cfg, who):
    """The test-time augmentation of ``cfg`` (DESIGN.md section 3 "Pooled views"): (tta_flip, tta_zooms) -- ``tta_flip`` a bool,
    ``tta_zooms`` None or a non-empty sequence of finite zooms in (0, 16] -- and whether either is set.  A cfg without the fields means
    off.  Set, they are the default ``views`` of ``Detector.detect_images``; pooled views place a resize window, so they exclude
    ``forbid_resize``.  -> (flip, zooms or None, on)."""
    flip = getattr(cfg, 'tta_flip', False)
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError(f'{who}: tta_flip must be a bool, got {flip!r}')
    zooms = getattr(cfg, 'tta_zooms', None)
    if zooms is not None:
        try:
            z = tuple(float(v) for v in zooms)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: tta_zooms must be None or a sequence of numbers, got {zooms!r}') from None
        if not z or any(isinstance(v, (bool, np.bool_)) for v in zooms) or not all(np.isfinite(v) and 0. < v <= 16. for v in z):
            raise ValueError(f'{who}: tta_zooms must be a non-empty sequence of finite numbers in (0, 16], got {zooms!r}')
        zooms = z
    on = bool(flip) or zooms is not None
    if on and bool(getattr(cfg, 'forbid_resize', False)):
        raise ValueError(f'{who}: tta_flip / tta_zooms pool views of a resize window, they exclude forbid_resize')
    return bool(flip), zooms, on


def make_cfg(arch='squeezedet', input_size=KITTI_INPUT_SIZE, anchors_seed=KITTI_ANCHORS_SEED,
             num_classes=3, class_names=None, device='cuda', **overrides):
    """Namespace with the reference's defaults (src/utils/config.py:23-85) plus the
    dataset-derived fields of ``Config.update_dataset_info`` (:121-131).  ``num_classes``: 1 .. 256 (the head kernels' limit: 16
    lanes x 16 registers per anchor row); ``class_names``: one name per class (default: KITTI's three, else 'class0', 'class1', ...)."""
    num_classes = int(num_classes)
    if not 1 <= num_classes <= MAX_CLASSES:
        raise ValueError(f'make_cfg: num_classes must be in 1 .. {MAX_CLASSES}, got {num_classes}')
    if class_names is None:
        class_names = KITTI_CLASS_NAMES if num_classes == len(KITTI_CLASS_NAMES) else tuple(f'class{i}' for i in range(num_classes))
    if len(class_names) != num_classes:
        raise ValueError(f'make_cfg: {len(class_names)} class_names for num_classes = {num_classes} (one name per class, at most {MAX_CLASSES})')
    grid_size = tuple(x // 16 for x in input_size)           # src/datasets/kitti.py:26
    anchors = generate_anchors(grid_size, input_size, np.asarray(anchors_seed))
    cfg = SimpleNamespace(
        mode='eval', arch=arch, dropout_prob=0.5,
        lr=0.01, momentum=0.9, weight_decay=1e-4, grad_norm=5., batch_size=20,
        class_loss_weight=1., positive_score_loss_weight=3.75,
        negative_score_loss_weight=100., bbox_loss_weight=6.,
        bbox_loss='l2',              # the regression term: 'l2' (squared error on the deltas, the reference) or 1 - q of the decoded box against
                                     # the gt box, q = 'iou' | 'giou' | 'diou' | 'ciou' (bbox_loss_weight stays the user's to set)
        nms_thresh=0.4, score_thresh=0.3, keep_top_k=64,
        nms_mode='hard',             # 'hard' (the reference) | 'linear' | 'gaussian': Soft-NMS decays the score of an overlapped box instead of
                                     # deleting it ("NMS modes"); nms_sigma: the Gaussian mode's width
        nms_sigma=0.5,
        nms_agnostic=False,          # True: one suppression group for all classes instead of one per class
        box_vote_iou=None,           # None: off.  A float in (0, 1] (0.5 .. 0.8 are usual): box voting -- every kept box becomes the mean, weighted
                                     # by score, of the same-class candidates overlapping it by that IoU ("Box voting")
        gpus=[0], chunk_sizes=[20], num_iters=-1, print_interval=10, debug=0, num_workers=4, forbid_resize=False,
        flip_prob=0.5, drift_prob=1., seed=42,      # training augmentation (train_data.TrainLoader), src/utils/config.py:53-56
        brightness_jitter=0., contrast_jitter=0., saturation_jitter=0.,      # colour jitter amounts (augment.draw_color); 0 = off
        letterbox=False,             # input geometry: resize with the aspect ratio kept, pad the rest with the whitened mean (excludes forbid_resize)
        zoom_out=0.,                 # training, with letterbox: shrink the window by uniform(1 - zoom_out, 1) and place it at random; 0 = off
        mosaic_prob=0.,              # training, with letterbox: the share of images composed of four sources around a random centre (DESIGN.md 6b
                                     # "Mosaic"); mosaic_scale: each source's zoom on its letterbox window, uniform(lo, hi); mosaic_min_visible:
                                     # a box cut by its tile's rectangle stays a positive while this share of its area is visible
        mosaic_scale=(0.5, 1.0), mosaic_min_visible=0.25,
        sparse_gt=False,             # training ground truth as the list of positives (ops.SparseGT in batch['gt_sparse']) instead of dense
        ignore_overlap=None,         # None: off.  A float in (0, 1] (0.5 is the documented value; needs sparse_gt): anchors covered to that share
                                     # by a flagged box (DontCare / difficult / crowd) leave the loss (batch['gt_ignore'], ops.loss_masked_*)
        match_iou=None,              # None: off (one anchor per box, the reference).  A float in (0, 1] (needs sparse_gt): anchors that overlap a
                                     # box by that IoU are positives too (ops.anchor_match); match_ignore_iou: anchors whose best IoU is in
                                     # [match_ignore_iou, match_iou) leave the loss (None: no band); match_max_extra: extra positives kept per
                                     # image, the rest leave the loss too (batch['gt_match_overflow'] counts them)
        match_ignore_iou=None, match_max_extra=512,
        graph_step=False,            # training: replay the step as one captured hipGraph (trainer.GraphedStep; needs a FusedClipSGD or a
                                     # FusedClipAdamW, one process)
        optimizer='sgd',             # 'sgd' | 'adamw': which fused optimizer trainer.make_train_step builds (FusedClipSGD / FusedClipAdamW)
        ema_decay=0.,                # > 0: the optimizer keeps an exponential moving average of the weights inside its step launch
        ema_warmup=False,            # the EMA's decay starts at min(ema_decay, (1 + n) / (10 + n)) after n averaged steps
        ema_eval=False,              # Trainer.val_epoch runs on the averaged weights (optimizer.averaged_weights())
        tta_flip=False,              # test-time augmentation (DESIGN.md section 3 "Pooled views"; off by default): Detector.detect_images also runs
                                     # the mirror image, and / or the zooms of tta_zooms (None: off; e.g. (1.0, 0.75)), and pools all
                                     # candidates of an image into one top-k and one NMS (views.tta_views); not in the captured lanes
        tta_zooms=None,
        inflight=2,                  # batches in flight on the device in Detector.stream / detect_dataset (lanes.DetectStream)
        input_size=tuple(input_size), num_classes=num_classes, class_names=tuple(class_names),
        anchors=anchors, anchors_per_grid=int(np.asarray(anchors_seed).shape[0]),
        num_anchors=int(anchors.shape[0]), grid_size=grid_size, device=device,
    )
    for k, v in overrides.items():
        setattr(cfg, k, v)
    check_geometry(cfg, 'make_cfg')
    check_mosaic(cfg, 'make_cfg')
    check_bbox_loss(cfg.bbox_loss, 'make_cfg')
    check_nms(cfg, 'make_cfg')
    check_box_vote(cfg, 'make_cfg')
    check_match(cfg, 'make_cfg')
    check_tta(cfg, 'make_cfg')
    return cfg
