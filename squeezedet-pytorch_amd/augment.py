"""Training-time input pipeline: the reference's train-phase ``BaseDataset.preprocess`` (src/datasets/base.py:43-59 with drift and
flip active; src/utils/image.py:22-74 ``drift`` / ``flip``, then ``resize`` :77-88 or ``crop_or_pad`` :91-124) on the GPU.

The random parameters are drawn on the host, in the reference's order and with the reference's arguments
(``draw_augmentation``); the boxes are transformed on the host in float32, op for op as the reference does (``transform_boxes``);
the pixels go up as packed uint8 and ONE launch (``preprocess.launch_u8``: the ``_aug_`` entry of the geometry)
whitens, drifts, flips, resizes (or pads / crops) and transposes the whole batch.  The dense ``gt`` is then encoded on the device
(``annotations.encode_annotations``).

Two departures, both where the reference raises instead: an image without boxes draws its drift with the reference's
``boxes is None`` bound (``max_boxes = max_drift``); an axis whose ``randint`` range is empty (an image under 4 rows or 8 columns)
gets drift 0 on that axis and consumes no draw for it.

Colour jitter (this project's own rule, DESIGN.md 6b "Colour jitter"; off by default): per-image brightness / contrast / saturation
factors (``draw_color``) ride in the header of the same upload; ``launch`` then sums the image's channels on the device
(``sqd_image_stats_u8``, the contrast pivot) and calls the geometry's ``_aug_color_`` entry on the same stream.  The boxes and the geometric draws do not depend on it.

Letterbox and zoom-out (this project's own rule, DESIGN.md 6b "Letterbox and zoom-out"; off by default): the drifted, flipped image
is resized with its aspect ratio kept into a window of the canvas (``boxes.letterbox_window``) and the rest is the whitened mean, 0.
Zoom-out (``draw_zoom``) shrinks that window and places it at random; the window rides in the header of the same upload and the
letterbox launch reads it there.  No box is ever lost.

Mosaic (this project's own rule, DESIGN.md 6b "Mosaic"; off by default, needs letterbox): an output image is a list of up to four tiles,
each a rectangle of the canvas showing part of one source image's letterbox window (``draw_mosaic``, ``mosaic_tiles``, ``one_tile``); the
upload then holds the S source images and a tile block (``pack_layout(..., tiles=B)``), ONE launch of the mosaic entry composes the batch
(``launch_mosaic``), and the boxes are clipped to their tiles and kept, dropped or turned into ignore regions (``transform_boxes_mosaic``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .boxes import letterbox_meta, letterbox_window, pad_crop
from .preprocess import KITTI_RGB_MEAN, KITTI_RGB_STD, _staging, launch_u8

HDR_ALIGN = 256          # the packed pixels start this many bytes into the upload, after the int header


def clip_boxes(boxes, orig_size):
    """``preprocess``' first step (base.py:45-46): a float32 copy of the xyxy boxes clipped to the original image."""
    b = np.array(boxes, dtype=np.float32).reshape(-1, 4)
    orig = np.asarray(orig_size, dtype=np.int32)
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0., orig[1] - 1.)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0., orig[0] - 1.)
    return b


def draw_augmentation(rng, orig_sizes, boxes_list, drift_prob, flip_prob):
    """Per image, in batch order: ``rng.uniform()`` for the drift, then (drift taken) ``rng.randint`` for dy and dx with the
    reference's bounds (image.py:26-33, on the clipped boxes), then ``rng.uniform()`` for the flip (image.py:57).  ``rng`` is a
    ``np.random.RandomState``.  Returns int32 [B, 3] = (dy, dx, flipped)."""
    aug = np.zeros((len(orig_sizes), 3), dtype=np.int32)
    for i, size in enumerate(orig_sizes):
        orig = np.asarray(size, dtype=np.int32)
        if rng.uniform() < drift_prob:
            max_drift_y, max_drift_x = orig[0] // 4, orig[1] // 8
            boxes = None if boxes_list[i] is None else clip_boxes(boxes_list[i], orig)
            if boxes is None or boxes.shape[0] == 0:      # departure: the reference's ``boxes is None`` bound
                max_boxes_y, max_boxes_x = max_drift_y, max_drift_x
            else:
                max_boxes_y, max_boxes_x = min(boxes[:, 1]), min(boxes[:, 0])
            for k, (lo, hi) in enumerate(((-max_drift_y, min(max_drift_y, max_boxes_y)), (-max_drift_x, min(max_drift_x, max_boxes_x)))):
                if int(hi) > int(lo):                     # numpy truncates the float bound; departure: empty range -> 0, no draw
                    aug[i, k] = rng.randint(lo, hi)
        aug[i, 2] = rng.uniform() < flip_prob
    return aug


def draw_color(rng, n, brightness, contrast, saturation):
    """Colour factors of ``n`` images, float32 [n, 3] = (brightness, contrast, saturation).  Per image, in that order, one
    ``rng.uniform(max(0, 1 - d), 1 + d)`` for each axis whose jitter ``d`` is > 0; an axis with ``d == 0`` is 1.0 and draws nothing."""
    ds = [float(brightness), float(contrast), float(saturation)]
    if any(not np.isfinite(d) or d < 0 for d in ds):
        raise ValueError(f'draw_color: jitter amounts must be finite and >= 0, got {ds}')
    color = np.ones((int(n), 3), dtype=np.float32)
    for i in range(int(n)):
        for k, d in enumerate(ds):
            if d > 0:
                color[i, k] = rng.uniform(max(0., 1. - d), 1. + d)
    return color


def draw_zoom(rng, windows, canvas, zoom_out):
    """Zoom-out (the SSD "expand" step) of letterbox ``windows`` int32 [n, 4] = (top, left, h1, w1) on ``canvas`` = (H, W).  Per image, in
    this order: ``z = rng.uniform(1 - zoom_out, 1)``, then ``h1 <- max(1, floor(h1 * z + 0.5))`` and ``w1`` likewise (float64),
    ``top = rng.randint(0, H - h1 + 1)``, ``left = rng.randint(0, W - w1 + 1)``: three draws per image, always.  Returns int32 [n, 4]."""
    d = float(zoom_out)
    if not (np.isfinite(d) and 0. < d < 1.):
        raise ValueError(f'draw_zoom: zoom_out must be finite and in (0, 1), got {zoom_out!r}')
    H, W = int(canvas[0]), int(canvas[1])
    out = np.array(windows, dtype=np.int32).reshape(-1, 4)
    for i in range(out.shape[0]):
        z = rng.uniform(1. - d, 1.)
        h1 = max(1, int(np.floor(np.float64(out[i, 2]) * z + 0.5)))
        w1 = max(1, int(np.floor(np.float64(out[i, 3]) * z + 0.5)))
        if h1 > H or w1 > W:
            raise ValueError(f'draw_zoom: window {out[i].tolist()} is larger than the canvas {(H, W)}')
        out[i] = (rng.randint(0, H - h1 + 1), rng.randint(0, W - w1 + 1), h1, w1)
    return out


MOSAIC_TILES = 4         # tiles of an output image (own image TL, partners TR, BL, BR)
TILE_INTS = 9            # (src, top, left, h1, w1, y0, x0, y1, x1)
MOSAIC_WINDOW_MAX = 65535      # the kernel clamps a tile window's h1, w1 and |top|, |left| there


def draw_mosaic(rng, n, n_dataset, canvas, prob, scale, partner=None, drift_prob=1.0, flip_prob=0.5):
    """The mosaic draws of ``n`` images (a global batch) on ``canvas`` = (H, W), from ``rng`` (the loader's mosaic RandomState).  For every
    image, in batch order and always: ``u = rng.uniform()`` (a mosaic iff ``u < prob``), three ``rng.randint(0, n_dataset)`` partner indices,
    ``cy = rng.randint(H // 4, H - H // 4 + 1)``, ``cx = rng.randint(W // 4, W - W // 4 + 1)``, four ``rng.uniform(lo, hi)`` zooms with
    ``scale`` = (lo, hi): ten draws per image.  After those, for the mosaic images only and in (image, tile) order, the partners' drift
    and flip by ``draw_augmentation`` on the same ``rng``; ``partner(index) -> ((H0, W0), unflagged boxes or None)`` gives what that needs
    (``partner=None``: no such draws, all zero).  Returns a dict: ``'mosaic'`` bool [n], ``'partners'`` int64 [n, 3], ``'centre'`` int32
    [n, 2] = (cy, cx), ``'scale'`` float64 [n, 4] (tile order), ``'aug'`` int32 [n, 3, 3] = the partners' (dy, dx, flipped)."""
    H, W = int(canvas[0]), int(canvas[1])
    lo, hi = float(scale[0]), float(scale[1])
    n = int(n)
    out = {'mosaic': np.zeros(n, bool), 'partners': np.zeros((n, 3), np.int64), 'centre': np.zeros((n, 2), np.int32),
           'scale': np.ones((n, MOSAIC_TILES), np.float64), 'aug': np.zeros((n, 3, 3), np.int32)}
    for i in range(n):
        out['mosaic'][i] = rng.uniform() < prob
        for k in range(3):
            out['partners'][i, k] = rng.randint(0, int(n_dataset))
        out['centre'][i] = (rng.randint(H // 4, H - H // 4 + 1), rng.randint(W // 4, W - W // 4 + 1))
        for k in range(MOSAIC_TILES):
            out['scale'][i, k] = rng.uniform(lo, hi)
    if partner is not None:
        for i in np.flatnonzero(out['mosaic']):
            info = [partner(int(j)) for j in out['partners'][i]]
            out['aug'][i] = draw_augmentation(rng, [s for s, _ in info], [b for _, b in info], drift_prob, flip_prob)
    return out


def one_tile(window, src=0):
    """The tile list int32 [4, 9] of a plain letterbox image: one tile whose rectangle is its ``window`` = (top, left, h1, w1)."""
    top, left, h1, w1 = (int(v) for v in window)
    t = np.full((MOSAIC_TILES, TILE_INTS), -1, np.int32)
    t[0] = (int(src), top, left, h1, w1, top, left, top + h1, left + w1)
    return t


def mosaic_tiles(drifted_sizes, centre, zooms, canvas, src=0):
    """The tile list int32 [4, 9] of one mosaic image (DESIGN.md 6b "Mosaic").  ``drifted_sizes``: (Hd, Wd) of the four sources in tile
    order (own image, then the partners); ``centre`` = (cy, cx); ``zooms``: the four z.  Source t's window is (h, w) of its centred
    ``letterbox_window`` scaled as ``draw_zoom`` rounds, ``h1 = max(1, floor(h * z + 0.5))`` (float64), and placed so that the corner that
    faces the centre touches it: TL (cy - h1, cx - w1), TR (cy - h1, cx), BL (cy, cx - w1), BR (cy, cx).  Its rectangle is quadrant x window x
    canvas; ``src + t`` is its source row.  An empty rectangle stays in the list (the kernel skips it)."""
    H, W = int(canvas[0]), int(canvas[1])
    cy, cx = int(centre[0]), int(centre[1])
    if not (0 <= cy <= H and 0 <= cx <= W):
        raise ValueError(f'mosaic_tiles: centre {(cy, cx)} outside the canvas {(H, W)}')
    quad = ((0, 0, cy, cx), (0, cx, cy, W), (cy, 0, H, cx), (cy, cx, H, W))
    tiles = np.zeros((MOSAIC_TILES, TILE_INTS), np.int32)
    for t in range(MOSAIC_TILES):
        _, _, h, w = letterbox_window(drifted_sizes[t], (H, W))
        h1 = max(1, int(np.floor(np.float64(h) * np.float64(zooms[t]) + 0.5)))
        w1 = max(1, int(np.floor(np.float64(w) * np.float64(zooms[t]) + 0.5)))
        if h1 > MOSAIC_WINDOW_MAX or w1 > MOSAIC_WINDOW_MAX:
            raise ValueError(f'mosaic_tiles: a {(h1, w1)} window is past the kernel\'s limit of {MOSAIC_WINDOW_MAX}')
        top, left = (cy - h1 if t < 2 else cy), (cx - w1 if t % 2 == 0 else cx)
        qy0, qx0, qy1, qx1 = quad[t]
        y0, x0 = max(qy0, top, 0), max(qx0, left, 0)
        y1, x1 = min(qy1, top + h1, H), min(qx1, left + w1, W)
        tiles[t] = (int(src) + t, top, left, h1, w1, y0, x0, max(y1, y0), max(x1, x0))
    return tiles


def check_tiles(tiles, B, S):
    """``tiles`` as int32 [B, 4, 9]; every listed tile must name a source in [0, S), a window within the kernel's limits and a
    rectangle (possibly empty) inside the window and the canvas' non-negative quadrant."""
    t = np.ascontiguousarray(np.asarray(tiles, np.int32))
    if t.size != B * MOSAIC_TILES * TILE_INTS:
        raise ValueError(f'mosaic tiles must be int32 [{B}, {MOSAIC_TILES}, {TILE_INTS}]')
    t = t.reshape(B, MOSAIC_TILES, TILE_INTS)
    for b in range(B):
        for row in t[b]:
            if row[0] < 0:
                break
            s, top, left, h1, w1, y0, x0, y1, x1 = (int(v) for v in row)
            if s >= S or not (1 <= h1 <= MOSAIC_WINDOW_MAX and 1 <= w1 <= MOSAIC_WINDOW_MAX and abs(top) <= MOSAIC_WINDOW_MAX and abs(left) <= MOSAIC_WINDOW_MAX):
                raise ValueError(f'mosaic tile {row.tolist()} of image {b}: source outside [0, {S}) or window past the kernel\'s limits')
            if not (max(top, 0) <= y0 <= y1 <= top + h1 and max(left, 0) <= x0 <= x1 <= left + w1):
                raise ValueError(f'mosaic tile {row.tolist()} of image {b}: the rectangle must lie inside the window')
    return t


def tile_count(tiles):
    """Number of listed tiles of one image's int32 [4, 9] list (``src < 0`` ends it)."""
    neg = np.flatnonzero(np.asarray(tiles)[:, 0] < 0)
    return int(neg[0]) if neg.size else MOSAIC_TILES


def is_plain_tile_list(tiles, canvas):
    """True for the tile list of a plain letterbox image: one tile whose rectangle is its window, inside the canvas."""
    if tile_count(tiles) != 1:
        return False
    _, top, left, h1, w1, y0, x0, y1, x1 = (int(v) for v in tiles[0])
    return (y0, x0, y1, x1) == (top, left, top + h1, left + w1) and top >= 0 and left >= 0 and y1 <= int(canvas[0]) and x1 <= int(canvas[1])


def clip_boxes_to_tile(boxes, rect, min_visible):
    """The mosaic box rule for the transformed boxes float32 [n, 4] (xyxy) of one tile with rectangle ``rect`` = (y0, x0, y1, x1): clip x to
    [x0, x1 - 1] and y to [y0, y1 - 1]; a box is KEPT iff its clipped width (x2 - x1) and height are each >= 2 and its clipped area is >=
    ``min_visible`` times its unclipped area (all float32); it is VISIBLE while its clipped width and height are > 0.  Returns (clipped
    float32 [n, 4], kept bool [n], visible bool [n])."""
    b = np.array(boxes, np.float32).reshape(-1, 4)
    y0, x0, y1, x1 = (int(v) for v in rect)
    c = b.copy()
    c[:, [0, 2]] = np.clip(b[:, [0, 2]], np.float32(x0), np.float32(x1 - 1))
    c[:, [1, 3]] = np.clip(b[:, [1, 3]], np.float32(y0), np.float32(y1 - 1))
    cw, ch = c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    kept = (cw >= 2) & (ch >= 2) & (cw * ch >= np.float32(min_visible) * area)
    return c, kept, (cw > 0) & (ch > 0)


def transform_boxes_mosaic(sources, tiles, input_size, min_visible=0.25, ignore=False):
    """The box half of one mosaic image.  ``sources``: per listed tile, in tile order, (class_ids [n], boxes [n, 4], flagged boxes [m, 4] or
    None, (H0, W0), aug) of that tile's source; ``tiles``: its int32 [4, 9] list.  Each source's boxes go through ``transform_boxes(...,
    letterbox=True, window=tile window)`` unchanged and then through ``clip_boxes_to_tile``: kept boxes become the image's boxes (clipped), in
    tile order; flagged boxes are clipped and kept while visible; with ``ignore`` (``cfg.ignore_overlap`` set) the visible remainder of a
    dropped unflagged box joins them, so that a half-cut object is neither a positive nor a negative.  A tile with an empty rectangle
    contributes nothing.  Returns (class_ids int64 [k], boxes float32 [k, 4], ignore boxes float32 [j, 4], tile 0's meta)."""
    cls, out, ign, meta0 = [], [], [], None
    for k, (c, bx, fl, size, aug) in enumerate(sources):
        _, top, left, h1, w1, y0, x0, y1, x1 = (int(v) for v in tiles[k])
        tb, meta = transform_boxes(bx, size, aug, input_size, False, True, (top, left, h1, w1), overhang=True)
        if k == 0:
            meta0 = meta
        if y1 <= y0 or x1 <= x0:
            continue
        cb, kept, vis = clip_boxes_to_tile(tb, (y0, x0, y1, x1), min_visible)
        out.append(cb[kept])
        cls.append(np.asarray(c, np.int64).reshape(-1)[kept])
        if ignore:
            ign.append(cb[vis & ~kept])
        if fl is not None and len(fl):
            fb, _, fvis = clip_boxes_to_tile(transform_boxes(fl, size, aug, input_size, False, True, (top, left, h1, w1), overhang=True)[0],
                                             (y0, x0, y1, x1), min_visible)
            ign.append(fb[fvis])
    cat = lambda rows, shape, dt: np.concatenate(rows).astype(dt) if rows else np.zeros(shape, dt)      # noqa: E731
    return cat(cls, (0,), np.int64), cat(out, (0, 4), np.float32), cat(ign, (0, 4), np.float32), meta0


def check_window(window, B, canvas):
    """``window`` as int32 [B, 4] = (top, left, h1, w1); every window must lie inside ``canvas``."""
    w = np.ascontiguousarray(np.asarray(window, np.int32)).reshape(-1)
    H, W = int(canvas[0]), int(canvas[1])
    if w.size != 4 * B:
        raise ValueError(f'letterbox windows must be {B} (top, left, h1, w1) rows')
    w = w.reshape(B, 4)
    if np.any(w[:, 2] < 1) or np.any(w[:, 3] < 1) or np.any(w[:, :2] < 0) or np.any(w[:, 0] + w[:, 2] > H) or np.any(w[:, 1] + w[:, 3] > W):
        raise ValueError(f'letterbox windows must lie inside the canvas {(H, W)}')
    return w


def check_color(color, B):
    """``color`` as float32 [B, 3]; the factors must be finite and >= 0."""
    color = np.ascontiguousarray(np.asarray(color, np.float32)).reshape(-1)
    if color.size != 3 * B or not np.all(np.isfinite(color)) or np.any(color < 0):
        raise ValueError(f'colour factors must be {B} finite (brightness, contrast, saturation) triples >= 0')
    return color.reshape(B, 3)


def transform_boxes(boxes, orig_size, aug, input_size, forbid_resize=False, letterbox=False, window=None, overhang=False):
    """The box half of the train-phase ``preprocess`` for one image, in float32 and in the reference's order: clip to the original
    image, subtract the drift, flip with the drifted width, then scale by ``scales`` (or shift by padding / crops).
    ``letterbox``: scale by the window's ``scales`` = (h1 / Hd, w1 / Wd) and move to the window, ``x <- x * sx + left``, ``y <- y * sy + top``;
    ``window`` = (top, left, h1, w1), default the centred ``letterbox_window`` of the drifted size; ``overhang``: the window is a mosaic
    tile's and may extend past the canvas.
    Returns (boxes float32 [n, 4], meta dict of that image: drifts, drifted_size, flipped, scales or padding / crops; letterbox:
    ``letterbox_meta``'s scales, padding, letterbox)."""
    orig = np.asarray(orig_size, dtype=np.int32)
    H0, W0 = int(orig[0]), int(orig[1])
    dy, dx, flipped = int(aug[0]), int(aug[1]), bool(aug[2])
    b = clip_boxes(boxes, orig)
    b[:, [0, 2]] -= dx
    b[:, [1, 3]] -= dy
    Hd, Wd = H0 - dy, W0 - dx
    if flipped:
        widths = b[:, 2] - b[:, 0]
        b[:, 0] = Wd - 1 - b[:, 2]
        b[:, 2] = b[:, 0] + widths
    meta = {'drifts': np.array([dy, dx], np.int32), 'drifted_size': np.array([Hd, Wd, 3], np.int32), 'flipped': flipped}
    H, W = int(input_size[0]), int(input_size[1])
    if letterbox:
        if forbid_resize:
            raise ValueError('transform_boxes: letterbox and forbid_resize are two different input geometries')
        win = letterbox_window((Hd, Wd), (H, W)) if window is None else tuple(int(v) for v in window)
        meta.update(letterbox_meta((Hd, Wd), win, (H, W), overhang))
        b[:, [0, 2]] *= meta['scales'][1]
        b[:, [1, 3]] *= meta['scales'][0]
        b[:, [0, 2]] += np.float32(win[1])
        b[:, [1, 3]] += np.float32(win[0])
        return b, meta
    if not forbid_resize:
        scales = np.array([H / Hd, W / Wd], dtype=np.float32)
        b[:, [0, 2]] *= scales[1]
        b[:, [1, 3]] *= scales[0]
        meta['scales'] = scales
        return b, meta
    pt, pb, ct, cb = pad_crop(Hd, H)
    pl, pr, cl, cr = pad_crop(Wd, W)
    padding, crops = np.array([pt, pb, pl, pr], np.int16), np.array([ct, cb, cl, cr], np.int16)
    if not np.all(padding == 0):
        # as the reference's ``pad`` (image.py:133-137): it rebinds ``padding`` to np.pad's ((top, bottom), (left, right), (0, 0))
        # before shifting, so x moves by (0, 0) and (y1, y2) by (top, bottom) -- reproduced for parity of the training targets
        b[:, [0, 2]] += np.array([0, 0])
        b[:, [1, 3]] += padding[:2]
    if not np.all(crops == 0):
        b[:, [0, 2]] -= crops[2]
        b[:, [1, 3]] -= crops[0]
        b = np.maximum(b, 0.)
    meta.update(padding=padding, crops=crops)
    return b, meta


def batch_meta(metas, sizes, rgb_mean, rgb_std):
    """Per-image meta dicts -> the stacked ``image_meta`` of a batch (the reference's default collate)."""
    B = len(metas)
    out = {'orig_size': np.concatenate([np.asarray(sizes, np.int32).reshape(B, 2), np.full((B, 1), 3, np.int32)], 1),
           'rgb_mean': np.tile(np.asarray(rgb_mean, np.float32).reshape(1, 1, 1, 3), (B, 1, 1, 1)),
           'rgb_std': np.tile(np.asarray(rgb_std, np.float32).reshape(1, 1, 1, 3), (B, 1, 1, 1)),
           'flipped': [m['flipped'] for m in metas]}
    for k in ('drifts', 'drifted_size', 'scales', 'padding', 'crops', 'letterbox'):
        if k in metas[0]:
            out[k] = np.stack([m[k] for m in metas])
    return out


def as_u8_image(im, what):
    """uint8 [H, W, 3] view / copy of ``im``; float pixels must be uint8-representable (the reference's ``skimage`` float32 loads)."""
    im = np.asarray(im)
    if im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
        raise ValueError(f'{what}: expected an [H, W, 3] RGB image, got shape {im.shape}')
    if im.dtype == np.uint8:
        return im
    u8 = im.astype(np.uint8)
    if im.dtype.kind not in 'fiu' or not np.array_equal(u8, im):
        raise ValueError(f'{what}: pixels must be uint8 or uint8-representable values, got {im.dtype} outside 0..255 or fractional')
    return u8


def window_offset(B, color=False):
    """Byte offset of the int32 [B, 4] window block in a ``pack_layout(sizes, color, window=True)`` header."""
    return 28 * B + (12 * B if color else 0)


def tiles_offset(S):
    """Byte offset of the int32 [B, 4, 9] tile block in a ``pack_layout(sizes, ..., tiles=B)`` header of S sources; the colour rows of the B
    output images follow it."""
    return 28 * S


def pack_layout(sizes, color=False, window=False, tiles=None):
    """Byte layout of one upload: int64 offsets [B], int32 sizes [B, 2], int32 aug [B, 3], (``color``: float32 color [B, 3],)
    (``window``: int32 letterbox windows [B, 4],) then (at HDR_ALIGN) the pixels.  Returns (header bytes, pixel offsets int64 [B]
    relative to the pixel base, total bytes).
    ``tiles`` = B, the number of output images of a mosaic upload (DESIGN.md 6b "Mosaic"): ``sizes`` are then the S SOURCE images, the three
    leading blocks have S rows -- what ``ops.image_stats_u8(dev_buf, S, hdr)`` reads --, the int32 tile block [B, 4, 9] follows at
    ``tiles_offset(S)`` and (``color``) the float32 [B, 3] factors of the output images after it; there is no window block."""
    B = len(sizes)
    if tiles is not None:
        if window:
            raise ValueError('pack_layout: a mosaic upload has no window block (the tiles carry the windows)')
        nb = 28 * B + 4 * MOSAIC_TILES * TILE_INTS * int(tiles) + (12 * int(tiles) if color else 0)
    else:
        nb = 8 * B + 20 * B + (12 * B if color else 0) + (16 * B if window else 0)
    hdr = -(-nb // HDR_ALIGN) * HDR_ALIGN
    offsets = np.zeros(B, np.int64)
    total = 0
    for i, (h, w) in enumerate(sizes):
        offsets[i] = total
        total += int(h) * int(w) * 3
    return hdr, offsets, hdr + total


def write_header(buf_np, offsets, sizes, aug, color=None, window=None, tiles=None):
    """Fill the header of a packed upload (``buf_np``: the uint8 numpy view of the whole pinned buffer).  ``color``: float32 [B, 3]
    factors for a ``pack_layout(sizes, color=True)`` layout; ``window``: int32 [B, 4] letterbox windows for a ``window=True`` layout.
    ``tiles``: int32 [B, 4, 9] for a ``pack_layout(sizes, color, tiles=B)`` layout -- ``offsets``, ``sizes`` and ``aug`` are then those of the
    S sources and ``color`` has one row per output image."""
    B = len(offsets)
    buf_np[:8 * B].view(np.int64)[:] = offsets
    buf_np[8 * B:16 * B].view(np.int32)[:] = np.asarray(sizes, np.int32).reshape(-1)
    buf_np[16 * B:28 * B].view(np.int32)[:] = np.asarray(aug, np.int32).reshape(-1)
    if tiles is not None:
        if window is not None:
            raise ValueError('write_header: a mosaic upload has no window block')
        t = np.ascontiguousarray(np.asarray(tiles, np.int32)).reshape(-1, MOSAIC_TILES, TILE_INTS)
        off, nt = tiles_offset(B), t.size * 4
        buf_np[off:off + nt].view(np.int32)[:] = t.reshape(-1)
        if color is not None:
            buf_np[off + nt:off + nt + 12 * t.shape[0]].view(np.float32)[:] = check_color(color, t.shape[0]).reshape(-1)
        return
    if color is not None:
        buf_np[28 * B:40 * B].view(np.float32)[:] = check_color(color, B).reshape(-1)
    if window is not None:
        off = window_offset(B, color is not None)
        buf_np[off:off + 16 * B].view(np.int32)[:] = np.asarray(window, np.int32).reshape(-1)


def launch(dev_buf, B, hdr, input_size, out, forbid_resize, rgb_mean, rgb_std, color=False, sums=None, letterbox=False, window=False):
    """One augmented preprocessing launch on the device copy ``dev_buf`` of a packed upload.  Returns the device tensor the kernel
    writes next to ``out``: scales fp32 [B, 2], or (forbid_resize) padcrop int32 [B, 8], or (letterbox) fp32 [2, B, 2] = (scales, shifts).

    ``letterbox``: the letterbox entry points; ``window``: true when the upload carries the window block (``pack_layout(...,
    window=True)``, written by ``write_header``), false for the kernel's own centred window.

    ``color``: true when the upload has the colour header (``pack_layout(sizes, color=True)``, factors written by ``write_header``).
    The per-image channel sums the contrast pivot needs are then taken on the device first (``sqd_image_stats_u8`` into ``sums``,
    int64 [B, 3, 2] on the device, allocated when not given) and the colour entry point follows on the same stream: no host
    synchronisation, nothing is copied back."""
    H, W = int(input_size[0]), int(input_size[1])
    base, dev = dev_buf.data_ptr(), dev_buf.device
    p = lambda off: ctypes.c_void_p(base + off)      # noqa: E731
    if letterbox and forbid_resize:
        raise ValueError('launch: letterbox and forbid_resize are two different input geometries')
    if color and hdr < 40 * B:
        raise ValueError(f'launch: a header of {hdr} bytes has no room for the colour factors of {B} images')
    if window and (not letterbox or hdr < window_offset(B, color) + 16 * B):
        raise ValueError(f'launch: a header of {hdr} bytes has no room for the letterbox windows of {B} images (or letterbox is off)')
    blocks = {}
    if color:
        from .ops import image_stats_u8
        blocks.update(color=p(28 * B), sums=image_stats_u8(dev_buf, B, hdr, out=sums))
    if letterbox:
        side = torch.empty(2, B, 2, device=dev, dtype=torch.float32)
        blocks.update(win=p(window_offset(B, color)) if window else None, scales=side[0], shifts=side[1])
    elif forbid_resize:
        side = torch.empty(B, 8, device=dev, dtype=torch.int32)
        blocks.update(padcrop=side)
    else:
        side = torch.empty(B, 2, device=dev, dtype=torch.float32)
        blocks.update(scales=side)
    launch_u8('letterbox' if letterbox else 'padcrop' if forbid_resize else 'resize', p(hdr), p(0), p(8 * B), out, B, H, W, rgb_mean, rgb_std,
              dev, aug=p(16 * B), **blocks)
    return side


def launch_mosaic(dev_buf, B, S, hdr, input_size, out, rgb_mean, rgb_std, color=False, sums=None):
    """The mosaic launch on the device copy ``dev_buf`` of a ``pack_layout(sizes, color, tiles=B)`` upload of S sources: B output images
    into ``out``.  ``color``: the upload carries the output images' factors; the channel sums of the S sources are then taken on the device
    first (``sqd_image_stats_u8`` into ``sums``, int64 [S, 3, 2], allocated when not given), as ``launch`` does.  No side outputs."""
    H, W = int(input_size[0]), int(input_size[1])
    B, S = int(B), int(S)
    base, dev = dev_buf.data_ptr(), dev_buf.device
    p = lambda off: ctypes.c_void_p(base + off)      # noqa: E731
    need = tiles_offset(S) + 4 * MOSAIC_TILES * TILE_INTS * B + (12 * B if color else 0)
    if not 1 <= S <= MOSAIC_TILES * B or hdr < need:
        raise ValueError(f'launch_mosaic: {S} sources for {B} images, or a header of {hdr} bytes without room for {need}')
    blocks = {}
    if color:
        from .ops import image_stats_u8
        blocks.update(color=p(tiles_offset(S) + 4 * MOSAIC_TILES * TILE_INTS * B), sums=image_stats_u8(dev_buf, S, hdr, out=sums))
    launch_u8('mosaic', p(hdr), p(0), p(8 * S), out, B, H, W, rgb_mean, rgb_std, dev, aug=p(16 * S), tiles=p(tiles_offset(S)), S=S, **blocks)


def check_out(out, B, H, W, device):
    if out is None:
        return torch.empty(B, 3, H, W, device=device, dtype=torch.float32)
    if tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError('preprocess_train_batch: out must be a contiguous float32 [B, 3, H, W] tensor on the device')
    return out


def _default_anchors(input_size):
    from .boxes import KITTI_ANCHORS_SEED, generate_anchors
    return generate_anchors(tuple(x // 16 for x in input_size), tuple(input_size), np.asarray(KITTI_ANCHORS_SEED))


def preprocess_train_batch(images, class_ids_list, boxes_list, input_size, rng, drift_prob=1.0, flip_prob=0.5,
                           rgb_mean=KITTI_RGB_MEAN, rgb_std=KITTI_RGB_STD, forbid_resize=False, device='cuda', out=None,
                           anchors=None, num_classes=3, aug=None, color_jitter=(0., 0., 0.), color=None, letterbox=False, window=None,
                           tiles=None, sources=None, mosaic_min_visible=0.25):
    """A training batch the reference's way (``BaseDataset.__getitem__`` in the train phase + default collate), built on the GPU.

    images: list of uint8 (or uint8-representable float) [H0, W0, 3] RGB arrays; class_ids_list / boxes_list: per image [n] and
    xyxy [n, 4] in original-image coordinates; rng: ``np.random.RandomState`` the draws come from (``aug``: int32 [B, 3] to use
    instead of drawing); color_jitter: (brightness, contrast, saturation) amounts, any > 0 draws the colour factors from ``rng`` after
    the geometric draws of the whole batch (``draw_color``); color: float32 [B, 3] factors to use instead of drawing (``image_meta``
    then carries them as ``'color'``); letterbox: the letterbox geometry (``image_meta`` then carries ``letterbox_meta``'s keys), with
    ``window``: int32 [B, 4] windows to use (default: the centred ones; ``draw_zoom`` makes zoomed-out ones); anchors: ``cfg.anchors`` (default: the KITTI anchors of ``input_size``).  Returns (image fp32 NCHW on
    ``device`` -- ``out`` when given --, image_meta with the reference's keys, dense gt [B, A, num_classes + 9] on ``device``).
    Uploads: one packed uint8 buffer (int header included) and the boxes of ``encode_annotations``; nothing waits on the device.

    Mosaic (DESIGN.md 6b "Mosaic"; needs ``letterbox=True``): ``tiles`` int32 [B, 4, 9] composes B output images from the S = len(images)
    SOURCE images given -- ``class_ids_list``, ``boxes_list`` and ``aug`` are per source, ``color`` per output image, ``window`` is not
    taken (the tiles carry the windows).  An image whose list is one tile with rectangle == window inside the canvas is a plain letterbox
    image and keeps all its boxes; every other image follows ``transform_boxes_mosaic`` with ``mosaic_min_visible`` (no fallback here: the
    tiles given are used as they are).  ``sources``: int [B, 4] labels of the tiles' sources (dataset indices, -1 unused) recorded as
    ``image_meta['mosaic_index']``, default the tiles' own source rows; ``image_meta['mosaic']`` is the tile block and the other keys are
    those of each image's tile 0."""
    B = len(images)
    if B == 0:
        raise ValueError('preprocess_train_batch: empty batch')
    if tiles is not None:
        if not letterbox or forbid_resize or window is not None:
            raise ValueError('preprocess_train_batch: tiles needs letterbox=True and takes no window')
        return _mosaic_train_batch(images, class_ids_list, boxes_list, input_size, rng, drift_prob, flip_prob, rgb_mean, rgb_std, device, out,
                                   anchors, num_classes, aug, color_jitter, color, tiles, sources, mosaic_min_visible)
    if sources is not None:
        raise ValueError('preprocess_train_batch: sources goes with tiles')
    H, W = int(input_size[0]), int(input_size[1])
    ims = [as_u8_image(im, f'preprocess_train_batch: image {i}') for i, im in enumerate(images)]
    sizes = [im.shape[:2] for im in ims]
    if aug is None:
        aug = draw_augmentation(rng, sizes, boxes_list, drift_prob, flip_prob)
    aug = np.asarray(aug, np.int32).reshape(B, 3)
    if color is not None:
        color = check_color(color, B)
    elif any(float(d) > 0 for d in color_jitter):
        color = draw_color(rng, B, *color_jitter)
    if letterbox:
        if window is not None:
            window = check_window(window, B, (H, W))
        else:
            window = np.array([letterbox_window((h - int(a[0]), w - int(a[1])), (H, W)) for (h, w), a in zip(sizes, aug)], np.int32)
    elif window is not None:
        raise ValueError('preprocess_train_batch: window needs letterbox=True')
    wins = window if letterbox else [None] * B
    tb, metas = zip(*[transform_boxes(bx, (h, w), a, input_size, forbid_resize, letterbox, wn)
                      for bx, (h, w), a, wn in zip(boxes_list, sizes, aug, wins)])
    hdr, offsets, total = pack_layout(sizes, color is not None, letterbox)
    packed = _staging(total)
    pk = packed.numpy()
    write_header(pk, offsets, sizes, aug, color, window)
    for im, off in zip(ims, offsets):
        pk[hdr + off:hdr + off + im.size] = np.ascontiguousarray(im).reshape(-1)
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    dev_buf = packed.to(dev, non_blocking=True)
    out = check_out(out, B, H, W, dev)
    launch(dev_buf, B, hdr, input_size, out, forbid_resize, rgb_mean, rgb_std, color=color is not None, letterbox=letterbox, window=letterbox)
    from .annotations import encode_annotations
    gt = encode_annotations(class_ids_list, list(tb), _default_anchors(input_size) if anchors is None else anchors, num_classes, device=dev)
    meta = batch_meta(metas, sizes, rgb_mean, rgb_std)
    if color is not None:
        meta['color'] = color
    return out, meta, gt


def mosaic_boxes(tiles, per_source, input_size, min_visible, ignore=False):
    """The boxes of B output images from their tile block int32 [B, 4, 9]; ``per_source[s]`` = (class_ids, boxes, flagged boxes or None, (H0,
    W0), aug) of source s.  A plain one-tile image (``is_plain_tile_list``) takes the letterbox path of ``transform_boxes`` and keeps every
    box (its flagged boxes ``annotations.clip_ignore_boxes``); the others ``transform_boxes_mosaic``.  Returns per image lists (class_ids,
    boxes, ignore boxes, tile 0's meta)."""
    from .annotations import clip_ignore_boxes
    cls, out, ign, metas = [], [], [], []
    for t in tiles:
        n = tile_count(t)
        if n == 0:
            raise ValueError('mosaic_boxes: an output image needs at least one tile')
        if is_plain_tile_list(t, input_size):
            c, bx, fl, size, a = per_source[int(t[0, 0])]
            tb, meta = transform_boxes(bx, size, a, input_size, False, True, t[0, 1:5])
            fb = np.zeros((0, 4), np.float32) if fl is None or not len(fl) else transform_boxes(fl, size, a, input_size, False, True, t[0, 1:5])[0]
            c, fb = np.asarray(c), clip_ignore_boxes(fb, input_size)
        else:
            c, tb, fb, meta = transform_boxes_mosaic([per_source[int(s)] for s in t[:n, 0]], t, input_size, min_visible, ignore)
        cls.append(c); out.append(tb); ign.append(fb); metas.append(meta)
    return cls, out, ign, metas


def _mosaic_train_batch(images, class_ids_list, boxes_list, input_size, rng, drift_prob, flip_prob, rgb_mean, rgb_std, device, out, anchors,
                        num_classes, aug, color_jitter, color, tiles, sources, min_visible):
    """``preprocess_train_batch`` with ``tiles=``: S source images -> B output images in one mosaic launch."""
    S = len(images)
    H, W = int(input_size[0]), int(input_size[1])
    ims = [as_u8_image(im, f'preprocess_train_batch: image {i}') for i, im in enumerate(images)]
    sizes = [im.shape[:2] for im in ims]
    tiles = np.asarray(tiles, np.int32)
    if tiles.ndim != 3:
        raise ValueError('preprocess_train_batch: tiles must be int32 [B, 4, 9]')
    B = tiles.shape[0]
    tiles = check_tiles(tiles, B, S)
    if not 1 <= S <= MOSAIC_TILES * B:
        raise ValueError(f'preprocess_train_batch: {S} source images for {B} output images (at most {MOSAIC_TILES} each)')
    if aug is None:
        aug = draw_augmentation(rng, sizes, boxes_list, drift_prob, flip_prob)
    aug = np.asarray(aug, np.int32).reshape(S, 3)
    if color is not None:
        color = check_color(color, B)
    elif any(float(d) > 0 for d in color_jitter):
        color = draw_color(rng, B, *color_jitter)
    per_source = [(c, bx, None, s, a) for c, bx, s, a in zip(class_ids_list, boxes_list, sizes, aug)]
    cls, tb, _ign, metas = mosaic_boxes(tiles, per_source, input_size, min_visible)
    hdr, offsets, total = pack_layout(sizes, color is not None, tiles=B)
    packed = _staging(total)
    pk = packed.numpy()
    write_header(pk, offsets, sizes, aug, color, tiles=tiles)
    for im, off in zip(ims, offsets):
        pk[hdr + off:hdr + off + im.size] = np.ascontiguousarray(im).reshape(-1)
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    dev_buf = packed.to(dev, non_blocking=True)
    out = check_out(out, B, H, W, dev)
    launch_mosaic(dev_buf, B, S, hdr, input_size, out, rgb_mean, rgb_std, color=color is not None)
    from .annotations import encode_annotations
    gt = encode_annotations(cls, tb, _default_anchors(input_size) if anchors is None else anchors, num_classes, device=dev)
    meta = batch_meta(metas, [sizes[int(t[0, 0])] for t in tiles], rgb_mean, rgb_std)
    meta['mosaic'] = tiles
    meta['mosaic_index'] = np.where(tiles[:, :, 0] >= 0, tiles[:, :, 0], -1).astype(np.int64) if sources is None \
        else np.asarray(sources, np.int64).reshape(B, MOSAIC_TILES)
    if color is not None:
        meta['color'] = color
    return out, meta, gt
