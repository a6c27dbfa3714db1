"""Pooled-view inference (DESIGN.md section 3 "Pooled views"): the planner of test-time augmentation and sliced inference.

A VIEW of an image is (zoom, flip, optional source rectangle): one network input canvas that shows the image, its mirror image, another
scale of it, or one tile of a large frame.  The V views of an image go through the backbone as V rows of the batch and meet again in
``ops.detect_views``: one top-k and one suppression per image, in original-image coordinates.  This module turns images and views into

* the packed upload of ``augment.launch_mosaic`` (``pack_layout(..., tiles=B*V)`` / ``write_header``): every image's pixels are stored
  ONCE; an image's unflipped and flipped views read two source rows that share one ``offsets`` value, with ``aug`` = (0, 0, 0) and
  (0, 0, 1); every output canvas is one tile ``(src, top, left, h1, w1, 0, 0, H, W)`` -- the kernel clips the rectangle to the window;
* ``view_xf`` float32 [B*V, 6] = (sy, sx, dy, dx, flip, mirror), computed on the host from the same integers with
  ``boxes.letterbox_meta(size, window, canvas, overhang=True)``: (sy, sx) its scales, (dy, dx) = (-padding_top, -padding_left),
  ``mirror = W0 - 1``.

The window of a view (``view_window``), integers only:

1. the base window (top, left, h1, w1) of the SHOWN extent (hs, ws) -- the whole image (H0, W0), or the source rectangle's (rh, rw) --
   on the canvas (H, W): ``boxes.letterbox_window((hs, ws), (H, W))`` under ``cfg.letterbox``, the whole canvas (0, 0, H, W) under the
   default stretch geometry (``cfg.forbid_resize`` has no window: ValueError);
2. zoom z: ``h1 <- max(1, floor(h1 * z + 0.5))``, ``w1`` likewise (float64, the rounding of ``augment.draw_zoom``), re-centred with floor
   division, ``top = (H - h1) // 2``, ``left = (W - w1) // 2``; z > 1 overhangs the canvas: a centre crop;
3. a source rectangle (ry, rx, rh, rw) in image pixels: the window so far is the RECTANGLE's; the image's window is the one that puts
   the rectangle there, ``H1 = max(1, (H0 * h1 + rh // 2) // rh)``, ``TOP = top - (ry * H1 + H0 // 2) // H0`` and the same in x (a
   flipped view places the mirrored rectangle, ``rx <- W0 - rx - rw``).  With the rectangle's size equal to the canvas the scale is
   exactly 1: the tile is seen at native resolution.  Canvas pixels beside the rectangle show the image around it.

``view_xf`` always comes from the final integers, so it is the inverse of what the input launch rendered, not of what was asked for.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

from .augment import MOSAIC_TILES, MOSAIC_WINDOW_MAX, TILE_INTS, as_u8_image, launch_mosaic, pack_layout, write_header
from .boxes import letterbox_meta, letterbox_window

MAX_ZOOM = 16.0


class View(NamedTuple):
    """One network view of an image: ``zoom`` on the base window, ``flip`` (horizontal mirror), ``rect`` = (ry, rx, rh, rw) source
    rectangle in image pixels or None for the whole image."""
    zoom: float = 1.0
    flip: bool = False
    rect: Optional[Tuple[int, int, int, int]] = None


def check_zooms(who, zooms):
    """``zooms`` as a non-empty tuple of finite floats in (0, MAX_ZOOM]."""
    try:
        z = tuple(float(v) for v in zooms)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: zooms must be a sequence of numbers, got {zooms!r}') from None
    if not z or any(isinstance(v, (bool, np.bool_)) for v in zooms) or not all(np.isfinite(v) and 0. < v <= MAX_ZOOM for v in z):
        raise ValueError(f'{who}: zooms must be a non-empty sequence of finite numbers in (0, {MAX_ZOOM}], got {zooms!r}')
    return z


def tta_views(flip=True, zooms=(1.0,)):
    """The views of test-time augmentation: for every zoom, in order, the image and (``flip``) its mirror image.  The first view of the
    default arguments is the plain image, so ties between views go to it."""
    if not isinstance(flip, (bool, np.bool_)):
        raise ValueError(f'tta_views: flip must be a bool, got {flip!r}')
    out = []
    for z in check_zooms('tta_views', zooms):
        out.append(View(z, False, None))
        if flip:
            out.append(View(z, True, None))
    return out


def _axis_starts(size, tile, overlap):
    if size <= tile:
        return [0]
    stride = tile - overlap
    n = -(-(size - tile) // stride) + 1
    return [min(i * stride, size - tile) for i in range(n)]


def tile_views(orig_size, tile, overlap):
    """The views of sliced inference: a regular grid of ``tile`` = (th, tw) rectangles over a frame of ``orig_size`` = (H0, W0), row by
    row, neighbours ``overlap`` pixels (an int, or (oy, ox)) apart from a full tile step; the last row and column are shifted inward so
    that every tile is full (an axis shorter than the tile has one tile of the axis' length).  Every pixel is covered and neighbouring
    tiles share at least ``overlap`` pixels."""
    H0, W0 = int(orig_size[0]), int(orig_size[1])
    th, tw = int(tile[0]), int(tile[1])
    oy, ox = (int(overlap), int(overlap)) if np.ndim(overlap) == 0 else (int(overlap[0]), int(overlap[1]))
    if H0 < 1 or W0 < 1 or th < 1 or tw < 1 or not (0 <= oy < th and 0 <= ox < tw):
        raise ValueError(f'tile_views: need a non-empty frame and tile and 0 <= overlap < tile, got {orig_size}, {tile}, {overlap}')
    return [View(1.0, False, (y, x, min(th, H0), min(tw, W0))) for y in _axis_starts(H0, th, oy) for x in _axis_starts(W0, tw, ox)]


def view_window(size, view, canvas, letterbox=False):
    """The window (top, left, h1, w1) of ``view`` of an image of ``size`` = (H0, W0) on ``canvas`` = (H, W): the integer rule of the
    module docstring."""
    H0, W0 = int(size[0]), int(size[1])
    H, W = int(canvas[0]), int(canvas[1])
    zoom, flip, rect = view
    zoom = check_zooms('view_window', (zoom,))[0]
    if rect is None:
        ry, rx, rh, rw = 0, 0, H0, W0
    else:
        ry, rx, rh, rw = (int(v) for v in rect)
        if rh < 1 or rw < 1 or ry < 0 or rx < 0 or ry + rh > H0 or rx + rw > W0:
            raise ValueError(f'view_window: rectangle {tuple(rect)} outside the image {(H0, W0)}')
        if flip:
            rx = W0 - rx - rw
    _, _, h1, w1 = letterbox_window((rh, rw), (H, W)) if letterbox else (0, 0, H, W)
    h1 = max(1, int(np.floor(np.float64(h1) * zoom + 0.5)))
    w1 = max(1, int(np.floor(np.float64(w1) * zoom + 0.5)))
    top, left = (H - h1) // 2, (W - w1) // 2
    if rect is not None:
        h1, w1 = max(1, (H0 * h1 + rh // 2) // rh), max(1, (W0 * w1 + rw // 2) // rw)
        top, left = top - (ry * h1 + H0 // 2) // H0, left - (rx * w1 + W0 // 2) // W0
    if h1 > MOSAIC_WINDOW_MAX or w1 > MOSAIC_WINDOW_MAX or abs(top) > MOSAIC_WINDOW_MAX or abs(left) > MOSAIC_WINDOW_MAX:
        raise ValueError(f'view_window: the window {(top, left, h1, w1)} is past the input kernel\'s limit of {MOSAIC_WINDOW_MAX}')
    return top, left, h1, w1


def view_transform(size, window, canvas, flip):
    """One ``view_xf`` row float32 [6] = (sy, sx, dy, dx, flip, mirror) from the final integers."""
    m = letterbox_meta((int(size[0]), int(size[1])), window, canvas, overhang=True)
    return np.array([m['scales'][0], m['scales'][1], -m['padding'][0], -m['padding'][2], 1.0 if flip else 0.0, int(size[1]) - 1],
                    np.float32)


def visible_rect(size, window, canvas, flip=False):
    """The part of the image a view shows, (y0, x0, y1, x1) float64 in original-image pixels (continuous: a box with corners inside it
    lies on the canvas): the canvas cut with the window, taken back through the window's scale and the flip."""
    H0, W0 = int(size[0]), int(size[1])
    top, left, h1, w1 = (int(v) for v in window)
    cy0, cy1 = max(top, 0), min(top + h1, int(canvas[0])) - 1
    cx0, cx1 = max(left, 0), min(left + w1, int(canvas[1])) - 1
    y0, y1 = (cy0 - top) * H0 / h1, min((cy1 - top) * H0 / h1, H0 - 1.0)
    x0, x1 = (cx0 - left) * W0 / w1, min((cx1 - left) * W0 / w1, W0 - 1.0)
    if flip:
        x0, x1 = W0 - 1 - x1, W0 - 1 - x0
    return y0, x0, y1, x1


class ViewPlan(NamedTuple):
    """``plan_views``' result for n images of V views each.  ``sizes`` int32 [n, 2]; ``src_image`` int [S], ``src_aug`` int32 [S, 3]: the
    source rows of the upload (an image's unflipped row, then its flipped row, each only if a view reads it); ``tiles`` int32 [n*V, 4, 9];
    ``windows`` int32 [n*V, 4]; ``view_xf`` float32 [n*V, 6]; ``views``: per image the V views.  Output canvas b*V + v is view v of image b."""
    V: int
    sizes: np.ndarray
    src_image: np.ndarray
    src_aug: np.ndarray
    tiles: np.ndarray
    windows: np.ndarray
    view_xf: np.ndarray
    views: list


def per_image_views(views, n):
    """One list of views for all n images, or one list per image -> the per-image lists."""
    views = list(views)
    if views and isinstance(views[0], View):
        return [views] * n
    per = [list(v) for v in views]
    if len(per) != n:
        raise ValueError(f'views: {len(per)} view lists for {n} images')
    return per


def plan_views(sizes, views, canvas, letterbox=False, forbid_resize=False):
    """``sizes``: (H0, W0) of n images; ``views``: one list of ``View`` for all images, or one list per image (all of the same length V).
    -> ``ViewPlan``."""
    if forbid_resize:
        raise ValueError('plan_views: pooled views place a resize window, forbid_resize (crop_or_pad) has none')
    sizes = np.asarray(sizes, np.int32).reshape(-1, 2)
    n = sizes.shape[0]
    per = per_image_views(views, n)
    V = len(per[0]) if per else 0
    if n < 1 or V < 1 or any(len(p) != V for p in per):
        raise ValueError('plan_views: need at least one image and the same number (>= 1) of views for every image')
    H, W = int(canvas[0]), int(canvas[1])
    src_image, src_aug, row_of = [], [], {}
    for i in range(n):
        for f in (False, True):
            if any(bool(v.flip) == f for v in per[i]):
                row_of[(i, f)] = len(src_image)
                src_image.append(i)
                src_aug.append((0, 0, int(f)))
    tiles = np.full((n * V, MOSAIC_TILES, TILE_INTS), -1, np.int32)
    windows = np.zeros((n * V, 4), np.int32)
    xf = np.zeros((n * V, 6), np.float32)
    for i in range(n):
        for k, v in enumerate(per[i]):
            v = View(float(v[0]), bool(v[1]), v[2])
            win = view_window(sizes[i], v, (H, W), letterbox)
            windows[i * V + k] = win
            tiles[i * V + k, 0] = (row_of[(i, v.flip)],) + win + (0, 0, H, W)
            xf[i * V + k] = view_transform(sizes[i], win, (H, W), v.flip)
    return ViewPlan(V, sizes, np.asarray(src_image, np.int64), np.asarray(src_aug, np.int32).reshape(-1, 3), tiles, windows, xf, per)


def pack_views(images, plan, staging=None):
    """The packed upload of ``plan`` for ``images`` (uint8 [H0, W0, 3]): header (``pack_layout(source sizes, tiles=n*V)``'s size, filled by
    ``write_header``) + every image's pixels once; paired source rows share their offset.  ``staging(nbytes)`` -> uint8 torch tensor to
    fill (default: a fresh numpy buffer).  -> (buffer, header bytes, offsets int64 [S])."""
    ims = [as_u8_image(im, f'pack_views: image {i}') for i, im in enumerate(images)]
    if len(ims) != plan.sizes.shape[0] or any(tuple(im.shape[:2]) != tuple(s) for im, s in zip(ims, plan.sizes)):
        raise ValueError('pack_views: the images are not those the plan was made for')
    src_sizes = plan.sizes[plan.src_image]
    hdr, _, _ = pack_layout([tuple(s) for s in src_sizes], tiles=plan.tiles.shape[0])
    img_off = np.zeros(len(ims), np.int64)
    total = 0
    for i, im in enumerate(ims):
        img_off[i] = total
        total += im.size
    offsets = img_off[plan.src_image]
    buf = np.zeros(hdr + total, np.uint8) if staging is None else staging(hdr + total)
    pk = buf if isinstance(buf, np.ndarray) else buf.numpy()
    pk[:hdr] = 0
    write_header(pk, offsets, src_sizes, plan.src_aug, tiles=plan.tiles)
    for im, off in zip(ims, img_off):
        pk[hdr + off:hdr + off + im.size] = np.ascontiguousarray(im).reshape(-1)
    return buf, hdr, offsets


def render_views(images, plan, canvas, device, rgb_mean, rgb_std, out=None):
    """Upload + ONE mosaic launch: the n*V input canvases fp32 [n*V, 3, H, W] on ``device`` and ``view_xf`` there."""
    import torch
    from .preprocess import _staging
    packed, hdr, _ = pack_views(images, plan, _staging)
    dev = torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    dev_buf = packed.to(dev, non_blocking=True)
    xf = torch.from_numpy(plan.view_xf).to(dev, non_blocking=True)
    BV = plan.tiles.shape[0]
    H, W = int(canvas[0]), int(canvas[1])
    if out is None:
        out = torch.empty(BV, 3, H, W, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (BV, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError('render_views: out must be a contiguous float32 [n*V, 3, H, W] tensor on the device')
    launch_mosaic(dev_buf, BV, len(plan.src_image), hdr, (H, W), out, rgb_mean, rgb_std)
    return out, xf
