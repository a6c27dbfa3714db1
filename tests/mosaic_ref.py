"""Plain numpy restatement of the mosaic rule ("Mosaic"): the yardstick of tests/test_mosaic_host.py and
tests/test_mosaic_gpu.py.  No project code is involved (tests/letterbox_ref.py and tests/color_jitter_ref.py are yardsticks themselves).

An output image is a list of at most 4 tiles (src, top, left, h1, w1, y0, x0, y1, x1); ``src < 0`` ends the list.  Per tile,
V = drift_flip(whiten(source)), full = oracle.resize_linear_f32(V, (h1, w1)), and full[y0 - top:y1 - top, x0 - left:x1 - left] is pasted
into a zero canvas at the rectangle -- where no earlier tile of the list has pasted.  Colour: the source goes through
color_jitter_ref.jitter with the OUTPUT image's factors and its OWN pivot before the whitening.

The kernel's clamp (``clamp_tiles``): src to S - 1, h1 / w1 to 1..65535, top / left to -65535..65535, the rectangle into canvas and
window.  The tile rule (``tiles_of``) and the box rule (``boxes_of``) are restated as plain loops over Python numbers."""
import math

import numpy as np

import oracle

import color_jitter_ref as cref
import letterbox_ref as lref

LIMIT = 65535


def clamp_tiles(tiles, S, canvas):
    """One image's raw int rows -> the list of (src, top, left, h1, w1, y0, x0, y1, x1) the kernel acts on (empty rectangles dropped)."""
    H, W = int(canvas[0]), int(canvas[1])
    out = []
    for row in np.asarray(tiles).reshape(-1, 9)[:4]:
        s, top, left, h1, w1, y0, x0, y1, x1 = (int(v) for v in row)
        if s < 0:
            break
        s = min(s, S - 1)
        h1, w1 = max(min(h1, LIMIT), 1), max(min(w1, LIMIT), 1)
        top, left = max(min(top, LIMIT), -LIMIT), max(min(left, LIMIT), -LIMIT)
        y0, x0 = max(y0, 0, top), max(x0, 0, left)
        y1, x1 = min(y1, H, top + h1), min(x1, W, left + w1)
        if y0 < y1 and x0 < x1:
            out.append((s, top, left, h1, w1, y0, x0, y1, x1))
    return out


def resize_window(v, h1, w1, rows, cols):
    """oracle.resize_linear_f32(v, (h1, w1))[rows[0]:rows[1], cols[0]:cols[1]].  A window far larger than the canvas is not formed whole:
    the rule is separable and local, so the wanted block is cut from the resize of the few destination rows and columns it needs --
    which oracle.resize_linear_f32 gives only for a full destination size, hence the restatement of its rule here for that case."""
    if h1 * w1 <= 1 << 22:
        return oracle.resize_linear_f32(v, (h1, w1))[rows[0]:rows[1], cols[0]:cols[1]]
    hd, wd = v.shape[:2]

    def taps(n_dst, n_src, a, b):
        i = np.arange(a, b)
        f = ((i + 0.5) * (np.float64(n_src) / np.float64(n_dst)) - 0.5).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        f = f - s.astype(np.float32)
        lo, hi = s < 0, s >= n_src - 1
        s = np.where(lo, 0, np.where(hi, n_src - 1, s))
        f = np.where(lo | hi, np.float32(0), f).astype(np.float32)
        return s, np.minimum(s + 1, n_src - 1), f
    sy, sy1, fy = taps(h1, hd, *rows)
    sx, sx1, fx = taps(w1, wd, *cols)
    one = np.float32(1)
    ax0, ax1 = (one - fx)[None, :, None], fx[None, :, None]
    r0 = v[sy][:, sx] * ax0 + v[sy][:, sx1] * ax1
    r1 = v[sy1][:, sx] * ax0 + v[sy1][:, sx1] * ax1
    return (r0 * (one - fy)[:, None, None] + r1 * fy[:, None, None]).astype(np.float32)


def compose(images, augs, tiles, canvas, color=None, mean=lref.MEAN, std=lref.STD):
    """One output image float32 [3, H, W] and its ownership map int [H, W] (-1: fill) from the source ``images`` (uint8), their ``augs`` and the
    image's raw tile rows (clamped here).  ``color``: the output image's (fb, fc, fs)."""
    H, W = int(canvas[0]), int(canvas[1])
    out = np.zeros((H, W, 3), np.float32)
    owner = np.full((H, W), -1, np.int64)
    for k, (s, top, left, h1, w1, y0, x0, y1, x1) in enumerate(clamp_tiles(tiles, len(images), canvas)):
        im = images[s]
        x = lref.whiten(im, mean, std) if color is None else cref.whiten(cref.jitter(im, color), mean, std).astype(np.float32)
        v = lref.drift_flip(x, augs[s])
        block = resize_window(v, h1, w1, (y0 - top, y1 - top), (x0 - left, x1 - left))
        free = owner[y0:y1, x0:x1] < 0
        out[y0:y1, x0:x1][free] = block[free]
        owner[y0:y1, x0:x1][free] = k
    return np.ascontiguousarray(out.transpose(2, 0, 1)), owner


def check_fill(out, owner, tag=""):
    vals = out[:, owner < 0]
    assert np.array_equal(vals, np.zeros_like(vals)), f"{tag}: the fill region is not exactly 0"
    assert not np.signbit(vals).any(), f"{tag}: negative zero in the fill region"


def tiles_of(drifted_sizes, centre, zooms, canvas, src=0):
    """The tile rule as loops: four rows (src + t, top, left, h1, w1, y0, x0, y1, x1)."""
    H, W = int(canvas[0]), int(canvas[1])
    cy, cx = int(centre[0]), int(centre[1])
    rows = []
    for t in range(4):
        _, _, h, w = lref.window(drifted_sizes[t], canvas)
        h1 = max(1, int(math.floor(float(h) * float(zooms[t]) + 0.5)))
        w1 = max(1, int(math.floor(float(w) * float(zooms[t]) + 0.5)))
        top = cy - h1 if t in (0, 1) else cy
        left = cx - w1 if t in (0, 2) else cx
        qy0, qy1 = (0, cy) if t in (0, 1) else (cy, H)
        qx0, qx1 = (0, cx) if t in (0, 2) else (cx, W)
        y0, y1 = max(qy0, top, 0), min(qy1, top + h1, H)
        x0, x1 = max(qx0, left, 0), min(qx1, left + w1, W)
        rows.append((src + t, top, left, h1, w1, y0, x0, max(y1, y0), max(x1, x0)))
    return rows


def letterbox_box(box, size, aug, window):
    """One xyxy box of an H0 x W0 image through clip, drift, flip and the letterbox window, every step in float32 (the order of
    ``BaseDataset.preprocess``, then x * sx + left, y * sy + top with (sy, sx) = float32(h1 / Hd), float32(w1 / Wd))."""
    f = np.float32
    h0, w0 = int(size[0]), int(size[1])
    dy, dx, fl = (int(v) for v in aug)
    top, left, h1, w1 = (int(v) for v in window)
    x1, y1, x2, y2 = (f(v) for v in box)
    x1, x2 = (min(max(v, f(0)), f(w0 - 1.)) for v in (x1, x2))
    y1, y2 = (min(max(v, f(0)), f(h0 - 1.)) for v in (y1, y2))
    x1, x2, y1, y2 = f(x1 - f(dx)), f(x2 - f(dx)), f(y1 - f(dy)), f(y2 - f(dy))
    hd, wd = h0 - dy, w0 - dx
    if fl:
        width = f(x2 - x1)
        x1 = f(f(wd - 1) - x2)
        x2 = f(x1 + width)
    sy, sx = f(h1 / hd), f(w1 / wd)
    return f(f(x1 * sx) + f(left)), f(f(y1 * sy) + f(top)), f(f(x2 * sx) + f(left)), f(f(y2 * sy) + f(top))


def clip_rule(box, rect, min_visible):
    """One transformed box against a rectangle (y0, x0, y1, x1): (clipped box, kept, visible), float32."""
    f = np.float32
    y0, x0, y1, x1 = (int(v) for v in rect)
    bx1, by1, bx2, by2 = (f(v) for v in box)
    cx1, cx2 = (min(max(v, f(x0)), f(x1 - 1)) for v in (bx1, bx2))
    cy1, cy2 = (min(max(v, f(y0)), f(y1 - 1)) for v in (by1, by2))
    cw, ch = f(cx2 - cx1), f(cy2 - cy1)
    area = f(f(bx2 - bx1) * f(by2 - by1))
    kept = bool(cw >= 2 and ch >= 2 and f(cw * ch) >= f(f(min_visible) * area))
    return (cx1, cy1, cx2, cy2), kept, bool(cw > 0 and ch > 0)


def boxes_of(sources, tiles, min_visible, ignore):
    """The box rule of one mosaic image as loops.  ``sources``: per tile (class_ids, boxes, flagged boxes, (H0, W0), aug); ``tiles``: the rows of
    ``tiles_of``.  Returns (class ids, boxes, ignore boxes, counts) with counts = {'whole', 'clipped', 'dropped'} of the unflagged boxes."""
    cls, out, ign = [], [], []
    counts = {"whole": 0, "clipped": 0, "dropped": 0}
    for (c, boxes, flagged, size, aug), row in zip(sources, tiles):
        _, top, left, h1, w1, y0, x0, y1, x1 = row
        if y1 <= y0 or x1 <= x0:
            counts["dropped"] += len(boxes)
            continue
        for ci, box in zip(c, boxes):
            tb = letterbox_box(box, size, aug, (top, left, h1, w1))
            cb, kept, vis = clip_rule(tb, (y0, x0, y1, x1), min_visible)
            if kept:
                cls.append(int(ci)); out.append(cb)
                counts["whole" if tuple(cb) == tuple(tb) else "clipped"] += 1
            else:
                counts["dropped"] += 1
                if ignore and vis:
                    ign.append(cb)
        for box in flagged:
            cb, _, vis = clip_rule(letterbox_box(box, size, aug, (top, left, h1, w1)), (y0, x0, y1, x1), min_visible)
            if vis:
                ign.append(cb)
    return (np.asarray(cls, np.int64), np.asarray(out, np.float32).reshape(-1, 4), np.asarray(ign, np.float32).reshape(-1, 4), counts)
