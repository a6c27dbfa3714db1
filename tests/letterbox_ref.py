"""Plain numpy restatement of the letterbox geometry ("Letterbox and zoom-out"): the yardstick of
tests/test_letterbox_host.py and tests/test_letterbox_gpu.py.  No project code is involved.

V is the image after whitening (oracle arithmetic), drift (slicing, with a zero fill AFTER whitening) and flip -- the composition
tests/test_augment_gpu.py uses -- of size Hd x Wd.  The window (top, left, h1, w1) on the H x W canvas is, unless given,
  H * Wd <= W * Hd:  h1 = H, w1 = max(1, (Wd * H + Hd // 2) // Hd);   else:  w1 = W, h1 = max(1, (Hd * W + Wd // 2) // Wd);
  top = (H - h1) // 2, left = (W - w1) // 2.
Inside the window the pixels are ``oracle.resize_linear_f32(V, (h1, w1))``, outside it +0.0.  ``scales`` = (h1 / Hd, w1 / Wd) as float32
(float64 division, cast), ``shifts`` = (-(float32)top / sy, -(float32)left / sx), ``padding`` = (top / sy, bottom / sy, left / sx,
right / sx) in float32."""
import numpy as np

import oracle

MEAN = oracle.KITTI_RGB_MEAN.reshape(1, 1, 3).astype(np.float32)
STD = oracle.KITTI_RGB_STD.reshape(1, 1, 3).astype(np.float32)


def window(size, canvas):
    """(top, left, h1, w1) of an Hd x Wd image on the canvas: Python integers, floor divisions."""
    hd, wd = int(size[0]), int(size[1])
    H, W = int(canvas[0]), int(canvas[1])
    if H * wd <= W * hd:
        h1, w1 = H, max(1, (wd * H + hd // 2) // hd)
    else:
        h1, w1 = max(1, (hd * W + wd // 2) // wd), W
    return (H - h1) // 2, (W - w1) // 2, h1, w1


def whiten(im, mean=MEAN, std=STD):
    return (np.asarray(im).astype(np.float32) - np.asarray(mean, np.float32).reshape(1, 1, 3)) / np.asarray(std, np.float32).reshape(1, 1, 3)


def drift_flip(x, aug):
    """A whitened float32 [H0, W0, 3] image -> V: drift with a zero fill, then flip."""
    dy, dx, fl = (int(v) for v in aug)
    h0, w0 = x.shape[:2]
    v = np.zeros((h0 - dy, w0 - dx, 3), np.float32)
    v[max(-dy, 0):, max(-dx, 0):] = x[max(dy, 0):, max(dx, 0):]
    return np.ascontiguousarray(v[:, ::-1] if fl else v)


def compose(v, canvas, win=None):
    """V float32 [Hd, Wd, 3] -> (canvas image float32 [3, H, W], the window)."""
    H, W = int(canvas[0]), int(canvas[1])
    top, left, h1, w1 = window(v.shape[:2], canvas) if win is None else (int(t) for t in win)
    out = np.zeros((H, W, 3), np.float32)
    out[top:top + h1, left:left + w1] = oracle.resize_linear_f32(v, (h1, w1))
    return np.ascontiguousarray(out.transpose(2, 0, 1)), (top, left, h1, w1)


def reference(im, aug, canvas, win=None, x=None):
    """One uint8 image (or its already whitened form ``x``) -> (image [3, H, W], window, (Hd, Wd))."""
    v = drift_flip(whiten(im) if x is None else x, aug)
    y, w = compose(v, canvas, win)
    return y, w, v.shape[:2]


def inside(win, canvas):
    """bool [H, W]: true inside the window."""
    top, left, h1, w1 = (int(t) for t in win)
    m = np.zeros((int(canvas[0]), int(canvas[1])), bool)
    m[top:top + h1, left:left + w1] = True
    return m


def scales_shifts_padding(size, win, canvas):
    """(scales float32 [2], shifts float32 [2], padding float32 [4]) of an Hd x Wd image in the window."""
    top, left, h1, w1 = (int(t) for t in win)
    H, W = int(canvas[0]), int(canvas[1])
    scales = np.array([h1 / int(size[0]), w1 / int(size[1])], dtype=np.float32)
    sy, sx = scales
    f = np.float32
    shifts = np.array([-f(top) / sy, -f(left) / sx], np.float32)
    padding = np.array([f(top) / sy, f(H - h1 - top) / sy, f(left) / sx, f(W - w1 - left) / sx], np.float32)
    return scales, shifts, padding


def check_fill(out, win, canvas, tag=""):
    """The fill region of ``out`` [3, H, W] is exactly +0.0f (no NaN left over, no negative zero)."""
    fill = ~inside(win, canvas)
    vals = out[:, fill]
    assert np.array_equal(vals, np.zeros_like(vals)), f"{tag}: the fill region is not exactly 0"
    assert not np.signbit(vals).any(), f"{tag}: negative zero in the fill region"
