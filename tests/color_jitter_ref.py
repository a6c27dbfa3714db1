"""Plain numpy float64 restatement of the colour-jitter rule ("Colour jitter"): the yardstick of
tests/test_color_jitter_host.py and tests/test_color_jitter_gpu.py.  This file is the definition; nothing third-party is involved.

Per image, with factors (fb, fc, fs) given as float32 and every operation below in float64:
  g  = (0.299 Sr + 0.587 Sg + 0.114 Sb) / (H0 W0) from the exact integer channel sums of the untouched image, rounded to float32 once;
  p  = min(fb g, 255);
  t(v) = clamp(fc min(fb v, 255) + (1 - fc) p, 0, 255) for a source byte v;
  y  = 0.299 t(r) + 0.587 t(g) + 0.114 t(b) per pixel;
  c' = clamp(fs t(c) + (1 - fs) y, 0, 255) per channel;
then ``whiten``: (c' - mean) / std with the float32 mean / std.  The jitter is a property of the source pixels: drift, flip, resize and
crop_or_pad act on its whitened result exactly as they act on the whitened source without it."""
import numpy as np

LUMA = (0.299, 0.587, 0.114)


def channel_sums(im):
    """Exact per-channel pixel sums of a uint8 [H, W, 3] image as Python ints."""
    x = np.asarray(im)
    assert x.dtype == np.uint8 and x.ndim == 3 and x.shape[2] == 3
    return [int(x[:, :, c].sum(dtype=np.uint64)) for c in range(3)]


def mean_luma(im):
    """g: float64 from the exact sums, rounded to float32 once (returned as float64)."""
    s = channel_sums(im)
    n = int(im.shape[0]) * int(im.shape[1])
    g = (LUMA[0] * float(s[0]) + LUMA[1] * float(s[1]) + LUMA[2] * float(s[2])) / float(n)
    return np.float64(np.float32(g))


def pivot(im, color):
    fb = np.float64(np.float32(color[0]))
    return min(fb * mean_luma(im), np.float64(255.0))


def tone(v, color, p):
    """t(v), float64, elementwise over ``v`` (source byte values)."""
    fb, fc = np.float64(np.float32(color[0])), np.float64(np.float32(color[1]))
    v = np.asarray(v, np.float64)
    return np.clip(fc * np.minimum(fb * v, 255.0) + (1.0 - fc) * p, 0.0, 255.0)


def jitter(im, color):
    """uint8 [H, W, 3] -> float64 [H, W, 3]: the jittered pixels c', before whitening."""
    fs = np.float64(np.float32(color[2]))
    t = tone(np.asarray(im), color, pivot(im, color))
    y = LUMA[0] * t[:, :, 0] + LUMA[1] * t[:, :, 1] + LUMA[2] * t[:, :, 2]
    return np.clip(fs * t + (1.0 - fs) * y[:, :, None], 0.0, 255.0)


def whiten(x, mean, std):
    """(x - mean) / std in float64 with the float32 mean / std values."""
    m = np.asarray(mean, np.float32).reshape(1, 1, 3).astype(np.float64)
    s = np.asarray(std, np.float32).reshape(1, 1, 3).astype(np.float64)
    return (np.asarray(x, np.float64) - m) / s
