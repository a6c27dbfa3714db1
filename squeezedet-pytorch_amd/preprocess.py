"""GPU-side input pipeline.

The reference pre-processes every image on the CPU inside DataLoader worker processes
(``DataWrapper.__getitem__`` src/engine/detector.py:132-142 -> ``BaseDataset.preprocess`` src/datasets/base.py:43-59:
``whiten`` src/utils/image.py:9-19, ``resize`` :77-88 = ``cv2.resize`` INTER_LINEAR, then ``transpose(2, 0, 1)``) and
uploads 5.75 MB of fp32 per image.  Here the raw uint8 HWC images are uploaded (4x fewer bytes) and ONE kernel
whitens, resizes and transposes the whole batch on the GPU.  ``image_meta`` carries the same keys the reference's
eval path produces (``orig_size``, ``rgb_mean``, ``rgb_std``, ``scales``, ``drifts``, ``drifted_size``, ``flipped``).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native as nat
from .boxes import letterbox_meta, letterbox_window, pad_crop

KITTI_RGB_MEAN = np.array([93.877, 98.801, 95.923], dtype=np.float32)      # src/datasets/kitti.py:17
KITTI_RGB_STD = np.array([78.782, 80.130, 81.200], dtype=np.float32)       # src/datasets/kitti.py:18


_ENTRY_STEM = {'resize': 'sqd_preprocess_u8', 'padcrop': 'sqd_preprocess_u8_padcrop', 'letterbox': 'sqd_preprocess_u8_letterbox',
               'mosaic': 'sqd_preprocess_u8_mosaic'}
_Float3 = ctypes.c_float * 3


def c_float3(values):
    """Three floats (a mean or a std) as the host ``const float*`` the input entry points take."""
    return values if isinstance(values, _Float3) else _Float3(*[float(v) for v in np.asarray(values).reshape(-1)])


def entry_name(geometry, aug=False, color=False):
    """The C entry point of one of the input kernels (csrc/preproc.hip): geometry x (eval, aug, aug + colour); 'mosaic' (training
    only) has the two aug forms."""
    if geometry not in _ENTRY_STEM:
        raise ValueError(f"launch_u8: geometry must be 'resize', 'padcrop', 'letterbox' or 'mosaic', got {geometry!r}")
    if geometry == 'mosaic' and not aug:
        raise ValueError('launch_u8: mosaic is a training geometry, it has no eval entry (give aug)')
    if color and not aug:
        raise ValueError('launch_u8: the colour forms exist only with aug (there is no eval-time colour entry)')
    return _ENTRY_STEM[geometry] + ('_aug' if aug else '') + ('_color' if color else '') + '_fwd'


def launch_u8(geometry, src, offsets, sizes, out, B, H, W, mean, std, device, *, aug=None, color=None, sums=None, win=None,
              scales=None, shifts=None, padcrop=None, tiles=None, S=None, stream=None):
    """The one launch of the uint8 input pipeline: picks the entry point from (``geometry``, ``aug`` given, ``color`` given), puts its
    arguments in the entry's order (include/sqd_hip.h) and checks its status.  Pointer arguments are device tensors, ``ctypes.c_void_p``
    addresses (blocks inside a packed upload) or None; ``mean`` / ``std`` anything ``c_float3`` takes.  Argument blocks per geometry:
    ``aug`` int32 [B,3] (any geometry); ``color`` fp32 [B,3] with ``sums`` [B,3,2] of ``ops.image_stats_u8`` (only with ``aug``); ``win`` int32
    [B,4] (letterbox only); outputs ``scales`` (resize, letterbox), ``shifts`` (padcrop, letterbox), ``padcrop`` int32 [B,8] (padcrop).
    ``geometry='mosaic'`` (DESIGN.md 6b "Mosaic"): ``tiles`` int32 [B,4,9] and ``S``, the number of source images -- ``offsets``, ``sizes``,
    ``aug`` and ``sums`` then have S rows, ``color`` stays [B,3]; no side outputs.
    ``stream``: a raw stream handle instead of ``device``'s current stream.  A combination without an entry raises ValueError."""
    name = entry_name(geometry, aug is not None, color is not None)
    if (tiles is not None or S is not None) != (geometry == 'mosaic') or (geometry == 'mosaic' and (tiles is None or S is None)):
        raise ValueError('launch_u8: tiles and S belong to the mosaic geometry, which needs both')
    if geometry == 'mosaic' and (scales is not None or shifts is not None):
        raise ValueError('launch_u8: mosaic writes no scales or shifts (the tile list is the record)')
    if (color is None) != (sums is None):
        raise ValueError('launch_u8: color and sums go together')
    if win is not None and geometry != 'letterbox':
        raise ValueError('launch_u8: win belongs to the letterbox geometry')
    if padcrop is not None and geometry != 'padcrop':
        raise ValueError(f'launch_u8: padcrop is an output of the padcrop geometry, not of {geometry}')
    if (scales is not None and geometry == 'padcrop') or (shifts is not None and geometry == 'resize'):
        raise ValueError(f'launch_u8: {geometry} writes ' + ('shifts and padcrop, not scales' if geometry == 'padcrop' else 'scales, not shifts'))
    p = lambda t: t if isinstance(t, ctypes.c_void_p) else nat.ptr(t)      # noqa: E731
    args = [p(src), p(offsets), p(sizes)]
    if aug is not None:
        args.append(p(aug))
    if geometry == 'letterbox':
        args.append(p(win))
    if geometry == 'mosaic':
        args.append(p(tiles))
    if color is not None:
        args += [p(color), p(sums)]
    args.append(p(out))
    args += {'resize': [p(scales)], 'padcrop': [p(shifts), p(padcrop)], 'letterbox': [p(scales), p(shifts)], 'mosaic': []}[geometry]
    dims = (B, int(S), H, W) if geometry == 'mosaic' else (B, H, W)
    rc = getattr(nat.lib(), name)(*args, c_float3(mean), c_float3(std), *dims, nat.stream_handle(device) if stream is None else stream)
    nat.check(rc, name)


_STAGE = [None, None]        # two pinned staging buffers used alternately: the H2D copy of the previous batch may still run


def _staging(nbytes):
    _STAGE.reverse()
    buf = _STAGE[0]
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        _STAGE[0] = buf
    return buf[:nbytes]


_POOL = None


def _pack_pool():
    global _POOL
    if _POOL is None:
        import concurrent.futures
        import os
        _POOL = concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1), thread_name_prefix='sqd-pack')
    return _POOL


def preprocess_batch(images, input_size, device='cuda', rgb_mean=KITTI_RGB_MEAN, rgb_std=KITTI_RGB_STD, out=None, forbid_resize=False,
                     letterbox=False):
    """images: list of uint8 numpy arrays [H0, W0, 3] (RGB, any sizes).  Returns (image fp32 NCHW [B,3,H,W] on
    ``device``, scales fp32 [B,2] = (H/H0, W/W0) on ``device``, image_meta dict of per-image lists/arrays).
    ``forbid_resize`` (``cfg.forbid_resize``, src/datasets/base.py:53-54): whiten + ``crop_or_pad`` instead of whiten + resize --
    the second return value is then the box shift fp32 [B,2] = (dy, dx) = (crops - padding)(top, left) that ``ops.detect(...,
    shifts=)`` adds (``boxes_postprocess``' padding / crops terms), and ``image_meta`` carries ``padding`` / ``crops`` (int16 [B,4],
    (top, bottom, left, right)) instead of ``scales``.  Bit-exact against the reference (tests/golden/padcrop.npz).
    ``letterbox`` (``cfg.letterbox``, DESIGN.md 6b "Letterbox and zoom-out"): whiten + resize with the aspect ratio kept into the centred
    window of ``boxes.letterbox_window``, zeros around it -- the second return value is then the pair (scales, shifts), fp32 [B,2] each,
    that ``ops.detect(..., scales=, shifts=)`` takes, and ``image_meta`` carries ``boxes.letterbox_meta``'s ``scales``, ``padding`` (float32,
    in original-image pixels) and ``letterbox`` (the window)."""
    if letterbox and forbid_resize:
        raise ValueError('preprocess_batch: letterbox and forbid_resize are two different input geometries')
    if len(images) == 0:
        raise ValueError('preprocess_batch: empty batch')
    H, W = int(input_size[0]), int(input_size[1])
    B = len(images)
    sizes = np.empty((B, 2), dtype=np.int32)
    offsets = np.empty(B, dtype=np.int64)
    total = 0
    for i, im in enumerate(images):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f'preprocess_batch: image {i} must be uint8 [H,W,3], got {im.dtype} {im.shape}')
        if im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError('preprocess_batch: empty image')
        sizes[i] = im.shape[:2]
        offsets[i] = total
        total += im.shape[0] * im.shape[1] * 3
    packed = _staging(total)                             # cached pinned host buffer (page-locking costs milliseconds)
    pk = packed.numpy()

    def _copy(i):
        im = images[i]
        pk[offsets[i]:offsets[i] + im.size] = np.ascontiguousarray(im).reshape(-1)

    if B >= 4 and total >= (1 << 22):                    # numpy releases the GIL while copying: pack in parallel
        list(_pack_pool().map(_copy, range(B)))
    else:
        for i in range(B):
            _copy(i)
    dev = torch.device(device)
    src = packed.to(dev, non_blocking=True)
    d_off = torch.from_numpy(offsets).to(dev, non_blocking=True)
    d_sizes = torch.from_numpy(sizes).to(dev, non_blocking=True)
    if out is None:
        out = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
    elif tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError('preprocess_batch: bad out tensor')
    scales = torch.empty(B, 2, device=dev, dtype=torch.float32)
    base_meta = {'orig_size': np.concatenate([sizes, np.full((B, 1), 3, np.int32)], 1),
                 'drifts': np.zeros((B, 2), np.int32), 'flipped': [False] * B,
                 'rgb_mean': np.tile(np.asarray(rgb_mean, np.float32).reshape(1, 1, 1, 3), (B, 1, 1, 1)),
                 'rgb_std': np.tile(np.asarray(rgb_std, np.float32).reshape(1, 1, 1, 3), (B, 1, 1, 1))}
    if letterbox:
        shifts = torch.empty(B, 2, device=dev, dtype=torch.float32)
        launch_u8('letterbox', src, d_off, d_sizes, out, B, H, W, rgb_mean, rgb_std, dev, scales=scales, shifts=shifts)
        metas = [letterbox_meta(s, letterbox_window(s, (H, W)), (H, W)) for s in sizes]      # the same integers on the host
        base_meta.update({k: np.stack([m[k] for m in metas]) for k in ('scales', 'padding', 'letterbox')})
        return out, (scales, shifts), base_meta
    if forbid_resize:
        launch_u8('padcrop', src, d_off, d_sizes, out, B, H, W, rgb_mean, rgb_std, dev, shifts=scales)
        rows = np.array([pad_crop(int(h0), H) + pad_crop(int(w0), W) for h0, w0 in sizes], np.int16)      # the same integers on the host
        base_meta.update(padding=rows[:, [0, 1, 4, 5]], crops=rows[:, [2, 3, 6, 7]])
        return out, scales, base_meta
    launch_u8('resize', src, d_off, d_sizes, out, B, H, W, rgb_mean, rgb_std, dev, scales=scales)
    meta = dict(base_meta, scales=np.stack([np.array([H / s[0], W / s[1]], dtype=np.float32) for s in sizes]))
    return out, scales, meta
