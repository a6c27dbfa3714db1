"""``TrainLoader``: the training side of ``Detector.detect_dataset`` -- batches of a reference-protocol dataset (``load_image(i)``,
``load_annotations(i)``, ``__len__``, ``rgb_mean``, ``rgb_std``; src/datasets/base.py, src/datasets/kitti.py) delivered on the
device as ``{'image', 'image_meta', 'gt'}`` (with ``cfg.sparse_gt``: ``'gt_sparse'``, an ``ops.SparseGT``, in place of the dense ``'gt'``),
augmented the reference's train-phase way (``augment``), ready for ``Trainer.run_epoch``.

``load_annotations(i)`` may return a third element, per-box flags (bool / uint8 [n], nonzero = ignore: KITTI ``DontCare``, VOC
``difficult``, COCO ``crowd``).  A flagged box never becomes a positive and never bounds the drift, so the draws of a dataset are the
same with and without its flagged boxes.  With ``cfg.ignore_overlap`` unset the flagged boxes are dropped (what the reference's KITTI
loader does to ``DontCare``); with it set (``cfg.sparse_gt`` only) they follow the image's draw, are clipped to the network input and
become ``'gt_ignore'``, the anchor ignore bitmap of ``ops.anchor_ignore_mask`` that the masked loss reads.  An image without an
unflagged box is a legal, object-free image.  With ``cfg.match_iou`` set (``cfg.sparse_gt`` only; ``config.check_match``) the IoU-threshold
matcher (``ops.anchor_match``) runs after the encoder: ``'gt_sparse'`` then holds its extra positives too, ``'gt_ignore'`` its band and
overflow (ORed onto the regions' bits), and ``'gt_match_overflow'`` the per-image overflow counts, a device tensor nothing waits on.

``cfg.num_workers`` threads load the next batch and pack its raw pixels into a pinned staging buffer owned by the loader (two,
used alternately; one is refilled only after an event shows its previous host-to-device copy has finished).  The main thread
draws the epoch permutation and every augmentation parameter from ONE ``np.random.RandomState``, in dataset order, so the batches
do not depend on ``num_workers``.  This departs on purpose from the reference, whose forked DataLoader workers each start from
the same numpy state and so repeat one another's draws; with ``shuffle=False`` and a fixed seed the draws here are those of a
single-process reference run under ``np.random.seed(seed)``.

Data parallel: every rank draws for the whole global batch (``cfg.batch_size`` images) and keeps its ``shard_sizes`` slice, so
the union of the ranks' batches is the one-rank batch.  The other ranks' images are only needed for their sizes (the drift
bounds); a dataset may provide ``image_size(i) -> (H, W)`` to spare loading them, and sizes are cached across epochs.

Mosaic (``cfg.mosaic_prob > 0``, with ``cfg.letterbox``; DESIGN.md 6b "Mosaic"): an image becomes, with that probability, a composition of
itself and three partner images drawn from the dataset around a random centre.  Everything is drawn from a fourth RandomState
(``[seed mod 2^32, MOSAIC_STREAM]``, ``augment.draw_mosaic``), for the whole global batch, so ``index``, ``aug``, ``color`` and the letterbox
windows of a dataset are the same with mosaic on and off.  Each rank loads the partners of its own slice only; the upload then holds
the S source images in (image, tile) order and ONE launch of the mosaic entry composes the batch.  ``loader.mosaic_prob`` may be changed
between epochs (the usual recipe switches mosaic off for the last ones); at 0 the loader takes the path without mosaic: the same
launches, the same bytes.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import augment
from .config import check_geometry, check_match, check_mosaic
from .annotations import clip_ignore_boxes, encode_annotations, ignore_overlap_of, split_flagged
from .trainer import shard_sizes


COLOR_STREAM = 0xC0105EED      # second word of the colour RandomState's seed key
ZOOM_STREAM = 0x200D0075       # ... and of the zoom-out one
MOSAIC_STREAM = 0x305A1C04     # ... and of the mosaic one


class _Stage:
    """One pinned upload buffer and the event of its latest host-to-device copy."""

    def __init__(self):
        self.buf = None
        self.np = None
        self.copied = None

    def acquire(self, nbytes):
        if self.copied is not None:
            self.copied.synchronize()                 # the previous copy out of this buffer has finished
            self.copied = None
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
            self.np = self.buf.numpy()
        return self.np


class TrainLoader:
    """Iterable of device-resident training batches over ``dataset`` (see the module docstring).

    cfg fields read: batch_size (global), input_size, num_workers, device, drift_prob, flip_prob, seed, forbid_resize, anchors,
    num_classes, brightness_jitter, contrast_jitter, saturation_jitter, sparse_gt, ignore_overlap, match_iou, match_ignore_iou, match_max_extra, letterbox, zoom_out.  ``seed`` (default ``cfg.seed``) seeds the loader's RandomState
    once (and, as ``[seed mod 2^32, COLOR_STREAM]``, the colour one; as ``[seed mod 2^32, ZOOM_STREAM]``, the zoom-out one); each epoch
    (``iter``) continues them.  ``cfg.letterbox``: the letterbox geometry (DESIGN.md 6b "Letterbox and zoom-out"), the window of every
    image in ``plan()``'s ``'window'`` and ``image_meta['letterbox']``; ``cfg.zoom_out`` = d in (0, 1) shrinks and places it
    (``augment.draw_zoom``, three draws per image of the global batch from the zoom-out RandomState: the drift / flip / colour draws of a
    dataset are the same with and without it)."""

    def __init__(self, dataset, cfg, seed=None, shuffle=True, drop_last=True, rank=0, world=1):
        self.dataset, self.cfg = dataset, cfg
        self.shuffle, self.drop_last = bool(shuffle), bool(drop_last)
        self.rank, self.world = int(rank), int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f'TrainLoader: rank {rank} outside world {world}')
        self.batch_size = int(cfg.batch_size)
        self.ignore_overlap = ignore_overlap_of(cfg, 'TrainLoader')
        self.match = check_match(cfg, 'TrainLoader')
        seed = getattr(cfg, 'seed', 42) if seed is None else seed
        self.rng = np.random.RandomState(seed)
        self.color_rng = np.random.RandomState(None if seed is None else np.append(np.asarray(seed, np.int64).reshape(-1) & 0xFFFFFFFF, COLOR_STREAM))
        self.color_jitter = tuple(float(getattr(cfg, k, 0.)) for k in ('brightness_jitter', 'contrast_jitter', 'saturation_jitter'))
        if any(not np.isfinite(d) or d < 0 for d in self.color_jitter):
            raise ValueError(f'TrainLoader: colour jitter amounts must be finite and >= 0, got {self.color_jitter}')
        self.color_on = any(d > 0 for d in self.color_jitter)
        self.letterbox, self.zoom_out = check_geometry(cfg, 'TrainLoader')
        self.zoom_rng = np.random.RandomState(None if seed is None else np.append(np.asarray(seed, np.int64).reshape(-1) & 0xFFFFFFFF, ZOOM_STREAM))
        self.mosaic_prob, self.mosaic_scale, self.mosaic_min_visible = check_mosaic(cfg, 'TrainLoader')
        self.mosaic_rng = np.random.RandomState(None if seed is None else np.append(np.asarray(seed, np.int64).reshape(-1) & 0xFFFFFFFF, MOSAIC_STREAM))
        self.drift_prob = float(getattr(cfg, 'drift_prob', 1.0))
        self.flip_prob = float(getattr(cfg, 'flip_prob', 0.5))
        self.forbid_resize = bool(getattr(cfg, 'forbid_resize', False))
        self.workers = int(getattr(cfg, 'num_workers', 4))
        self.device = torch.device(cfg.device)
        self.rgb_mean = getattr(dataset, 'rgb_mean', augment.KITTI_RGB_MEAN)
        self.rgb_std = getattr(dataset, 'rgb_std', augment.KITTI_RGB_STD)
        self._sizes = {}
        self._stages = [_Stage(), _Stage()]
        n = len(dataset)
        last = n % self.batch_size
        if self.world > 1 and not self.drop_last and 0 < last < self.world:
            raise ValueError(f'TrainLoader: the last batch ({last} images) leaves a rank without images; use drop_last')

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _global_batches(self):
        n = len(self.dataset)
        order = self.rng.permutation(n) if self.shuffle else np.arange(n)
        return [order[i:i + self.batch_size] for i in range(0, len(self) * self.batch_size, self.batch_size) if i < n]

    def _local(self, idxs):
        sh = shard_sizes(len(idxs), self.world)
        lo = sum(sh[:self.rank])
        return lo, lo + sh[self.rank]

    def _size_of(self, i):
        if i not in self._sizes:
            if hasattr(self.dataset, 'image_size'):
                h, w = self.dataset.image_size(i)[:2]
            else:
                h, w = np.asarray(self.dataset.load_image(i)[0]).shape[:2]
            self._sizes[i] = (int(h), int(w))
        return self._sizes[i]

    def _load(self, i):
        im = self.dataset.load_image(i)
        im = im[0] if isinstance(im, tuple) else im
        im = augment.as_u8_image(im, f'TrainLoader: image {i}')
        self._sizes[int(i)] = (int(im.shape[0]), int(im.shape[1]))
        return im

    def _draw_mosaic(self, idxs):
        """The mosaic draws of one global batch (main thread, batch order), or None while ``mosaic_prob`` is 0.  The partners' sizes come
        through the size cache and their annotations are loaded here: their drift draws need both.  The dict of ``augment.draw_mosaic``
        plus ``'ann'``: {partner index: split annotations}."""
        prob = float(self.mosaic_prob)
        if not (np.isfinite(prob) and 0. <= prob <= 1.):
            raise ValueError(f'TrainLoader: mosaic_prob must be in [0, 1], got {self.mosaic_prob!r}')
        if prob == 0.:
            return None
        if not self.letterbox:
            raise ValueError('TrainLoader: mosaic composes letterbox windows, it needs cfg.letterbox')
        ann = {}

        def partner(j):
            if j not in ann:
                ann[j] = split_flagged(self.dataset.load_annotations(j))
            return self._size_of(j), ann[j][1]

        mz = augment.draw_mosaic(self.mosaic_rng, len(idxs), len(self.dataset), self.cfg.input_size, prob, self.mosaic_scale, partner,
                                 self.drift_prob, self.flip_prob)
        mz['ann'] = ann
        return mz

    def _sources(self, idxs, mz):
        """This rank's source images in (image, tile) order: (dataset indices, position of every local image's own source)."""
        lo, hi = self._local(idxs)
        src, own = [], []
        for k in range(lo, hi):
            own.append(len(src))
            src.append(int(idxs[k]))
            if mz is not None and mz['mosaic'][k]:
                src += [int(j) for j in mz['partners'][k]]
        return src, own

    def _prepare(self, pool, stage, idxs, mz=None):
        """Start loading the batch's own images and every annotation of the global batch and packing the pixels into ``stage``
        (worker threads; inline without workers).  The global batch's other images only report their sizes.  Returns a function
        that waits for all of it and returns (local sizes, header bytes, pixel offsets, total bytes, annotations, global sizes).
        ``mz`` (``_draw_mosaic``): the partners of this rank's mosaic images are loaded and packed with the rest, in (image, tile) order."""
        lo, hi = self._local(idxs)
        mine, own = self._sources(idxs, mz)

        def others():
            return {int(i): self._size_of(int(i)) for k, i in enumerate(idxs) if not lo <= k < hi}

        def annotations():
            return [self.dataset.load_annotations(int(i)) for i in idxs]

        def pack(ims, parallel):
            sizes = [im.shape[:2] for im in ims]
            if mz is None:
                hdr, offsets, total = augment.pack_layout(sizes, self.color_on, self.letterbox)
            else:
                hdr, offsets, total = augment.pack_layout(sizes, self.color_on, tiles=hi - lo)
            pk = stage.acquire(total)

            def put(k):                               # (numpy releases the GIL while copying)
                pk[hdr + offsets[k]:hdr + offsets[k] + ims[k].size] = np.ascontiguousarray(ims[k]).reshape(-1)
            if parallel:
                for f in [pool.submit(put, k) for k in range(len(ims))]:
                    f.result()
            else:
                for k in range(len(ims)):
                    put(k)
            return sizes, hdr, offsets, total

        if pool is None:
            packed, oth, ann = pack([self._load(i) for i in mine], False), others(), annotations()
            return lambda: self._gather(idxs, packed, oth, ann, own)
        f_ims = [pool.submit(self._load, i) for i in mine]
        f_oth = pool.submit(others)
        f_ann = pool.submit(annotations)
        # the packer waits only on tasks queued before it (no deadlock in a one-thread pool); it fans the copies out to the other
        # threads when there are any
        f_pack = pool.submit(lambda: pack([f.result() for f in f_ims], self.workers > 1))
        return lambda: self._gather(idxs, f_pack.result(), f_oth.result(), f_ann.result(), own)

    def _gather(self, idxs, packed, oth, ann, own):
        sizes, hdr, offsets, total = packed
        lo, hi = self._local(idxs)
        gsizes = [sizes[own[k - lo]] if lo <= k < hi else oth[int(i)] for k, i in enumerate(idxs)]
        return sizes, hdr, offsets, total, ann, gsizes

    def _plan_batch(self, idxs, gsizes, ann, mz=None):
        """The host half of a batch: draws for the whole global batch (main thread, batch order), then this rank's slice of the
        draws, transformed boxes, per-image metas and class ids (jitter on: ``'color'``, this rank's slice of the colour factors).
        ``mz``: the batch's mosaic draws (``_draw_mosaic``), see ``_plan_mosaic``."""
        lo, hi = self._local(idxs)
        ann = [split_flagged(a) for a in ann]             # (class ids, boxes, flagged boxes): the draws see the unflagged boxes only
        box_all = [b for _, b, _ in ann]
        aug_all = augment.draw_augmentation(self.rng, gsizes, box_all, self.drift_prob, self.flip_prob)
        aug = aug_all[lo:hi]
        wins = [None] * (hi - lo)
        if self.letterbox:
            # the windows of the whole global batch (the zoom draws depend on them), then this rank's slice
            win_all = np.array([augment.letterbox_window((h - int(a[0]), w - int(a[1])), self.cfg.input_size)
                                for (h, w), a in zip(gsizes, aug_all)], np.int32).reshape(-1, 4)
            if self.zoom_out > 0:
                win_all = augment.draw_zoom(self.zoom_rng, win_all, self.cfg.input_size, self.zoom_out)
            wins = win_all[lo:hi]
        geo = (self.cfg.input_size, self.forbid_resize, self.letterbox)
        tb, metas = zip(*[augment.transform_boxes(b, s, a, *geo, w) for b, s, a, w in zip(box_all[lo:hi], gsizes[lo:hi], aug, wins)])
        p = {'index': np.asarray(idxs[lo:hi], np.int64), 'aug': aug, 'boxes': list(tb), 'metas': list(metas),
             'class_ids': [np.asarray(c) for c, _, _ in ann[lo:hi]]}
        if self.letterbox:
            p['window'] = wins
        if self.ignore_overlap is not None:
            p['ignore_boxes'] = [clip_ignore_boxes(augment.transform_boxes(f, s, a, *geo, w)[0], self.cfg.input_size)
                                 for (_, _, f), s, a, w in zip(ann[lo:hi], gsizes[lo:hi], aug, wins)]
        if self.color_on:
            p['color'] = augment.draw_color(self.color_rng, len(idxs), *self.color_jitter)[lo:hi]
        if mz is not None:
            self._plan_mosaic(p, idxs, gsizes, ann, aug_all, mz)
        return p

    def _plan_mosaic(self, p, idxs, gsizes, ann, aug_all, mz):
        """The mosaic half of a plan: the tile block (``'mosaic'`` int32 [n, 4, 9], source rows in this rank's (image, tile) order),
        ``'mosaic_index'`` int64 [n, 4] (dataset indices, -1 unused), the per-source draws ``'source_aug'`` int32 [S, 3] and dataset indices
        ``'source_index'`` int64 [S], this rank's slice of the draws themselves under ``'mosaic_draw'``, and for the mosaic
        images the merged ``'boxes'``, ``'class_ids'``, ``'ignore_boxes'`` and tile 0's meta in place of the plain ones.  An image whose own
        source has an unflagged box while the mosaic keeps none is demoted to the one-tile letterbox image of its own source (its plain
        plan: no draw is made), so mosaic never turns an image with objects into an object-free one."""
        lo, hi = self._local(idxs)
        src, own = self._sources(idxs, mz)
        n = hi - lo
        tiles = np.full((n, augment.MOSAIC_TILES, augment.TILE_INTS), -1, np.int32)
        index = np.full((n, augment.MOSAIC_TILES), -1, np.int64)
        saug = np.zeros((len(src), 3), np.int32)
        ignore = self.ignore_overlap is not None
        for j, k in enumerate(range(lo, hi)):
            saug[own[j]] = aug_all[k]
            tiles[j] = augment.one_tile(p['window'][j], own[j])
            index[j, 0] = int(idxs[k])
            if not mz['mosaic'][k]:
                continue
            parts = [int(q) for q in mz['partners'][k]]
            saug[own[j] + 1:own[j] + 4] = mz['aug'][k]
            entries = [(ann[k][0], ann[k][1], ann[k][2], gsizes[k], aug_all[k])]
            entries += [(mz['ann'][q][0], mz['ann'][q][1], mz['ann'][q][2], self._size_of(q), a) for q, a in zip(parts, mz['aug'][k])]
            drifted = [(s[0] - int(a[0]), s[1] - int(a[1])) for _, _, _, s, a in entries]
            t = augment.mosaic_tiles(drifted, mz['centre'][k], mz['scale'][k], self.cfg.input_size, own[j])
            c, bx, ign, meta = augment.transform_boxes_mosaic(entries, t, self.cfg.input_size, self.mosaic_min_visible, ignore)
            if len(bx) == 0 and len(ann[k][1]) > 0:
                continue                                  # the fallback: the plain one-tile plan stands
            tiles[j], index[j, 1:] = t, parts
            p['boxes'][j], p['class_ids'][j], p['metas'][j] = bx, c, meta
            if ignore:
                p['ignore_boxes'][j] = ign
        p.update(mosaic=tiles, mosaic_index=index, source_aug=saug, source_index=np.asarray(src, np.int64),
                 mosaic_draw={k: mz[k][lo:hi] for k in ('mosaic', 'partners', 'centre', 'scale', 'aug')})

    def plan(self):
        """One epoch's host side only (no pixels, no device): per batch this rank's dataset indices, draws, transformed boxes (jitter
        on: the colour factors under ``'color'``; ``cfg.letterbox``: the int32 [n, 4] windows under ``'window'``; ``cfg.ignore_overlap`` set: the transformed, clipped flagged boxes under ``'ignore_boxes'``; ``mosaic_prob > 0``: ``'mosaic'`` int32 [n, 4, 9] tiles and ``'mosaic_index'`` int64 [n, 4] dataset indices, -1 for unused, with ``'boxes'`` and ``'class_ids'`` the merged lists -- ``'window'`` stays the image's own letterbox window, the one of a one-tile image).  Consumes the loader's RandomStates exactly as iterating the epoch does."""
        for idxs in self._global_batches():
            mz = self._draw_mosaic(idxs)
            yield self._plan_batch(idxs, [self._size_of(int(i)) for i in idxs], [self.dataset.load_annotations(int(i)) for i in idxs], mz)

    def _emit(self, stage, idxs, prepared, mz=None):
        sizes, hdr, offsets, total, ann, gsizes = prepared
        lo, hi = self._local(idxs)
        p = self._plan_batch(idxs, gsizes, ann, mz)
        aug, tb, metas = p['aug'], p['boxes'], p['metas']
        color = p.get('color')
        if mz is None:
            augment.write_header(stage.np, offsets, sizes, aug, color, p.get('window'))
        else:
            augment.write_header(stage.np, offsets, sizes, p['source_aug'], color, tiles=p['mosaic'])
        B = hi - lo
        H, W = int(self.cfg.input_size[0]), int(self.cfg.input_size[1])
        dev_buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        dev_buf.copy_(stage.buf[:total], non_blocking=True)
        stage.copied = torch.cuda.Event()
        stage.copied.record(torch.cuda.current_stream(self.device))
        out = torch.empty(B, 3, H, W, device=self.device, dtype=torch.float32)
        if mz is None:
            augment.launch(dev_buf, B, hdr, self.cfg.input_size, out, self.forbid_resize, self.rgb_mean, self.rgb_std, color=color is not None,
                           letterbox=self.letterbox, window=self.letterbox)
        else:
            augment.launch_mosaic(dev_buf, B, len(sizes), hdr, self.cfg.input_size, out, self.rgb_mean, self.rgb_std, color=color is not None)
            sizes = gsizes[lo:hi]                         # (image_meta speaks of the output images' own sources)
        sparse = bool(getattr(self.cfg, 'sparse_gt', False))      # the positives as a list (ops.SparseGT): no dense tensor is built
        ignore = overflow = None
        if self.match is not None:
            gt, ignore, overflow = encode_annotations(p['class_ids'], tb, self.cfg.anchors, self.cfg.num_classes, device=self.device, dense=False,
                                                      ignore_boxes_list=p.get('ignore_boxes'), ignore_overlap=self.ignore_overlap,
                                                      match=self.match, return_overflow=True)
        elif self.ignore_overlap is not None:
            gt, ignore = encode_annotations(p['class_ids'], tb, self.cfg.anchors, self.cfg.num_classes, device=self.device, dense=False,
                                            ignore_boxes_list=p['ignore_boxes'], ignore_overlap=self.ignore_overlap)
        else:
            gt = encode_annotations(p['class_ids'], tb, self.cfg.anchors, self.cfg.num_classes, device=self.device, dense=not sparse)
        meta = augment.batch_meta(metas, sizes, self.rgb_mean, self.rgb_std)
        meta['index'] = p['index']
        if color is not None:
            meta['color'] = color
        if mz is not None:
            meta['mosaic'], meta['mosaic_index'] = p['mosaic'], p['mosaic_index']
        batch = {'image': out, 'image_meta': meta, 'gt_sparse' if sparse else 'gt': gt}
        if ignore is not None:
            batch['gt_ignore'] = ignore
        if overflow is not None:
            batch['gt_match_overflow'] = overflow
        return batch

    def __iter__(self):
        batches = self._global_batches()
        if not batches:
            return
        pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix='sqd-train') if self.workers > 0 else None
        try:
            mz = self._draw_mosaic(batches[0])
            pending = self._prepare(pool, self._stages[0], batches[0], mz)
            for it, idxs in enumerate(batches):
                prepared = pending()
                with torch.cuda.device(self.device):
                    batch = self._emit(self._stages[it % 2], idxs, prepared, mz)
                if it + 1 < len(batches):
                    mz = self._draw_mosaic(batches[it + 1])
                    pending = self._prepare(pool, self._stages[(it + 1) % 2], batches[it + 1], mz)
                yield batch
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)
