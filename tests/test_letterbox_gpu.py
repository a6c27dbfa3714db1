"""Letterbox and zoom-out on the MI355X ("Letterbox and zoom-out"): the three letterbox entry points
(sqd_preprocess_u8_letterbox_fwd / _aug_fwd / _aug_color_fwd) against the numpy restatement tests/letterbox_ref.py (oracle whitening,
drift and flip by slicing with a zero fill after whitening, oracle.resize_linear_f32 into a zero canvas), bitwise identity with the
resize kernel at an exact fit, host-given windows on and next to workgroup boundaries, colour, the way of the boxes back to the
original image through the detect kernels, the lane executor, and the TrainLoader with zoom-out feeding Trainer.run_epoch.

Bound of the pixel tests: atol 2e-5, rtol 0, the suite's own bar for the resize kernels against that oracle; the fill region is
compared exactly against +0.0 and every output buffer starts as NaN, so that an unwritten pixel fails."""
import numpy as np
import pytest
import torch

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment, synthetic
from squeezedet_pytorch_amd import boxes as host_boxes

import color_jitter_ref as cref
import letterbox_ref as lref

pytestmark = pytest.mark.gpu

MEAN, STD = lref.MEAN, lref.STD


def _images(sizes, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def _report(tag, out, ref):
    err = float(np.abs(out.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{tag}: max abs err {err:.3e}")
    return err


def _eval_launch(images, target):
    """preprocess_batch(letterbox=True) into a NaN-filled buffer: (out, scales, shifts, meta) as numpy."""
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    out = torch.full((len(images), 3, target[0], target[1]), float("nan"), device="cuda")
    x, (scales, shifts), meta = preprocess_batch(images, target, out=out, letterbox=True)
    torch.cuda.synchronize()
    assert x is out
    return out.cpu().numpy(), scales.cpu().numpy(), shifts.cpu().numpy(), meta


def _aug_launch(images, augs, target, win=None, color=None):
    """The training entry points through augment's packing: (out [B,3,H,W], scales [B,2], shifts [B,2]) as numpy.  ``win``: int32
    [B, 4] -> the window block of the header; None -> a null ``win`` (the kernel's own centred window)."""
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes, color is not None, win is not None)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    pk = buf.numpy()
    augment.write_header(pk, offsets, sizes, np.asarray(augs, np.int32), color, win)
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    dev = buf.cuda()
    out = torch.full((len(images), 3, target[0], target[1]), float("nan"), device="cuda")
    side = augment.launch(dev, len(images), hdr, target, out, False, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD, color=color is not None,
                          letterbox=True, window=win is not None)
    torch.cuda.synchronize()
    side = side.cpu().numpy()
    return out.cpu().numpy(), side[0], side[1]


def _augs_for(sizes, variant):                  # as tests/test_augment_gpu.py
    out = []
    for h, w in sizes:
        if variant == 0:
            out.append((min(h // 5, h - 1), min(w // 9, w - 1), 1))
        elif variant == 1:
            out.append((-(h // 4) - 1, -(w // 8) - 1, 0))
        else:
            out.append((-(h // 4) - 1, min(w // 9, w - 1), 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the eval kernel against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
EVAL_CASES = [
    # odd byte offsets, one-pixel sources, a portrait source whose side bars are wider than one 256-pixel workgroup, and (33 x 3001) a
    # 14-row window inside 384 rows: whole row groups are fill, one row group straddles each edge
    ([(33, 3001), (1, 1), (7, 1), (1, 9), (500, 375)], (384, 1248)),
    ([(40, 3000), (3, 2731)], (64, 96)),                          # segment larger than the LDS staging buffer: direct path
    ([(40, 2728), (41, 2729)], (64, 96)),                         # ... and just inside it
    ([(97, 300), (13, 1023)], (61, 517)),                         # canvas not a multiple of the workgroup tile
    ([(480, 640)], (96, 64)),                                     # a portrait canvas
]


@pytest.mark.parametrize("sizes,target", EVAL_CASES)
def test_eval_kernel_vs_reference(sizes, target):
    images = _images(sizes, 5)
    out, scales, shifts, meta = _eval_launch(images, target)
    for b, im in enumerate(images):
        ref, win, (hd, wd) = lref.reference(im, (0, 0, 0), target)
        _report(f"letterbox {sizes[b]} -> {target} window {win}", out[b], ref)
        np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0, err_msg=f"image {b} {sizes[b]}")
        lref.check_fill(out[b], win, target, f"image {b} {sizes[b]}")
        s, sh, pad = lref.scales_shifts_padding((hd, wd), win, target)
        assert np.array_equal(scales[b], s) and np.array_equal(shifts[b], sh), (b, scales[b], s, shifts[b], sh)
        assert meta["letterbox"][b].tolist() == list(win) and meta["letterbox"].dtype == np.int32
        assert np.array_equal(meta["scales"][b], s) and np.array_equal(meta["padding"][b], pad) and "crops" not in meta
    if target == (384, 1248):
        assert lref.window((33, 3001), target) == (185, 0, 14, 1248) and lref.window((500, 375), target) == (0, 480, 384, 288)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. an exact fit is the resize kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_fit_is_bitwise_the_resize_kernel():
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    target = (384, 1248)
    sizes = [(192, 624), (384, 1248)]                             # (375, 1242) does not fit exactly: h1 = 377
    images = _images(sizes, 2)
    out, scales, shifts, meta = _eval_launch(images, target)
    ref, scales_ref, _ = preprocess_batch(images, target)
    assert np.array_equal(out.view(np.uint32), ref.cpu().numpy().view(np.uint32))
    assert np.array_equal(scales, scales_ref.cpu().numpy())
    assert np.all(shifts == 0.0) and np.all(meta["padding"] == 0.0)
    assert meta["letterbox"].tolist() == [[0, 0, 384, 1248]] * 2
    # ... and the training form with the whole canvas as its window is the augmented resize kernel, drifted and flipped
    augs = _augs_for(sizes, 2)
    hdr, offsets, total = augment.pack_layout(sizes)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    augment.write_header(buf.numpy(), offsets, sizes, np.asarray(augs, np.int32))
    for im, off in zip(images, offsets):
        buf.numpy()[hdr + off:hdr + off + im.size] = im.reshape(-1)
    plain = torch.full((2, 3) + target, float("nan"), device="cuda")
    sc = augment.launch(buf.cuda(), 2, hdr, target, plain, False, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD)
    full = np.array([[0, 0, 384, 1248]] * 2, np.int32)
    o1, s1, h1 = _aug_launch(images, augs, target, win=full)
    assert np.array_equal(o1.view(np.uint32), plain.cpu().numpy().view(np.uint32)) and np.array_equal(s1, sc.cpu().numpy()) and np.all(h1 == 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. host-given windows with augmentation
# ---------------------------------------------------------------------------------------------------------------------------------
WIN_CANVAS = (64, 300)
WIN_SIZES = [(97, 300), (13, 1023), (40, 70), (70, 40)]
WINDOWS = {
    "one pixel in the last corner": (63, 299, 1, 1),
    "from column 255": (5, 255, 40, 45),                         # a workgroup boundary next to the edge
    "from column 256": (0, 256, 64, 44),                         # ... and on it
    "full height, one column": (0, 17, 64, 1),
    "centred": None,
}


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("kind", list(WINDOWS))
def test_given_windows_with_augmentation(kind, variant):
    images = _images(WIN_SIZES, 7)
    augs = _augs_for(WIN_SIZES, variant)
    drifted = [(h - a[0], w - a[1]) for (h, w), a in zip(WIN_SIZES, augs)]
    wins = np.array([WINDOWS[kind] or lref.window(d, WIN_CANVAS) for d in drifted], np.int32)
    out, scales, shifts = _aug_launch(images, augs, WIN_CANVAS, win=wins)
    for b, (im, a) in enumerate(zip(images, augs)):
        ref, win, size = lref.reference(im, a, WIN_CANVAS, wins[b])
        _report(f"{kind}: {WIN_SIZES[b]} aug {a} window {tuple(win)}", out[b], ref)
        np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0, err_msg=f"{kind} image {b} aug {a}")
        lref.check_fill(out[b], win, WIN_CANVAS, f"{kind} image {b}")
        s, sh, _pad = lref.scales_shifts_padding(size, win, WIN_CANVAS)
        assert np.array_equal(scales[b], s) and np.array_equal(shifts[b], sh), (kind, b)
    if kind == "centred":                                         # a null win is the same window
        o2, s2, h2 = _aug_launch(images, augs, WIN_CANVAS, win=None)
        assert np.array_equal(o2.view(np.uint32), out.view(np.uint32)) and np.array_equal(s2, scales) and np.array_equal(h2, shifts)


def test_a_window_outside_the_canvas_is_clamped_into_it():
    """The kernel clamps what the buffer holds (h1 to 1..H, w1 to 1..W, then top / left): every pixel is written, nothing out of range."""
    images = _images([(40, 70), (40, 70), (40, 70)], 3)
    bad = np.array([[-5, 290, 100, 50], [60, -9, 0, 0], [2 ** 30, 2 ** 30, 2 ** 30, -2 ** 30]], np.int32)
    want = [(0, 250, 64, 50), (60, 0, 1, 1), (0, 299, 64, 1)]
    out, scales, _ = _aug_launch(images, [(0, 0, 0)] * 3, WIN_CANVAS, win=bad)
    for b, im in enumerate(images):
        ref, win, size = lref.reference(im, (0, 0, 0), WIN_CANVAS, want[b])
        np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0)
        lref.check_fill(out[b], win, WIN_CANVAS, f"image {b}")
        assert np.array_equal(scales[b], lref.scales_shifts_padding(size, win, WIN_CANVAS)[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. colour
# ---------------------------------------------------------------------------------------------------------------------------------
def test_colour_identity_is_bitwise_and_a_real_triple_follows_the_rule():
    sizes, target = [(97, 300), (13, 1023), (300, 97)], (61, 517)
    images = _images(sizes, 5)
    for variant in (0, 2):
        augs = _augs_for(sizes, variant)
        drifted = [(h - a[0], w - a[1]) for (h, w), a in zip(sizes, augs)]
        wins = augment.draw_zoom(np.random.RandomState(variant), [lref.window(d, target) for d in drifted], target, 0.5)
        plain = _aug_launch(images, augs, target, win=wins)
        ones = _aug_launch(images, augs, target, win=wins, color=np.ones((len(images), 3), np.float32))
        assert np.array_equal(ones[0].view(np.uint32), plain[0].view(np.uint32))
        assert np.array_equal(ones[1], plain[1]) and np.array_equal(ones[2], plain[2])
        # bound: atol 2e-5, what tests/test_color_jitter_gpu.py holds its resize case to against the same float64 rule
        colors = np.float32([(1.4, 0.6, 1.7), (0.3, 1.9, 0.5), (1.8, 1., 1.)])       # per-tap, per-tap, table-only
        out, scales, shifts = _aug_launch(images, augs, target, win=wins, color=colors)
        for b, (im, a) in enumerate(zip(images, augs)):
            x = cref.whiten(cref.jitter(im, colors[b]), MEAN, STD).astype(np.float32)
            ref, win, _size = lref.reference(im, a, target, wins[b], x=x)
            _report(f"colour {tuple(colors[b])} {sizes[b]} aug {a} window {tuple(win)}", out[b], ref)
            np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0, err_msg=f"image {b} color {colors[b]}")
            lref.check_fill(out[b], win, target, f"colour image {b}")
        assert np.array_equal(scales, plain[1]) and np.array_equal(shifts, plain[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. boxes come home
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = (128, 256)
MIXED = [(200, 150), (150, 200), (375, 500), (128, 256), (90, 300), (300, 90)]


def _detector(**over):
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    cfg = sqd.make_cfg(input_size=SMALL, score_thresh=0.05, **over)
    cfg.batch_size = 3
    m = SqueezeDet(cfg)
    m.load_state_dict(synthetic.make_state_dict())
    return Detector(m, cfg), cfg


def _scene_images(sizes, seed):
    rs = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        base = rs.standard_normal((-(-h // 8), -(-w // 8), 3)) * 60 + 100
        out.append(np.clip(np.kron(base, np.ones((8, 8, 1))), 0, 255).astype(np.uint8)[:h, :w])
    return out


def _same(r, w):
    assert ("boxes" in r) == ("boxes" in w)
    if "boxes" in r:
        for k in ("anchor_idx", "boxes", "scores", "class_ids"):
            assert np.array_equal(r[k], w[k]) and r[k].dtype == w[k].dtype, k
    assert sorted(k for k in r["image_meta"] if k != "index") == sorted(k for k in w["image_meta"] if k != "index")
    for k in ("orig_size", "scales", "padding", "crops", "letterbox"):
        if k in w["image_meta"]:
            assert np.array_equal(np.asarray(r["image_meta"][k]), np.asarray(w["image_meta"][k])), k


@pytest.fixture(scope="module")
def small():
    det, cfg = _detector(letterbox=True)
    images = _scene_images(MIXED, 3)
    return det, cfg, images, det.detect_images(images)


def test_detect_images_equals_host_postprocess_of_detect_device(small):
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    det, cfg, images, res = small
    x, (scales, shifts), meta = preprocess_batch(images, SMALL, letterbox=True)
    cnt, cls, sc, bx, idx = (t.cpu().numpy() for t in det.detect_device(x))                   # network-input coordinates
    ndet = 0
    for b, r in enumerate(res):
        n = int(cnt[b])
        assert ("boxes" in r) == (n > 0)
        m = r["image_meta"]
        win = lref.window(MIXED[b], SMALL)
        s, _sh, pad = lref.scales_shifts_padding(MIXED[b], win, SMALL)
        assert np.array_equal(m["scales"], s) and np.array_equal(m["padding"], pad) and m["letterbox"].tolist() == list(win) and "crops" not in m
        if n:
            want = host_boxes.boxes_postprocess(bx[b, :n].copy(), {k: meta[k][b] for k in ("scales", "padding", "letterbox")})
            assert np.array_equal(r["boxes"], want), b                                       # bit for bit
            assert np.array_equal(want, oracle.boxes_unpad_uncrop(oracle.boxes_postprocess(bx[b, :n], s), pad, np.zeros(4, np.float32)))
            assert np.array_equal(r["anchor_idx"], idx[b, :n]) and np.array_equal(r["scores"], sc[b, :n]) and np.array_equal(r["class_ids"], cls[b, :n])
            ndet += n
    assert ndet > 10
    # Detector.detect on a batch that carries this meta takes the host route of boxes_postprocess: the same results
    res2 = det.detect({"image": x, "image_meta": dict(meta, index=np.arange(len(images)))})
    for r, r2 in zip(res, res2):
        assert ("boxes" in r) == ("boxes" in r2)
        if "boxes" in r:
            assert np.array_equal(r["boxes"], r2["boxes"]) and np.array_equal(r["anchor_idx"], r2["anchor_idx"])


def test_detect_stream_equals_detect_images_and_follows_the_mode(small):
    det, cfg, images, _res = small
    batches = [images[0:3], images[3:6], images[1:4], images[2:5], images[0:3]]      # 2 lanes: eager, eager, capture, capture, replay
    want = {True: [det.detect_images(b) for b in batches]}
    got = list(det.detect_stream(batches))
    ex = det.stream()
    assert ex.letterbox and not ex.degraded and ex.replayed_batches >= 1
    for res, w in zip(got, want[True]):
        for r, x in zip(res, w):
            _same(r, x)
    # the other mode on the same Detector: its own results, not a replay of the letterbox step -- and back
    cfg.letterbox = False
    want[False] = [det.detect_images(b) for b in batches]
    got = list(det.detect_stream(batches))
    assert det.stream() is not ex and not det.stream().letterbox
    differs = 0
    for res, w, wl in zip(got, want[False], want[True]):
        for r, x, xl in zip(res, w, wl):
            _same(r, x)
            assert "letterbox" not in r["image_meta"] and "padding" not in r["image_meta"]
            differs += ("boxes" in x) != ("boxes" in xl) or ("boxes" in x and (x["boxes"].shape != xl["boxes"].shape or not np.array_equal(x["boxes"], xl["boxes"])))
    assert differs > 0
    cfg.letterbox = True
    assert det.stream() is ex
    for res, w in zip(list(det.detect_stream(batches)), want[True]):
        for r, x in zip(res, w):
            _same(r, x)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. training
# ---------------------------------------------------------------------------------------------------------------------------------
class _MixedDataset:
    """Portrait and landscape images with 1 .. 3 boxes each and (``flags``) one more, flagged, box per image."""

    def __init__(self, n, flags=False, seed=0, sizes=((120, 250), (250, 120), (117, 241), (200, 90))):
        rs = np.random.RandomState(seed)
        self.images, self.ann = [], []
        for i in range(n):
            h, w = sizes[i % len(sizes)]
            self.images.append(rs.randint(0, 256, (h, w, 3), dtype=np.uint8))
            m = int(rs.randint(1, 4)) + int(flags)
            x1 = rs.uniform(0, w * 0.6, m); y1 = rs.uniform(0, h * 0.6, m)
            b = np.stack([x1, y1, x1 + rs.uniform(8, w * 0.4, m), y1 + rs.uniform(8, h * 0.4, m)], 1).astype(np.float32)
            f = np.zeros(m, np.uint8)
            f[-1] = int(flags)
            self.ann.append((rs.randint(0, 3, m).astype(np.int64), b, f))
        self.flags = flags
        self.rgb_mean, self.rgb_std = MEAN, STD

    def __len__(self):
        return len(self.images)

    def load_image(self, i):
        return self.images[i], f"{i:06d}"

    def load_annotations(self, i):
        c, b, f = self.ann[i]
        return (c.copy(), b.copy(), f.copy()) if self.flags else (c.copy(), b.copy())


@pytest.mark.parametrize("sparse", [False, True])
def test_loader_with_zoom_out_feeds_trainer_run_epoch(sparse):
    from squeezedet_pytorch_amd import ops
    from squeezedet_pytorch_amd.annotations import encode_annotations
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import Trainer
    kw = dict(sparse_gt=True, ignore_overlap=0.5) if sparse else {}
    cfg = sqd.make_cfg(input_size=SMALL, device="cuda", batch_size=4, num_workers=2, dropout_prob=0.0, letterbox=True, zoom_out=0.5, **kw)
    cfg.num_iters, cfg.print_interval = 2, 1000
    ds = _MixedDataset(8, flags=sparse)
    plans = list(TrainLoader(ds, cfg, seed=7).plan())
    batches = list(TrainLoader(ds, cfg, seed=7))
    assert len(batches) == len(plans) == 2
    for batch, p in zip(batches, plans):
        meta = batch["image_meta"]
        assert np.array_equal(meta["index"], p["index"]) and np.array_equal(meta["letterbox"], p["window"])
        assert np.any(p["window"][:, 2:] < np.array([lref.window((ds.images[i].shape[0] - a[0], ds.images[i].shape[1] - a[1]), SMALL)[2:]
                                                    for i, a in zip(p["index"], p["aug"])]))       # zoomed out
        img = batch["image"].cpu().numpy()
        for b, (i, a, w) in enumerate(zip(p["index"], p["aug"], p["window"])):
            ref, win, size = lref.reference(ds.images[int(i)], a, SMALL, w)
            _report(f"loader image {int(i)} aug {tuple(a)} window {tuple(win)}", img[b], ref)
            np.testing.assert_allclose(img[b], ref, atol=2e-5, rtol=0)
            lref.check_fill(img[b], win, SMALL, f"loader image {int(i)}")
            s, _sh, pad = lref.scales_shifts_padding(size, win, SMALL)
            assert np.array_equal(meta["scales"][b], s) and np.array_equal(meta["padding"][b], pad)
            # every box is still on the canvas, inside the window (zoom-out never loses one)
            bx = p["boxes"][b]
            assert len(bx) == len(ds.ann[int(i)][1]) - int(sparse)
            assert np.all(bx[:, 0] >= win[1] - 1e-3) and np.all(bx[:, 2] <= win[1] + win[3]) and np.all(bx[:, 1] >= win[0] - 1e-3) and np.all(bx[:, 3] <= win[0] + win[2])
        if sparse:
            want, bits = encode_annotations(p["class_ids"], p["boxes"], cfg.anchors, cfg.num_classes, device="cuda", dense=False,
                                            ignore_boxes_list=p["ignore_boxes"], ignore_overlap=0.5)
            assert isinstance(batch["gt_sparse"], ops.SparseGT) and all(torch.equal(x, y) for x, y in zip(batch["gt_sparse"], want))
            assert torch.equal(batch["gt_ignore"], bits) and sum(len(r) for r in p["ignore_boxes"]) >= 1       # (one flagged box per image)
        else:
            assert torch.equal(batch["gt"], encode_annotations(p["class_ids"], p["boxes"], cfg.anchors, cfg.num_classes, device="cuda"))
            # ... and the batch is preprocess_train_batch on the same images with the loader's draws and windows
            idx = [int(i) for i in p["index"]]
            x, m, gt = augment.preprocess_train_batch([ds.images[i] for i in idx], [ds.ann[i][0] for i in idx], [ds.ann[i][1] for i in idx], SMALL,
                                                      None, device="cuda", anchors=cfg.anchors, aug=p["aug"], rgb_mean=MEAN, rgb_std=STD,
                                                      letterbox=True, window=p["window"])
            assert torch.equal(x, batch["image"]) and torch.equal(gt, batch["gt"])
            assert np.array_equal(m["letterbox"], p["window"]) and np.array_equal(m["padding"], meta["padding"])
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict("squeezedet", seed=1234), strict=True)
    opt = torch.optim.SGD(m.parameters(), lr=0.001, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m.cuda(), opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
    stats = tr.run_epoch("train", 1, TrainLoader(ds, cfg, seed=1))
    for k in ("loss", "class_loss", "score_loss", "bbox_loss"):
        assert np.isfinite(stats[k]), (k, stats)
    assert stats["loss"] > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. the one Python dispatch puts every entry's arguments where the entry reads them
# ---------------------------------------------------------------------------------------------------------------------------------
def test_launch_u8_is_bitwise_a_direct_call_of_each_of_the_nine_entries():
    """``preprocess.launch_u8`` for every (geometry, aug, colour) against a ctypes call of the same entry whose arguments are written out
    here by hand, in include/sqd_hip.h's order: outputs and side outputs bit for bit (both start as NaN / -1, so an output the dispatch
    left out or swapped differs).  The numbers themselves are held by the tests above and by the other input-kernel modules."""
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd.preprocess import c_float3, launch_u8
    H, W = 64, 96
    images = _images([(9, 5), (50, 61), (123, 77)], 11)
    B = len(images)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    src = t(np.concatenate([im.reshape(-1) for im in images]))
    offsets = t(np.cumsum([0] + [im.size for im in images[:-1]]).astype(np.int64))
    sizes = t(np.array([im.shape[:2] for im in images], np.int32))
    aug = t(np.array([(0, 0, 0), (-7, 5, 1), (3, -11, 0)], np.int32))
    color = t(np.array([(1., 1., 1.), (1.25, 0.75, 1.5), (0.5, 1.5, 0.25)], np.float32))
    sums = t(np.array([[(int(im[..., c].astype(np.int64).sum()), int((im[..., c].astype(np.int64) ** 2).sum())) for c in range(3)]
                       for im in images], np.int64))                     # as sqd_image_stats_u8 writes them
    win = t(np.array([(5, 7, 40, 70)] * B, np.int32))                    # strictly inside the canvas
    mean, std = c_float3(oracle.KITTI_RGB_MEAN), c_float3(oracle.KITTI_RGB_STD)
    lib, p, st = nat.lib(), nat.ptr, nat.stream_handle(dev)

    def fresh():
        return {"out": torch.full((B, 3, H, W), float("nan"), device=dev), "scales": torch.full((B, 2), float("nan"), device=dev),
                "shifts": torch.full((B, 2), float("nan"), device=dev), "padcrop": torch.full((B, 8), -1, dtype=torch.int32, device=dev)}

    direct = {
        "sqd_preprocess_u8_fwd": lambda o: lib.sqd_preprocess_u8_fwd(
            p(src), p(offsets), p(sizes), p(o["out"]), p(o["scales"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_aug_fwd": lambda o: lib.sqd_preprocess_u8_aug_fwd(
            p(src), p(offsets), p(sizes), p(aug), p(o["out"]), p(o["scales"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_aug_color_fwd": lambda o: lib.sqd_preprocess_u8_aug_color_fwd(
            p(src), p(offsets), p(sizes), p(aug), p(color), p(sums), p(o["out"]), p(o["scales"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_padcrop_fwd": lambda o: lib.sqd_preprocess_u8_padcrop_fwd(
            p(src), p(offsets), p(sizes), p(o["out"]), p(o["shifts"]), p(o["padcrop"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_padcrop_aug_fwd": lambda o: lib.sqd_preprocess_u8_padcrop_aug_fwd(
            p(src), p(offsets), p(sizes), p(aug), p(o["out"]), p(o["shifts"]), p(o["padcrop"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_padcrop_aug_color_fwd": lambda o: lib.sqd_preprocess_u8_padcrop_aug_color_fwd(
            p(src), p(offsets), p(sizes), p(aug), p(color), p(sums), p(o["out"]), p(o["shifts"]), p(o["padcrop"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_letterbox_fwd": lambda o: lib.sqd_preprocess_u8_letterbox_fwd(
            p(src), p(offsets), p(sizes), p(win), p(o["out"]), p(o["scales"]), p(o["shifts"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_letterbox_aug_fwd": lambda o: lib.sqd_preprocess_u8_letterbox_aug_fwd(
            p(src), p(offsets), p(sizes), p(aug), p(win), p(o["out"]), p(o["scales"]), p(o["shifts"]), mean, std, B, H, W, st),
        "sqd_preprocess_u8_letterbox_aug_color_fwd": lambda o: lib.sqd_preprocess_u8_letterbox_aug_color_fwd(
            p(src), p(offsets), p(sizes), p(aug), p(win), p(color), p(sums), p(o["out"]), p(o["scales"]), p(o["shifts"]), mean, std,
            B, H, W, st),
    }
    side_of = {"resize": ("scales",), "padcrop": ("shifts", "padcrop"), "letterbox": ("scales", "shifts")}
    stem = {"resize": "sqd_preprocess_u8", "padcrop": "sqd_preprocess_u8_padcrop", "letterbox": "sqd_preprocess_u8_letterbox"}
    seen = {}
    for geometry, keys in side_of.items():
        for suffix, blocks in (("_fwd", {}), ("_aug_fwd", {"aug": aug}), ("_aug_color_fwd", {"aug": aug, "color": color, "sums": sums})):
            name = stem[geometry] + suffix
            got, want = fresh(), fresh()
            launch_u8(geometry, src, offsets, sizes, got["out"], B, H, W, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD, dev,
                      **blocks, **({"win": win} if geometry == "letterbox" else {}), **{k: got[k] for k in keys})
            assert direct[name](want) == 0, name
            torch.cuda.synchronize()
            for k in ("out", "scales", "shifts", "padcrop"):
                g, w = got[k].cpu().numpy(), want[k].cpu().numpy()
                assert np.array_equal(g.view(np.int32), w.view(np.int32)), (name, k)
                written = not (np.isnan(g).any() if g.dtype == np.float32 else (g == -1).any())
                assert written == (k == "out" or k in keys), (name, k)           # every output of the entry, and no other
            seen[name] = got["out"].cpu().numpy()
    assert sorted(seen) == sorted(direct)
    # the nine are nine different launches: no two combinations ran the same entry (the identity colour row aside, every image differs)
    names = sorted(seen)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(seen[a], seen[b]), (a, b)
