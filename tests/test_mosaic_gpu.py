"""Mosaic on the MI355X ("Mosaic"): the two mosaic entry points (sqd_preprocess_u8_mosaic_aug_fwd / _aug_color_fwd) against
the numpy restatement tests/mosaic_ref.py, their bitwise identities with the letterbox kernels and with themselves, colour with one pivot
per source, hostile tile blocks (a clamp check on well-defined input), and the TrainLoader with mosaic feeding Trainer.run_epoch and the
captured training step.

Bound of the pixel tests: atol 2e-5, rtol 0, the suite's own bar for the resize kernels against that oracle; the fill region is
compared exactly against +0.0 and every output buffer starts as NaN, so that an unwritten pixel fails."""
import numpy as np
import pytest
import torch

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment, synthetic

import mosaic_ref as mref
from test_letterbox_gpu import _MixedDataset, _aug_launch, _augs_for, _images

pytestmark = pytest.mark.gpu

MEAN, STD = mref.lref.MEAN, mref.lref.STD
CANVAS = (64, 300)
SIZES = [(97, 300), (13, 1023), (40, 70), (70, 40), (1, 1)]
ATOL = 2e-5


def _launch(images, augs, tiles, target, color=None):
    """The mosaic entry points through augment's packing: out [B, 3, H, W] as numpy.  ``tiles``: raw int rows [B, 4, 9], written as they are."""
    tiles = np.asarray(tiles, np.int32).reshape(-1, 4, 9)
    B, S = tiles.shape[0], len(images)
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes, color is not None, tiles=B)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    pk = buf.numpy()
    augment.write_header(pk, offsets, sizes, np.asarray(augs, np.int32), color, tiles=tiles)
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    out = torch.full((B, 3, target[0], target[1]), float("nan"), device="cuda")
    augment.launch_mosaic(buf.cuda(), B, S, hdr, target, out, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD, color=color is not None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(out, images, augs, tiles, target, tag, color=None):
    worst = 0.0
    for b in range(len(tiles)):
        ref, owner = mref.compose(images, augs, tiles[b], target, None if color is None else color[b])
        assert not np.isnan(out[b]).any(), f"{tag} image {b}: a pixel was not written"
        worst = max(worst, float(np.abs(out[b].astype(np.float64) - ref).max()))
        np.testing.assert_allclose(out[b], ref, atol=ATOL, rtol=0, err_msg=f"{tag} image {b} tiles {np.asarray(tiles[b]).tolist()}")
        mref.check_fill(out[b], owner, f"{tag} image {b}")
    print(f"{tag}: {len(tiles)} images, max abs err {worst:.3e}")


def _drifted(sizes, augs):
    return [(h - a[0], w - a[1]) for (h, w), a in zip(sizes, augs)]


def _four_tile_rows(sizes, augs, pick, centre, zooms, canvas):
    """mref.tiles_of for the sources ``pick`` (four indices into ``sizes``), with the src column naming them."""
    d = _drifted(sizes, augs)
    rows = np.array(mref.tiles_of([d[s] for s in pick], centre, zooms, canvas), np.int32)
    rows[:, 0] = pick
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. four-tile images against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
CX, CY, ZOOMS = (1, 255, 256, 257, 299), (1, 3, 4, 5, 63), (0.5, 1.0, 2.0)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_four_tile_images_vs_reference(variant):
    """Every (cy, cx) of the seam grid -- on and beside the 256-column and 4-row workgroup edges and one pixel inside each canvas edge --,
    each tile seeing every zoom of {0.5, 1, 2} (windows hang over every canvas side), the sources rotating through the five images."""
    images = _images(SIZES, 7)
    augs = _augs_for(SIZES, variant)
    tiles, i = [], 0
    for cy in CY:
        for cx in CX:
            pick = [(i + t) % len(SIZES) for t in range(4)]
            zooms = [ZOOMS[(i + t) % 3] for t in range(4)]
            tiles.append(_four_tile_rows(SIZES, augs, pick, (cy, cx), zooms, CANVAS))
            i += 1
    tiles = np.stack(tiles)
    assert (tiles[:, :, 1] < 0).any() and (tiles[:, :, 2] < 0).any()                                   # over the top and the left ...
    assert (tiles[:, :, 1] + tiles[:, :, 3] > CANVAS[0]).any() and (tiles[:, :, 2] + tiles[:, :, 4] > CANVAS[1]).any()      # ... bottom and right
    out = _launch(images, augs, tiles, CANVAS)
    _check(out, images, augs, tiles, CANVAS, f"four tiles, variant {variant}")


@pytest.mark.parametrize("sizes,canvas,centre", [
    ([(97, 300), (13, 1023), (40, 70), (70, 40)], (61, 517), (30, 258)),      # canvas not a multiple of the workgroup tile
    ([(3, 2731), (40, 3000), (3, 2731), (40, 70)], (64, 96), (31, 50)),       # a source row segment beyond the LDS staging size: direct path
])
def test_ragged_canvas_and_the_direct_path(sizes, canvas, centre):
    images = _images(sizes, 5)
    for variant in (0, 1):
        augs = _augs_for(sizes, variant)
        tiles = np.stack([_four_tile_rows(sizes, augs, [0, 1, 2, 3], centre, z, canvas) for z in ([1.0] * 4, [2.0, 0.5, 1.0, 2.0])])
        out = _launch(images, augs, tiles, canvas)
        _check(out, images, augs, tiles, canvas, f"{sizes[0]} -> {canvas} variant {variant}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. bitwise identities
# ---------------------------------------------------------------------------------------------------------------------------------
def test_one_tile_images_are_bitwise_the_letterbox_kernel():
    sizes = SIZES[:4]
    images = _images(sizes, 7)
    for variant in (0, 1, 2):
        augs = _augs_for(sizes, variant)
        wins = np.array([(63, 299, 1, 1), (5, 255, 40, 45), (0, 256, 64, 44), mref.lref.window(_drifted(sizes, augs)[3], CANVAS)], np.int32)
        tiles = np.stack([augment.one_tile(w, s) for s, w in enumerate(wins)])
        want = _aug_launch(images, augs, CANVAS, win=wins)[0]
        got = _launch(images, augs, tiles, CANVAS)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), variant
        colors = np.float32([(1.4, 0.6, 1.7), (0.3, 1.9, 0.5), (1.8, 1., 1.), (1., 1., 1.)])
        want = _aug_launch(images, augs, CANVAS, win=wins, color=colors)[0]
        got = _launch(images, augs, tiles, CANVAS, color=colors)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (variant, "colour")
    # ... and a window covering the whole canvas is the augmented resize kernel
    full = np.array([(0, 0) + CANVAS] * 4, np.int32)
    hdr, offsets, total = augment.pack_layout(sizes)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    augment.write_header(buf.numpy(), offsets, sizes, np.asarray(augs, np.int32))
    for im, off in zip(images, offsets):
        buf.numpy()[hdr + off:hdr + off + im.size] = im.reshape(-1)
    plain = torch.full((4, 3) + CANVAS, float("nan"), device="cuda")
    augment.launch(buf.cuda(), 4, hdr, CANVAS, plain, False, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD)
    got = _launch(images, augs, np.stack([augment.one_tile(w, s) for s, w in enumerate(full)]), CANVAS)
    assert np.array_equal(got.view(np.uint32), plain.cpu().numpy().view(np.uint32))


def _mixed_tiles(sizes, augs):
    four = _four_tile_rows(sizes, augs, [0, 1, 2, 3], (30, 256), [1.0, 2.0, 0.5, 1.0], CANVAS)
    other = _four_tile_rows(sizes, augs, [3, 2, 1, 0], (5, 130), [2.0, 1.0, 1.0, 0.5], CANVAS)
    tiles = np.full((4, 4, 9), -1, np.int32)
    tiles[0, :1] = augment.one_tile((5, 255, 40, 45), 2)[:1]
    tiles[1, :2] = four[[0, 3]]
    tiles[2, :3] = other[[1, 2, 3]]
    tiles[3] = four
    return tiles


def test_identity_colour_and_each_image_launched_alone():
    sizes = SIZES[:4]
    images = _images(sizes, 9)
    augs = _augs_for(sizes, 2)
    tiles = _mixed_tiles(sizes, augs)
    assert [augment.tile_count(t) for t in tiles] == [1, 2, 3, 4]
    plain = _launch(images, augs, tiles, CANVAS)
    ones = _launch(images, augs, tiles, CANVAS, color=np.ones((4, 3), np.float32))
    assert np.array_equal(ones.view(np.uint32), plain.view(np.uint32))
    _check(plain, images, augs, tiles, CANVAS, "mixed tile counts")
    colors = np.float32([(1.4, 0.6, 1.7), (0.3, 1.9, 0.5), (1.8, 1., 1.), (0.7, 1.2, 1.3)])
    tinted = _launch(images, augs, tiles, CANVAS, color=colors)
    for b in range(4):
        alone = _launch(images, augs, tiles[b:b + 1], CANVAS)
        assert np.array_equal(alone[0].view(np.uint32), plain[b].view(np.uint32)), b
        alone = _launch(images, augs, tiles[b:b + 1], CANVAS, color=colors[b:b + 1])
        assert np.array_equal(alone[0].view(np.uint32), tinted[b].view(np.uint32)), (b, "colour")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. colour: the pivot is each source's own
# ---------------------------------------------------------------------------------------------------------------------------------
def test_colour_uses_each_sources_own_pivot():
    sizes = SIZES[:4]
    rs = np.random.RandomState(3)
    spans = [(0, 60), (190, 256), (60, 140), (120, 256)]                     # four sources of clearly different mean luma
    images = [rs.randint(lo, hi, (h, w, 3), dtype=np.uint8) for (h, w), (lo, hi) in zip(sizes, spans)]
    lumas = [float(mref.cref.mean_luma(im)) for im in images]
    assert min(abs(a - b) for i, a in enumerate(lumas) for b in lumas[i + 1:]) > 20
    augs = _augs_for(sizes, 0)
    rows = _four_tile_rows(sizes, augs, [0, 1, 2, 3], (30, 256), [1.0, 1.0, 2.0, 0.5], CANVAS)
    tiles = np.stack([rows, rows])
    colors = np.float32([(1.4, 0.6, 1.7), (1.3, 0.5, 1.)])                   # per-tap, table-only; contrast != 1: the pivot matters
    out = _launch(images, augs, tiles, CANVAS, color=colors)
    _check(out, images, augs, tiles, CANVAS, "colour, four pivots", color=colors)
    # a pivot taken from the wrong source would move a table-only pixel by (1 - fc) |p0 - p1| / std: far more than the bound
    p0, p1 = mref.cref.pivot(images[0], colors[1]), mref.cref.pivot(images[1], colors[1])
    assert abs(p0 - p1) * (1 - colors[1][1]) / 81.2 > 100 * ATOL


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. hostile tile blocks: every pixel is written, and equals the reference built from the clamped tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hostile_tile_blocks_are_clamped():
    sizes = SIZES[:4]
    images = _images(sizes, 3)
    augs = _augs_for(sizes, 1)
    big = 2 ** 30
    tiles = np.full((6, 4, 9), -1, np.int32)
    # src past the last source (clamped to it); a window far larger than the canvas and far outside on the negative side
    tiles[0, 0] = (99, -70000, -70000, big, big, 0, 0, 40, 200)
    tiles[0, 1] = (2 ** 31 - 1, 10, 20, 30, 40, 0, 0, big, big)
    # negative and zero window sizes (clamped to 1), a rectangle outside canvas and window (clamped to empty), first owner on overlaps
    tiles[1, 0] = (1, 5, 7, -3, 0, -big, -big, big, big)
    tiles[1, 1] = (0, 0, 0, 64, 300, 70, 310, 90, 400)
    tiles[1, 2] = (2, -10, 100, 60, 150, 0, 0, 64, 300)
    tiles[1, 3] = (3, 0, 0, 64, 300, 0, 0, 64, 300)
    # overlapping rectangles, each inside its window: the first of the list owns the overlap
    tiles[2, 0] = (0, 0, 0, 64, 300, 10, 10, 40, 270)
    tiles[2, 1] = (1, -20, -30, 120, 400, 0, 0, 64, 300)
    # a rectangle turned inside out, then a normal tile
    tiles[3, 0] = (0, 0, 0, 64, 300, 40, 200, 10, 20)
    tiles[3, 1] = (3, 20, 250, 70, 40, 0, 0, 64, 300)
    # an empty list (tiles[4]); a list ended after one tile with rubbish behind the end mark
    tiles[5, 0] = (2, 3, 3, 40, 70, 3, 3, 43, 73)
    tiles[5, 2] = (0, 0, 0, 64, 300, 0, 0, 64, 300)
    want = [mref.clamp_tiles(t, len(images), CANVAS) for t in tiles]
    assert want[0] == [(3, 10, 20, 30, 40, 10, 20, 40, 60)]                  # (tile 0 clamps to an empty rectangle)
    assert [w[0] for w in want[1]] == [1, 2, 3] and want[1][0][1:] == (5, 7, 1, 1, 5, 7, 6, 8)
    assert want[4] == [] and len(want[5]) == 1 and len(want[3]) == 1
    out = _launch(images, augs, tiles, CANVAS)
    _check(out, images, augs, tiles, CANVAS, "hostile tiles")
    assert np.array_equal(out[4], np.zeros_like(out[4])) and not np.signbit(out[4]).any()
    colors = np.float32([(1.4, 0.6, 1.7)] * 6)
    _check(_launch(images, augs, tiles, CANVAS, color=colors), images, augs, tiles, CANVAS, "hostile tiles, colour", color=colors)


def test_a_huge_window_shows_its_clamped_form():
    """A window of 2^30 x 2^30 around the canvas is the 65535 x 65535 one: the canvas shows a 64 x 300 block of it."""
    images = _images([(40, 70)], 4)
    tiles = np.full((1, 4, 9), -1, np.int32)
    tiles[0, 0] = (0, -30000, -20000, 2 ** 30, 2 ** 30, 0, 0, 64, 300)
    assert mref.clamp_tiles(tiles[0], 1, CANVAS) == [(0, -30000, -20000, 65535, 65535, 0, 0, 64, 300)]
    _check(_launch(images, [(3, -5, 1)], tiles, CANVAS), images, [(3, -5, 1)], tiles, CANVAS, "huge window")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the loader, the trainer, the captured step
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = (128, 256)


def _loader_cfg(form, **kw):
    extra = {"dense": {}, "sparse": dict(sparse_gt=True), "masked": dict(sparse_gt=True, ignore_overlap=0.5)}[form]
    cfg = sqd.make_cfg(input_size=SMALL, device="cuda", batch_size=4, num_workers=2, dropout_prob=0.0, letterbox=True, **extra, **kw)
    cfg.num_iters, cfg.print_interval = 2, 1000
    return cfg


@pytest.mark.parametrize("form,kw", [("dense", dict(mosaic_prob=1.0)), ("sparse", dict(mosaic_prob=1.0)),
                                     ("masked", dict(mosaic_prob=1.0, mosaic_min_visible=0.6)),
                                     ("dense", dict(mosaic_prob=0.5, zoom_out=0.5, brightness_jitter=0.3, contrast_jitter=0.3))])
def test_loader_with_mosaic_feeds_trainer_run_epoch(form, kw):
    from squeezedet_pytorch_amd import ops
    from squeezedet_pytorch_amd.annotations import encode_annotations
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import Trainer
    cfg = _loader_cfg(form, **kw)
    ds = _MixedDataset(8, flags=form == "masked")
    plans = list(TrainLoader(ds, cfg, seed=7).plan())
    batches = list(TrainLoader(ds, cfg, seed=7))
    assert len(batches) == len(plans) == 2
    counts = []
    for batch, p in zip(batches, plans):
        meta = batch["image_meta"]
        for k in ("index", "mosaic", "mosaic_index"):
            assert np.array_equal(meta[k], p[k]) and meta[k].dtype == p[k].dtype, k
        assert p["mosaic"].shape == (4, 4, 9) and p["mosaic"].dtype == np.int32 and p["mosaic_index"].dtype == np.int64
        assert np.array_equal(p["mosaic_index"][:, 0], p["index"])
        counts += [augment.tile_count(t) for t in p["mosaic"]]
        srcs = [ds.images[int(i)] for i in p["source_index"]]
        color = p.get("color")
        img = batch["image"].cpu().numpy()
        _check(img, srcs, p["source_aug"], p["mosaic"], SMALL, f"loader {form} {kw}", color=color)
        for b, t in enumerate(p["mosaic"]):
            if augment.tile_count(t) == 1:
                assert np.array_equal(t[0, 1:5], p["window"][b]) and np.array_equal(meta["letterbox"][b], p["window"][b])
            else:
                assert np.array_equal(meta["letterbox"][b], t[0, 1:5])
                assert np.array_equal(p["mosaic_index"][b], [ds_i for ds_i in p["source_index"][t[:, 0]]])
        if form == "masked":
            want, bits = encode_annotations(p["class_ids"], p["boxes"], cfg.anchors, cfg.num_classes, device="cuda", dense=False,
                                            ignore_boxes_list=p["ignore_boxes"], ignore_overlap=0.5)
            assert all(torch.equal(x, y) for x, y in zip(batch["gt_sparse"], want)) and torch.equal(batch["gt_ignore"], bits)
        elif form == "sparse":
            want = encode_annotations(p["class_ids"], p["boxes"], cfg.anchors, cfg.num_classes, device="cuda", dense=False)
            assert isinstance(batch["gt_sparse"], ops.SparseGT) and all(torch.equal(x, y) for x, y in zip(batch["gt_sparse"], want))
        else:
            assert torch.equal(batch["gt"], encode_annotations(p["class_ids"], p["boxes"], cfg.anchors, cfg.num_classes, device="cuda"))
            # ... and the batch is preprocess_train_batch on the same sources with the loader's draws and tiles
            idx = [int(i) for i in p["source_index"]]
            x, m, _gt = augment.preprocess_train_batch([ds.images[i] for i in idx], [ds.ann[i][0] for i in idx], [ds.ann[i][1] for i in idx], SMALL,
                                                       None, device="cuda", anchors=cfg.anchors, aug=p["source_aug"], rgb_mean=MEAN, rgb_std=STD,
                                                       letterbox=True, tiles=p["mosaic"], sources=p["mosaic_index"], color=color,
                                                       mosaic_min_visible=cfg.mosaic_min_visible)
            assert torch.equal(x, batch["image"]) and torch.equal(_gt, batch["gt"]) and np.array_equal(m["mosaic_index"], p["mosaic_index"])
    if kw["mosaic_prob"] == 1.0:
        assert counts.count(4) >= 6, counts                                  # (a fallback may demote one)
    else:
        assert 1 in counts and 4 in counts, counts
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict("squeezedet", seed=1234), strict=True)
    opt = torch.optim.SGD(m.parameters(), lr=0.001, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m.cuda(), opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
    stats = tr.run_epoch("train", 1, TrainLoader(ds, cfg, seed=1))
    for k in ("loss", "class_loss", "score_loss", "bbox_loss"):
        assert np.isfinite(stats[k]), (k, stats)
    assert stats["loss"] > 0


def test_mosaic_off_is_todays_path_bit_for_bit():
    """``mosaic_prob`` 0 on a loader built with mosaic on: the images of the plain letterbox loader, and no mosaic keys."""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MixedDataset(8)
    on = TrainLoader(ds, _loader_cfg("dense", mosaic_prob=1.0, zoom_out=0.5), seed=5)
    on.mosaic_prob = 0.0
    off = TrainLoader(ds, _loader_cfg("dense", zoom_out=0.5), seed=5)
    for a, b in zip(on, off):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["gt"], b["gt"])
        assert sorted(a["image_meta"]) == sorted(b["image_meta"]) and "mosaic" not in a["image_meta"]


def test_captured_step_equals_the_eager_loop_on_mosaic_batches():
    """Three sparse mosaic batches (their positive counts differ: the sparse capacity follows its own rule) through GraphedStep and through
    the eager sequence, by the method of tests/test_graph_step_gpu.py: bit for bit after every step."""
    import test_graph_step_gpu as G
    from squeezedet_pytorch_amd.train_data import TrainLoader
    cfg = _loader_cfg("sparse", mosaic_prob=1.0, graph_step=True, lr=G.LR)
    batches = list(TrainLoader(_MixedDataset(12), cfg, seed=3))
    assert len(batches) == 3 and all(any(augment.tile_count(t) == 4 for t in b["image_meta"]["mosaic"]) for b in batches)
    torch.manual_seed(11)
    g = G.Graphed(cfg)
    torch.manual_seed(11)
    e = G.Eager(cfg)
    for i, batch in enumerate(batches + batches[:1]):
        out_g, out_e = g.step(batch), e.step(batch)
        G.assert_same_state(g, e, f"mosaic step {i}", out_g, out_e)
    assert g.gs.replays >= 1
