"""Colour jitter on the MI355X ("Colour jitter"): the colour entry points (sqd_preprocess_u8_aug_color_fwd /
sqd_preprocess_u8_padcrop_aug_color_fwd) against the float64 restatement of the rule (tests/color_jitter_ref.py) composed with the
test-local numpy composition of tests/test_augment_gpu.py (drift and flip by slicing with a zero fill after whitening, then
oracle.resize_linear_f32 / crop_or_pad); bitwise identity with the ``_aug_`` entry points at (1, 1, 1); the fill; the pivot sums; and
the TrainLoader with jitter on against jitter off.

Bound of the rule tests: atol 2e-5, the suite's own bound for this kernel.  The colour chain adds at most about ten float32
operations on values up to 255 (2^-17 each), amplified by at most fc * fs <= 4 and divided by std ~ 80: under 5e-6."""
import numpy as np
import pytest
import torch

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment, dataset_stats, synthetic

import color_jitter_ref as cref

pytestmark = pytest.mark.gpu

MEAN = oracle.KITTI_RGB_MEAN.reshape(1, 1, 3).astype(np.float32)
STD = oracle.KITTI_RGB_STD.reshape(1, 1, 3).astype(np.float32)

FACTORS = [(1.8, 1., 1.),        # the upper clamp reached, table-only branch (fs == 1)
           (0.3, 1.9, 1.),       # table-only, both clamps of the contrast step
           (1., 0., 1.),         # a flat image
           (1., 1., 0.),         # grey: the per-tap branch
           (1.4, 0.6, 1.7),      # per-tap, all three active
           (1., 1., 1.)]         # the identity


def _colors_for(n, start):
    return np.float32([FACTORS[(start + k) % len(FACTORS)] for k in range(n)])


def _launch(images, augs, target, forbid, color=None, sums=None):
    """The kernels through augment's packing: (out [B,3,H,W] numpy, scales fp32 [B,2] or padcrop int32 [B,8] numpy).
    ``color``: float32 [B, 3] -> the colour header and the colour entry points."""
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes, color is not None)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    pk = buf.numpy()
    augment.write_header(pk, offsets, sizes, np.asarray(augs, np.int32), color)
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    dev = buf.cuda()
    out = torch.full((len(images), 3, target[0], target[1]), float("nan"), device="cuda")
    side = augment.launch(dev, len(images), hdr, target, out, forbid, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD,
                          color=color is not None, sums=sums)
    torch.cuda.synchronize()
    return out.cpu().numpy(), side.cpu().numpy()


def _crop_or_pad(x, target):
    H, W = target
    h, w = x.shape[:2]
    out = np.zeros((H, W, 3), np.float32)
    pt, ct = max((H - h) // 2, 0), max((h - H) // 2, 0)
    pl, cl = max((W - w) // 2, 0), max((w - W) // 2, 0)
    nh, nw = min(h, H), min(w, W)
    out[pt:pt + nh, pl:pl + nw] = x[ct:ct + nh, cl:cl + nw]
    return out


def _compose(x, aug, target, forbid):
    """A whitened float32 [H0, W0, 3] image -> drift with a zero fill, flip, then resize or crop_or_pad; CHW."""
    dy, dx, fl = (int(v) for v in aug)
    h0, w0 = x.shape[:2]
    v = np.zeros((h0 - dy, w0 - dx, 3), np.float32)
    v[max(-dy, 0):, max(-dx, 0):] = x[max(dy, 0):, max(dx, 0):]
    if fl:
        v = v[:, ::-1]
    y = _crop_or_pad(v, target) if forbid else oracle.resize_linear_f32(np.ascontiguousarray(v), target)
    return np.ascontiguousarray(y.transpose(2, 0, 1)), v.shape[:2]


def _reference(im, aug, target, forbid, color):
    """The float64 rule on the source pixels, whitened in float64, rounded to float32 once, then the plain composition."""
    x = cref.whiten(cref.jitter(im, color), MEAN, STD).astype(np.float32)
    return _compose(x, aug, target, forbid)


def _source_mask(im, aug, target, forbid):
    """True where an output pixel takes anything from the source image (False: pure drift fill or padding)."""
    y, _ = _compose(np.ones(im.shape, np.float32), aug, target, forbid)
    return y != 0


def _augs_for(sizes, variant):
    out = []
    for h, w in sizes:
        if variant == 0:
            out.append((min(h // 5, h - 1), min(w // 9, w - 1), 1))
        elif variant == 1:
            out.append((-(h // 4) - 1, -(w // 8) - 1, 0))
        else:
            out.append((-(h // 4) - 1, min(w // 9, w - 1), 1))
    return out


def _report(tag, out, ref):
    err = float(np.abs(out.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{tag}: max abs err {err:.3e}")
    return err


RESIZE_CASES = [
    ([(33, 3001), (1, 1), (7, 1), (1, 9)], (64, 96)),           # odd byte offsets, one-pixel sources, the buffer ends inside a dword
    ([(40, 3000), (3, 2731)], (64, 96)),                          # segment larger than the LDS staging buffer: direct path
    ([(97, 300), (13, 1023)], (61, 517)),                         # target not a multiple of the workgroup tile
]


@pytest.mark.parametrize("sizes,target", RESIZE_CASES)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_resize_color_vs_float64_rule(sizes, target, variant):
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    augs = _augs_for(sizes, variant)
    colors = _colors_for(len(sizes), 2 * variant)                 # the three variants together use every factor triple
    out, scales = _launch(images, augs, target, False, colors)
    for b, (im, a) in enumerate(zip(images, augs)):
        ref, (hd, wd) = _reference(im, a, target, False, colors[b])
        _report(f"resize {sizes[b]} -> {target} aug {a} color {tuple(colors[b])}", out[b], ref)
        np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0, err_msg=f"image {b} aug {a} color {colors[b]}")
        assert np.array_equal(scales[b], np.array([target[0] / hd, target[1] / wd], np.float32))


def test_every_factor_triple_is_used_by_the_resize_cases():
    for sizes, _t in RESIZE_CASES:
        used = {tuple(c) for v in range(3) for c in _colors_for(len(sizes), 2 * v)}
        assert used == {tuple(np.float32(f)) for f in FACTORS}
    assert any(len({c[2] == 1 for c in _colors_for(len(s), 2 * v)}) == 2 for s, _t in RESIZE_CASES for v in range(3))   # both branches in one launch


PADCROP_SIZES, PADCROP_TARGET = [(1, 1), (400, 1300), (383, 1249), (5, 2000), (390, 7)], (384, 1248)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_padcrop_color_vs_float64_rule(variant):
    rs = np.random.RandomState(6)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in PADCROP_SIZES]
    augs = _augs_for(PADCROP_SIZES, variant)
    colors = _colors_for(len(images), 2 * variant)
    out, pc = _launch(images, augs, PADCROP_TARGET, True, colors)
    plain, pc_plain = _launch(images, augs, PADCROP_TARGET, True)
    assert np.array_equal(pc, pc_plain)                           # padding / crops: exactly as without colour
    for b, (im, a) in enumerate(zip(images, augs)):
        ref, _ = _reference(im, a, PADCROP_TARGET, True, colors[b])
        _report(f"padcrop {PADCROP_SIZES[b]} aug {a} color {tuple(colors[b])}", out[b], ref)
        np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0, err_msg=f"image {b} aug {a} color {colors[b]}")
        inside = _source_mask(im, a, PADCROP_TARGET, True)
        assert np.all(out[b][~inside] == 0.0) and np.all(plain[b][~inside] == 0.0)     # padding and fill: exactly 0.0
        _tb, meta = augment.transform_boxes(np.zeros((0, 4), np.float32), im.shape[:2], a, PADCROP_TARGET, True)
        assert pc[b].tolist() == meta["padding"].tolist() + meta["crops"].tolist()


@pytest.mark.parametrize("forbid", [False, True])
def test_identity_factors_are_bitwise_the_aug_kernel(forbid):
    rs = np.random.RandomState(2)
    sizes = [(375, 1242), (370, 1224), (33, 3001), (1, 1), (400, 1300), (97, 300)]
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    ones = np.ones((len(images), 3), np.float32)
    for target in ((384, 1248), (61, 517)):
        for augs in (np.zeros((len(images), 3), np.int32), _augs_for(sizes, 0), _augs_for(sizes, 2)):
            ref, side_ref = _launch(images, augs, target, forbid)
            out, side = _launch(images, augs, target, forbid, ones)
            assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
            assert np.array_equal(side, side_ref)                 # scales, or padding / crops


@pytest.mark.parametrize("aug", [(-100, -400, 0), (-100, -400, 1)])      # the fill covers whole workgroup segments (rows and columns)
def test_fill_stays_exactly_zero(aug):
    target, size, color = (384, 1248), (375, 1242), np.float32([[0.3, 1.9, 0.5]])
    im = np.random.RandomState(9).randint(0, 256, size + (3,), dtype=np.uint8)
    out, _ = _launch([im], [aug], target, False, color)
    ref, _ = _reference(im, aug, target, False, color[0])
    _report(f"fill aug {aug}", out[0], ref)
    np.testing.assert_allclose(out[0], ref, atol=2e-5, rtol=0)
    fill = ~_source_mask(im, aug, target, False)
    assert np.count_nonzero(fill) > 3 * 90 * 390                  # 100 of 475 rows and 400 of 1642 columns, scaled to the target
    assert np.all(out[0][fill] == 0.0)
    assert np.count_nonzero(out[0][~fill] == 0.0) < 100           # ... and the rest is not zero by construction


def test_pivot_sums_are_the_exact_host_sums():
    sizes, target = RESIZE_CASES[0]
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    sums = torch.full((len(images), 3, 2), -1, device="cuda", dtype=torch.int64)
    _launch(images, _augs_for(sizes, 0), target, False, _colors_for(len(images), 0), sums=sums)
    got = sums.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np.stack([dataset_stats.host_sums(im) for im in images]))


class _MemDataset:
    def __init__(self, n, seed=0, sizes=((120, 250), (131, 262), (117, 241))):
        rs = np.random.RandomState(seed)
        self.images, self.ann = [], []
        for i in range(n):
            h, w = sizes[i % len(sizes)]
            self.images.append(rs.randint(0, 256, (h, w, 3)).astype(np.float32))
            m = int(rs.randint(1, 4))
            x1 = rs.uniform(0, w * 0.6, m); y1 = rs.uniform(0, h * 0.6, m)
            b = np.stack([x1, y1, x1 + rs.uniform(8, w * 0.4, m), y1 + rs.uniform(8, h * 0.4, m)], 1).astype(np.float32)
            self.ann.append((rs.randint(0, 3, m).astype(np.int16), b))
        self.rgb_mean, self.rgb_std = MEAN, STD

    def __len__(self):
        return len(self.images)

    def load_image(self, i):
        return self.images[i], f"{i:06d}"

    def load_annotations(self, i):
        return self.ann[i][0].copy(), self.ann[i][1].copy()


JIT = dict(brightness_jitter=0.4, contrast_jitter=0.3, saturation_jitter=0.5)


def _cfg(**kw):
    return sqd.make_cfg(input_size=(128, 256), device="cuda", batch_size=4, **kw)


def _batches(loader):
    return [{"image": b["image"].cpu(), "gt": b["gt"].cpu(), "meta": b["image_meta"]} for b in loader]


@pytest.fixture(scope="module")
def loader_runs():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(8)
    return {"ds": ds,
            "on0": _batches(TrainLoader(ds, _cfg(num_workers=0, **JIT), seed=7)),
            "on3": _batches(TrainLoader(ds, _cfg(num_workers=3, **JIT), seed=7)),
            "off": _batches(TrainLoader(ds, _cfg(num_workers=3), seed=7)),
            "plan": list(TrainLoader(ds, _cfg(**JIT), seed=7).plan())}


def test_loader_with_jitter_is_identical_for_any_worker_count(loader_runs):
    a, b = loader_runs["on0"], loader_runs["on3"]
    assert len(a) == len(b) == 2
    for x, y in zip(a, b):
        assert torch.equal(x["image"], y["image"]) and torch.equal(x["gt"], y["gt"])
        assert np.array_equal(x["meta"]["color"], y["meta"]["color"]) and np.array_equal(x["meta"]["index"], y["meta"]["index"])


def test_loader_jitter_changes_the_pixels_and_nothing_else(loader_runs):
    on, off, plan = loader_runs["on3"], loader_runs["off"], loader_runs["plan"]
    for x, y, p in zip(on, off, plan):
        assert torch.equal(x["gt"], y["gt"]) and not torch.equal(x["image"], y["image"])
        assert "color" not in y["meta"]
        for k in ("index", "drifts", "scales", "drifted_size"):
            assert np.array_equal(x["meta"][k], y["meta"][k]), k
        assert x["meta"]["flipped"] == y["meta"]["flipped"]
        c = x["meta"]["color"]
        assert c.dtype == np.float32 and c.shape == (4, 3) and np.array_equal(c, p["color"])
        assert np.array_equal(x["meta"]["index"], p["index"])
    # a batch is preprocess_train_batch on the same images with the loader's geometric and colour draws
    ds, b0 = loader_runs["ds"], on[0]
    idx = b0["meta"]["index"]
    aug = np.stack([b0["meta"]["drifts"][:, 0], b0["meta"]["drifts"][:, 1], np.array(b0["meta"]["flipped"], np.int32)], 1)
    x, m, gt = augment.preprocess_train_batch([ds.images[i] for i in idx], [ds.ann[i][0] for i in idx], [ds.ann[i][1] for i in idx],
                                              (128, 256), None, device="cuda", anchors=_cfg().anchors, aug=aug, rgb_mean=MEAN,
                                              rgb_std=STD, color=b0["meta"]["color"])
    assert torch.equal(x.cpu(), b0["image"]) and torch.equal(gt.cpu(), b0["gt"]) and np.array_equal(m["color"], b0["meta"]["color"])


def test_loader_zero_jitter_is_bitwise_a_cfg_without_the_fields(loader_runs):
    from squeezedet_pytorch_amd.train_data import TrainLoader
    zero = _batches(TrainLoader(loader_runs["ds"], _cfg(num_workers=3, brightness_jitter=0., contrast_jitter=0., saturation_jitter=0.), seed=7))
    bare = _cfg(num_workers=3)
    for k in JIT:
        delattr(bare, k)
    none = _batches(TrainLoader(loader_runs["ds"], bare, seed=7))
    for x, y, z in zip(zero, none, loader_runs["off"]):
        assert torch.equal(x["image"], y["image"]) and torch.equal(x["gt"], y["gt"]) and "color" not in x["meta"] and "color" not in y["meta"]
        assert torch.equal(x["image"], z["image"])


def test_jittering_loader_feeds_trainer_run_epoch():
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import Trainer
    cfg = _cfg(num_workers=2, dropout_prob=0.0, **JIT)
    cfg.num_iters, cfg.print_interval = 2, 1000
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict("squeezedet", seed=1234), strict=True)
    opt = torch.optim.SGD(m.parameters(), lr=0.001, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m.cuda(), opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
    stats = tr.run_epoch("train", 1, TrainLoader(_MemDataset(8), cfg, seed=1))
    for k in ("loss", "class_loss", "score_loss", "bbox_loss"):
        assert np.isfinite(stats[k]), (k, stats)
    assert stats["loss"] > 0
