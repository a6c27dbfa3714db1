"""Training augmentation on the MI355X: the augmented preprocessing kernels (sqd_preprocess_u8_aug_fwd /
sqd_preprocess_u8_padcrop_aug_fwd) against the reference's train-phase preprocess (tests/golden/augment.npz) and against a
test-local numpy composition (oracle whiten, drift and flip by slicing, then oracle.resize_linear_f32 / crop_or_pad), identity
with the eval kernels at zero augmentation, the dense targets, and the TrainLoader feeding Trainer.run_epoch."""
import os

import numpy as np
import pytest
import torch

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment, synthetic

pytestmark = pytest.mark.gpu

MEAN = oracle.KITTI_RGB_MEAN.reshape(1, 1, 3).astype(np.float32)
STD = oracle.KITTI_RGB_STD.reshape(1, 1, 3).astype(np.float32)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def _image_of(seed, h, w):                    # as tests/golden/make_golden_augment.py
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _launch(images, augs, target, forbid):
    """The kernels through augment's packing: (out [B,3,H,W] numpy, scales fp32 [B,2] or padcrop int32 [B,8] numpy)."""
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    pk = buf.numpy()
    augment.write_header(pk, offsets, sizes, np.asarray(augs, np.int32))
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = im.reshape(-1)
    dev = buf.cuda()
    out = torch.full((len(images), 3, target[0], target[1]), float("nan"), device="cuda")
    side = augment.launch(dev, len(images), hdr, target, out, forbid, oracle.KITTI_RGB_MEAN, oracle.KITTI_RGB_STD)
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


def _reference(im, aug, target, forbid):
    """whiten (oracle arithmetic), drift with a zero fill AFTER whitening, flip, then resize or crop_or_pad; CHW."""
    x = (im.astype(np.float32) - MEAN) / STD
    dy, dx, fl = (int(v) for v in aug)
    h0, w0 = x.shape[:2]
    v = np.zeros((h0 - dy, w0 - dx, 3), np.float32)
    v[max(-dy, 0):, max(-dx, 0):] = x[max(dy, 0):, max(dx, 0):]
    if fl:
        v = v[:, ::-1]
    y = _crop_or_pad(v, target) if forbid else oracle.resize_linear_f32(np.ascontiguousarray(v), target)
    return np.ascontiguousarray(y.transpose(2, 0, 1)), v.shape[:2]


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


RESIZE_CASES = [
    ([(33, 3001), (1, 1), (7, 1), (1, 9)], (384, 1248)),        # odd byte offsets, one-pixel sources, the buffer ends inside a dword
    ([(40, 3000), (3, 2731)], (64, 96)),                          # segment larger than the LDS staging buffer: direct path
    ([(40, 2728), (41, 2729)], (64, 96)),                         # ... and just inside it
    ([(375, 1242)] * 3, (384, 1248)),
    ([(97, 300), (13, 1023)], (61, 517)),                         # target not a multiple of the workgroup tile
]


@pytest.mark.parametrize("sizes,target", RESIZE_CASES)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_resize_aug_vs_numpy_composition(sizes, target, variant):
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    augs = _augs_for(sizes, variant)
    out, scales = _launch(images, augs, target, False)
    for b, (im, a) in enumerate(zip(images, augs)):
        ref, (hd, wd) = _reference(im, a, target, False)
        np.testing.assert_allclose(out[b], ref, atol=2e-5, rtol=0, err_msg=f"image {b} aug {a}")
        assert np.array_equal(scales[b], np.array([target[0] / hd, target[1] / wd], np.float32))


PADCROP_CASES = [
    ([(1, 1), (400, 1300), (383, 1249), (5, 2000), (390, 7)], (384, 1248)),
    ([(61, 517), (60, 516), (62, 519), (3, 3)], (61, 517)),
]


@pytest.mark.parametrize("sizes,target", PADCROP_CASES)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_padcrop_aug_bit_exact_vs_numpy_composition(sizes, target, variant):
    rs = np.random.RandomState(6)
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    augs = _augs_for(sizes, variant)
    out, pc = _launch(images, augs, target, True)
    for b, (im, a) in enumerate(zip(images, augs)):
        ref, (hd, wd) = _reference(im, a, target, True)
        assert np.array_equal(out[b], ref), f"image {b} aug {a}"
        _tb, meta = augment.transform_boxes(np.zeros((0, 4), np.float32), im.shape[:2], a, target, True)
        assert pc[b].tolist() == meta["padding"].tolist() + meta["crops"].tolist()


@pytest.mark.parametrize("forbid,target,size,aug", [
    (False, (384, 1248), (375, 1242), (-100, -400, 0)),          # the fill covers whole workgroup segments (rows and columns)
    (False, (384, 1248), (375, 1242), (-100, -400, 1)),          # ... on the right under a flip
    (True, (64, 1248), (60, 700), (-30, -600, 0)),
    (True, (64, 1248), (60, 700), (-30, -600, 1)),
    (False, (64, 96), (1, 1), (-5, -7, 1)),                      # a 1x1 image, drifted and flipped
    (True, (64, 96), (1, 1), (-5, -7, 1)),
])
def test_aug_fill_covers_whole_segments(forbid, target, size, aug):
    im = np.random.RandomState(9).randint(0, 256, size + (3,), dtype=np.uint8)
    out, _ = _launch([im], [aug], target, forbid)
    ref, _ = _reference(im, aug, target, forbid)
    if forbid:
        assert np.array_equal(out[0], ref)
    else:
        np.testing.assert_allclose(out[0], ref, atol=2e-5, rtol=0)
    assert np.count_nonzero(out[0] == 0) > 0


@pytest.mark.parametrize("forbid", [False, True])
def test_zero_aug_is_bitwise_the_eval_kernel(forbid):
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    rs = np.random.RandomState(2)
    sizes = [(375, 1242), (370, 1224), (33, 3001), (1, 1), (400, 1300), (97, 300)]
    images = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    for target in ((384, 1248), (61, 517)):
        ref, side_ref, meta = preprocess_batch(images, target, forbid_resize=forbid)
        out, side = _launch(images, np.zeros((len(images), 3), np.int32), target, forbid)
        assert np.array_equal(out.view(np.uint32), ref.cpu().numpy().view(np.uint32))
        if forbid:
            assert np.array_equal(side[:, :4], meta["padding"]) and np.array_equal(side[:, 4:], meta["crops"])
        else:
            assert np.array_equal(side, side_ref.cpu().numpy())


def _gold_case(gold, c):
    seed, h, w, forbid = (int(v) for v in gold[f"c{c}_cfg"])
    imgs = gold[f"c{c}_images"]
    images = [_image_of(int(s), int(ih), int(iw)) for ih, iw, s in imgs]
    cls = [gold[f"c{c}_i{k}_cls"] for k in range(len(imgs))]
    boxes = [gold[f"c{c}_i{k}_boxes_in"] for k in range(len(imgs))]
    return seed, (h, w), bool(forbid), images, cls, boxes


def _ulps(a, b):
    return np.abs(a.astype(np.float32).view(np.int32).astype(np.int64) - b.astype(np.float32).view(np.int32).astype(np.int64))


def test_train_batch_vs_reference_fixture(gold):
    """preprocess_train_batch drawing from RandomState(seed) == the reference's preprocess + prepare_annotations under
    np.random.seed(seed): images (crop_or_pad bit-exact, resize within 2e-5), scales / padding / crops exact, dense gt equal where the
    reference's anchor picks are uniquely determined (regression targets within 1 ulp), the same boxes and classes everywhere."""
    for c in range(int(gold["n"])):
        seed, size, forbid, images, cls, boxes = _gold_case(gold, c)
        probs = gold[f"c{c}_probs"]
        cfg = sqd.make_cfg(input_size=size, device="cuda")
        rng = np.random.RandomState(seed)
        x, meta, gt = augment.preprocess_train_batch([im.astype(np.float32) for im in images], cls, boxes, size, rng, float(probs[0]),
                                                     float(probs[1]), forbid_resize=forbid, device="cuda", anchors=cfg.anchors)
        torch.cuda.synchronize()
        assert np.array_equal(np.stack([meta["drifts"][:, 0], meta["drifts"][:, 1], np.array(meta["flipped"], np.int32)], 1), gold[f"c{c}_aug"])
        x, gt = x.cpu().numpy(), gt.cpu().numpy()
        for k in range(len(images)):
            if size == (384, 1248):
                rows, cols = gold["sample_rows"], gold["sample_cols"]
                samp = x[k][:, rows][:, :, cols]
                sums = x[k].astype(np.float64).sum(axis=(1, 2))
                if forbid:
                    assert np.array_equal(samp, gold[f"c{c}_i{k}_sample"]) and np.array_equal(sums, gold[f"c{c}_i{k}_sums"]), (c, k)
                else:
                    np.testing.assert_allclose(samp, gold[f"c{c}_i{k}_sample"], atol=2e-5, rtol=0)
                    np.testing.assert_allclose(sums, gold[f"c{c}_i{k}_sums"], atol=2e-5 * x[k][0].size, rtol=0)
            elif forbid:
                assert np.array_equal(x[k], gold[f"c{c}_i{k}_image"]), (c, k)
            else:
                np.testing.assert_allclose(x[k], gold[f"c{c}_i{k}_image"], atol=2e-5, rtol=0)
            if forbid:
                assert np.array_equal(meta["padding"][k], gold[f"c{c}_i{k}_padding"]) and np.array_equal(meta["crops"][k], gold[f"c{c}_i{k}_crops"])
            else:
                assert np.array_equal(meta["scales"][k], gold[f"c{c}_i{k}_scales"])
            idx, ref_rows = gold[f"c{c}_i{k}_gt_idx"], gold[f"c{c}_i{k}_gt_rows"]
            mine = np.nonzero(gt[k][:, 0])[0]
            assert len(mine) == len(idx)
            key = lambda r: np.lexsort(r[:, ::-1].T)            # noqa: E731
            ra, rb = gt[k][mine][:, list(range(1, 5)) + list(range(9, 12))], ref_rows[:, list(range(1, 5)) + list(range(9, 12))]
            assert np.array_equal(ra[key(ra)], rb[key(rb)]), (c, k)
            if bool(gold[f"c{c}_i{k}_unique"]):
                assert np.array_equal(mine, idx), (c, k)
                assert np.array_equal(gt[k][idx][:, :5], ref_rows[:, :5]) and np.array_equal(gt[k][idx][:, 9:], ref_rows[:, 9:])
                assert _ulps(gt[k][idx][:, 5:9], ref_rows[:, 5:9]).max() <= 1, (c, k)


def test_loss_on_forced_draws_equals_loss_on_reference_batch(gold):
    """The model's per-image loss on a preprocess_train_batch batch whose draws are the fixture's == its loss on the
    reference-preprocessed batch (fixture images and targets), within 1e-4, where the reference's targets are fully determined."""
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    cases = [c for c in range(int(gold["n"])) if tuple(int(v) for v in gold[f"c{c}_cfg"][1:3]) == (64, 96)]
    checked = 0
    for c in cases:
        _seed, size, forbid, images, cls, boxes = _gold_case(gold, c)
        cfg = sqd.make_cfg(input_size=size, dropout_prob=0.0, device="cuda")
        m = SqueezeDetWithLoss(cfg)
        m.load_state_dict(synthetic.make_state_dict("squeezedet", seed=1234), strict=True)
        m = m.cuda().eval()
        x, _meta, gt = augment.preprocess_train_batch(images, cls, boxes, size, None, forbid_resize=forbid, device="cuda",
                                                      anchors=cfg.anchors, aug=gold[f"c{c}_aug"])
        n = len(images)
        xr = torch.from_numpy(np.stack([gold[f"c{c}_i{k}_image"] for k in range(n)])).cuda()
        gr = np.zeros((n, cfg.num_anchors, 12), np.float32)
        for k in range(n):
            gr[k][gold[f"c{c}_i{k}_gt_idx"]] = gold[f"c{c}_i{k}_gt_rows"]
        with torch.no_grad():
            loss, _ = m({"image": x, "gt": gt})
            loss_ref, _ = m({"image": xr, "gt": torch.from_numpy(gr).cuda()})
        loss, loss_ref = loss.cpu().numpy(), loss_ref.cpu().numpy()
        assert np.all(np.isfinite(loss))
        for k in range(n):
            if bool(gold[f"c{c}_i{k}_unique"]):
                assert abs(loss[k] - loss_ref[k]) <= 1e-4 * max(1.0, abs(loss_ref[k])), (c, k, loss[k], loss_ref[k])
                checked += 1
    assert checked >= 4


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


def _batches(loader):
    return [{"image": b["image"].cpu(), "gt": b["gt"].cpu(), "meta": b["image_meta"]} for b in loader]


@pytest.mark.parametrize("forbid", [False, True])
def test_loader_identical_for_any_worker_count(forbid):
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(11)
    runs = []
    for w in (0, 1, 4):
        cfg = sqd.make_cfg(input_size=(128, 256), device="cuda", batch_size=4, num_workers=w, forbid_resize=forbid)
        runs.append(_batches(TrainLoader(ds, cfg, seed=7)))
    assert len(runs[0]) == 2                                         # drop_last: 11 // 4
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a["image"], b["image"]) and torch.equal(a["gt"], b["gt"])
            assert np.array_equal(a["meta"]["index"], b["meta"]["index"]) and np.array_equal(a["meta"]["drifts"], b["meta"]["drifts"])
    cfg = sqd.make_cfg(input_size=(128, 256), device="cuda", batch_size=4, forbid_resize=forbid)
    last = _batches(TrainLoader(ds, cfg, seed=7, drop_last=False))
    assert len(last) == 3 and last[2]["image"].shape[0] == 3
    # a batch equals preprocess_train_batch on the same images with the loader's draws
    b0 = runs[0][0]
    idx = b0["meta"]["index"]
    aug = np.stack([b0["meta"]["drifts"][:, 0], b0["meta"]["drifts"][:, 1], np.array(b0["meta"]["flipped"], np.int32)], 1)
    x, _m, gt = augment.preprocess_train_batch([ds.images[i] for i in idx], [ds.ann[i][0] for i in idx], [ds.ann[i][1] for i in idx],
                                               (128, 256), None, forbid_resize=forbid, device="cuda", anchors=cfg.anchors, aug=aug,
                                               rgb_mean=MEAN, rgb_std=STD)
    assert torch.equal(x.cpu(), b0["image"]) and torch.equal(gt.cpu(), b0["gt"])


def test_loader_rejects_non_uint8_pixels():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(4)
    ds.images[2] = ds.images[2] + 0.5
    cfg = sqd.make_cfg(input_size=(128, 256), device="cuda", batch_size=4, num_workers=2)
    with pytest.raises(ValueError, match="image 2"):
        list(TrainLoader(ds, cfg, shuffle=False))


def test_loader_feeds_trainer_run_epoch():
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import Trainer
    cfg = sqd.make_cfg(input_size=(128, 256), device="cuda", batch_size=4, num_workers=2, dropout_prob=0.0)
    cfg.num_iters, cfg.print_interval = 2, 1000
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict("squeezedet", seed=1234), strict=True)
    opt = torch.optim.SGD(m.parameters(), lr=0.001, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m.cuda(), opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
    stats = tr.train_epoch(1, TrainLoader(_MemDataset(12), cfg, seed=1))
    for k in ("loss", "class_loss", "score_loss", "bbox_loss"):
        assert np.isfinite(stats[k]), (k, stats)
    assert stats["loss"] > 0


def test_train_batch_fills_out_in_place(gold):
    seed, size, forbid, images, cls, boxes = _gold_case(gold, 2)
    out = torch.empty(len(images), 3, size[0], size[1], device="cuda")
    x, _meta, _gt = augment.preprocess_train_batch(images, cls, boxes, size, np.random.RandomState(seed), forbid_resize=forbid,
                                                   device="cuda", out=out, anchors=sqd.make_cfg(input_size=size).anchors)
    assert x is out
    with pytest.raises(ValueError):
        augment.preprocess_train_batch(images, cls, boxes, size, np.random.RandomState(seed), device="cuda", out=out[:1])
