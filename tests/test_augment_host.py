"""Training augmentation, host side (CPU tier): the parameter draws, the box transform and the targets against the reference's own
train-phase ``preprocess`` / ``prepare_annotations`` (tests/golden/augment.npz, tests/golden/make_golden_augment.py), the two
documented departures, and the loader's epoch plan (rank shards, independence of ``num_workers``)."""
import os

import numpy as np
import pytest

import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment
from squeezedet_pytorch_amd import boxes as host_boxes


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def _cases(gold):
    for c in range(int(gold["n"])):
        seed, h, w, forbid = (int(v) for v in gold[f"c{c}_cfg"])
        drift_prob, flip_prob = (float(v) for v in gold[f"c{c}_probs"])
        imgs = gold[f"c{c}_images"]
        yield c, seed, (h, w), bool(forbid), drift_prob, flip_prob, imgs


def test_draws_and_rng_state_match_reference(gold):
    for c, seed, _size, _forbid, drift_prob, flip_prob, imgs in _cases(gold):
        rng = np.random.RandomState(seed)
        boxes = [gold[f"c{c}_i{k}_boxes_in"] for k in range(len(imgs))]
        aug = augment.draw_augmentation(rng, [tuple(im[:2]) for im in imgs], boxes, drift_prob, flip_prob)
        assert aug.dtype == np.int32 and np.array_equal(aug, gold[f"c{c}_aug"]), c
        st = rng.get_state()
        assert np.array_equal(st[1], gold[f"c{c}_state_key"]) and st[2] == int(gold[f"c{c}_state_pos"]), c


def test_global_numpy_state_gives_the_same_draws(gold):
    """Under ``np.random.seed(s)`` (the reference's single-process setting) the module-level RandomState draws the same."""
    c, seed, _size, _forbid, drift_prob, flip_prob, imgs = next(_cases(gold))
    np.random.seed(seed)
    aug = augment.draw_augmentation(np.random.mtrand._rand, [tuple(im[:2]) for im in imgs],
                                    [gold[f"c{c}_i{k}_boxes_in"] for k in range(len(imgs))], drift_prob, flip_prob)
    assert np.array_equal(aug, gold[f"c{c}_aug"])


def test_boxes_and_targets_bit_exact(gold):
    for c, _seed, size, forbid, _dp, _fp, imgs in _cases(gold):
        anchors = host_boxes.generate_anchors(tuple(x // 16 for x in size), size, host_boxes.KITTI_ANCHORS_SEED)
        for k, (h, w, _s) in enumerate(imgs):
            tb, meta = augment.transform_boxes(gold[f"c{c}_i{k}_boxes_in"], (h, w), gold[f"c{c}_aug"][k], size, forbid)
            ref = gold[f"c{c}_i{k}_boxes_out"]
            assert tb.dtype == np.float32 and np.array_equal(tb, ref), (c, k, tb, ref)
            if forbid:
                assert np.array_equal(meta["padding"], gold[f"c{c}_i{k}_padding"]) and np.array_equal(meta["crops"], gold[f"c{c}_i{k}_crops"])
                assert meta["padding"].dtype == np.int16
            else:
                assert meta["scales"].dtype == np.float32 and np.array_equal(meta["scales"], gold[f"c{c}_i{k}_scales"])
            assert np.array_equal(meta["drifted_size"], [h - meta["drifts"][0], w - meta["drifts"][1], 3])
            gt = host_boxes.prepare_annotations(gold[f"c{c}_i{k}_cls"], tb, anchors, 3)
            rows = np.nonzero(gt[:, 0])[0]
            assert np.array_equal(rows, gold[f"c{c}_i{k}_gt_idx"]) and np.array_equal(gt[rows], gold[f"c{c}_i{k}_gt_rows"]), (c, k)


def test_fixture_covers_both_branches_and_edge_bounds(gold):
    cases = list(_cases(gold))
    assert {f for _, _, _, f, _, _, _ in cases} == {True, False}
    assert {dp for _, _, _, _, dp, _, _ in cases} == {0.5, 1.0}
    flips = np.concatenate([gold[f"c{c}_aug"][:, 2] for c, *_ in cases])
    assert flips.min() == 0 and flips.max() == 1
    sizes = {tuple(im[:2]) for *_, imgs in cases for im in imgs}
    assert (375, 1242) in sizes and (370, 1224) in sizes


def test_empty_boxes_use_the_drift_bound():
    """Departure: the reference raises on an image without boxes (``min`` of an empty array); here it draws with its
    ``boxes is None`` bound, max_boxes = max_drift."""
    a = augment.draw_augmentation(np.random.RandomState(3), [(100, 200)], [np.zeros((0, 4), np.float32)], 1.0, 0.5)
    rs = np.random.RandomState(3)
    assert rs.uniform() < 1.0
    dy = rs.randint(-25, 25)
    dx = rs.randint(-25, 25)
    assert a.tolist() == [[dy, dx, int(rs.uniform() < 0.5)]]
    b = augment.draw_augmentation(np.random.RandomState(3), [(100, 200)], [None], 1.0, 0.5)
    assert np.array_equal(a, b)
    tb, meta = augment.transform_boxes(np.zeros((0, 4), np.float32), (100, 200), a[0], (48, 96))
    assert tb.shape == (0, 4) and meta["drifted_size"].tolist() == [100 - dy, 200 - dx, 3]


def test_empty_randint_range_gives_zero_drift_without_a_draw():
    """Departure: an image under 4 rows (or 8 columns) has an empty ``randint`` range on that axis (the reference raises): drift
    0 on that axis and no draw consumed for it."""
    boxes = [np.array([[1.0, 1.0, 5.0, 2.0]], np.float32)]
    rs = np.random.RandomState(5)
    a = augment.draw_augmentation(rs, [(3, 40)], boxes, 1.0, 0.5)
    ref = np.random.RandomState(5)
    ref.uniform()
    dx = ref.randint(-5, min(5, np.float32(1.0)))
    assert a.tolist() == [[0, dx, int(ref.uniform() < 0.5)]]
    assert np.array_equal(rs.get_state()[1], ref.get_state()[1]) and rs.get_state()[2] == ref.get_state()[2]
    a = augment.draw_augmentation(np.random.RandomState(5), [(1, 1)], [None], 1.0, 0.0)
    assert a.tolist() == [[0, 0, 0]]


def test_box_on_the_top_edge_keeps_drift_non_positive():
    """min(y1) = 0 -> ``randint(-H0 // 4, 0)``: the image never drifts up past a box that touches its top."""
    rng = np.random.RandomState(0)
    for _ in range(50):
        a = augment.draw_augmentation(rng, [(40, 80)], [np.array([[10., 0., 30., 20.]], np.float32)], 1.0, 0.5)
        assert -10 <= a[0, 0] < 0


def test_bad_image_raises():
    with pytest.raises(ValueError, match="image 3"):
        augment.as_u8_image(np.full((4, 4, 3), 0.5, np.float32), "image 3")
    with pytest.raises(ValueError, match="image 1"):
        augment.as_u8_image(np.zeros((4, 4), np.uint8), "image 1")
    assert augment.as_u8_image(np.full((2, 2, 3), 255.0, np.float32), "x").dtype == np.uint8


class _MemDataset:
    """The reference's dataset protocol over in-memory images (float32 as KITTI.load_image returns them)."""

    def __init__(self, n, seed=0, sizes=((40, 70), (37, 64), (45, 81))):
        rs = np.random.RandomState(seed)
        self.images, self.ann = [], []
        for i in range(n):
            h, w = sizes[i % len(sizes)]
            self.images.append(rs.randint(0, 256, (h, w, 3)).astype(np.float32))
            m = int(rs.randint(1, 4))
            x1 = rs.uniform(0, w * 0.6, m); y1 = rs.uniform(0, h * 0.6, m)
            b = np.stack([x1, y1, x1 + rs.uniform(4, w * 0.4, m), y1 + rs.uniform(4, h * 0.4, m)], 1).astype(np.float32)
            self.ann.append((rs.randint(0, 3, m).astype(np.int16), b))
        self.rgb_mean = augment.KITTI_RGB_MEAN.reshape(1, 1, 3)
        self.rgb_std = augment.KITTI_RGB_STD.reshape(1, 1, 3)

    def __len__(self):
        return len(self.images)

    def load_image(self, i):
        return self.images[i], f"{i:06d}"

    def load_annotations(self, i):
        return self.ann[i][0].copy(), self.ann[i][1].copy()


def _cfg(**kw):
    return sqd.make_cfg(input_size=(32, 64), device="cpu", batch_size=6, **kw)


def test_make_cfg_augmentation_defaults():
    cfg = sqd.make_cfg(device="cpu")
    assert (cfg.flip_prob, cfg.drift_prob, cfg.seed) == (0.5, 1.0, 42)


def test_rank_shards_concatenate_to_the_one_rank_batch():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(20)
    full = list(TrainLoader(ds, _cfg(), seed=3).plan())
    for world in (2, 3, 4):
        parts = [list(TrainLoader(ds, _cfg(), seed=3, rank=r, world=world).plan()) for r in range(world)]
        assert all(len(p) == len(full) for p in parts)
        for it, ref in enumerate(full):
            idx = np.concatenate([p[it]["index"] for p in parts])
            aug = np.concatenate([p[it]["aug"] for p in parts])
            assert np.array_equal(idx, ref["index"]) and np.array_equal(aug, ref["aug"]), (world, it)
            bx = [b for p in parts for b in p[it]["boxes"]]
            assert all(np.array_equal(x, y) for x, y in zip(bx, ref["boxes"]))


def test_plan_independent_of_workers_and_epochs_continue_the_stream():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(15)
    plans = [list(TrainLoader(ds, _cfg(num_workers=w), seed=11).plan()) for w in (0, 1, 4, 8)]
    for p in plans[1:]:
        assert all(np.array_equal(a["index"], b["index"]) and np.array_equal(a["aug"], b["aug"]) for a, b in zip(plans[0], p))
    ld = TrainLoader(ds, _cfg(), seed=11)
    e1, e2 = list(ld.plan()), list(ld.plan())
    assert len(ld) == 2 and len(e1) == 2                                  # drop_last: 15 // 6
    assert not all(np.array_equal(a["index"], b["index"]) for a, b in zip(e1, e2))
    assert len(TrainLoader(ds, _cfg(), seed=11, drop_last=False)) == 3


def test_unshuffled_plan_is_the_reference_draw_sequence():
    """shuffle=False: the draws are those of ``draw_augmentation`` over the dataset in order from a RandomState(seed)."""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(12)
    plan = list(TrainLoader(ds, _cfg(), seed=5, shuffle=False).plan())
    rng = np.random.RandomState(5)
    for it, p in enumerate(plan):
        idx = list(range(6 * it, 6 * it + 6))
        ref = augment.draw_augmentation(rng, [ds.images[i].shape[:2] for i in idx], [ds.ann[i][1] for i in idx], 1.0, 0.5)
        assert p["index"].tolist() == idx and np.array_equal(p["aug"], ref)
