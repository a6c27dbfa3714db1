"""Host half of the mosaic augmentation ("Mosaic"), on the CPU: the draws and their order, what mosaic leaves alone, rank
shards, the tile rule and the box rule against the plain loops of tests/mosaic_ref.py, the upload layout, the cfg checks and the two
entry points' argument checks.  Nothing here needs a device."""
import ctypes
import os

import numpy as np
import pytest

import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment

import mosaic_ref as mref
from test_letterbox_host import JIT, _MemDataset, _two_epochs

CANVAS = (32, 64)


def _cfg(**kw):
    return sqd.make_cfg(input_size=CANVAS, device="cpu", batch_size=6, **kw)


class _FlaggedDataset(_MemDataset):
    """_MemDataset whose every third image carries one more, flagged, box."""

    def load_annotations(self, i):
        c, b = super().load_annotations(i)
        f = np.zeros(len(b), np.uint8)
        if i % 3 == 0:
            h, w = self.images[i].shape[:2]
            c, b, f = np.append(c, 0), np.concatenate([b, np.float32([[1, 1, w - 2, h - 2]])]), np.append(f, 1)
        return c, b, f


# ---------------------------------------------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------------------------------------------
def test_draw_mosaic_consumes_exactly_the_stated_draws_in_order():
    H, W = 128, 256
    sizes = {j: (40 + 3 * j, 90 - 2 * j) for j in range(17)}
    boxes = {j: (None if j % 4 == 0 else np.float32([[5 + j, 6, 30 + j, 33]])) for j in range(17)}
    got = augment.draw_mosaic(np.random.RandomState(5), 9, 17, (H, W), 0.5, (0.5, 1.5), lambda j: (sizes[j], boxes[j]), 1.0, 0.5)
    rs = np.random.RandomState(5)
    mosaic, partners, centre, scale = [], [], [], []
    for _ in range(9):
        mosaic.append(rs.uniform() < 0.5)
        partners.append([rs.randint(0, 17), rs.randint(0, 17), rs.randint(0, 17)])
        centre.append((rs.randint(H // 4, H - H // 4 + 1), rs.randint(W // 4, W - W // 4 + 1)))
        scale.append([rs.uniform(0.5, 1.5) for _ in range(4)])
    aug = np.zeros((9, 3, 3), np.int32)
    for i in range(9):
        if mosaic[i]:
            for t, j in enumerate(partners[i]):                           # (image, tile) order, draw_augmentation's own draws per partner
                aug[i, t] = augment.draw_augmentation(rs, [sizes[j]], [boxes[j]], 1.0, 0.5)[0]
    assert 0 < sum(mosaic) < 9
    assert np.array_equal(got["mosaic"], mosaic) and np.array_equal(got["partners"], partners) and got["partners"].dtype == np.int64
    assert np.array_equal(got["centre"], centre) and np.array_equal(got["scale"], scale) and np.array_equal(got["aug"], aug)
    assert np.any(aug != 0)
    nxt = rs.uniform()
    probe = np.random.RandomState(5)
    augment.draw_mosaic(probe, 9, 17, (H, W), 0.5, (0.5, 1.5), lambda j: (sizes[j], boxes[j]), 1.0, 0.5)
    assert probe.uniform() == nxt                                         # not one draw more or fewer
    c = np.asarray(centre)
    assert c[:, 0].min() >= 32 and c[:, 0].max() <= 96 and c[:, 1].min() >= 64 and c[:, 1].max() <= 192


def test_mosaic_leaves_every_other_draw_alone_and_repeats_per_seed():
    from squeezedet_pytorch_amd.train_data import MOSAIC_STREAM, TrainLoader
    ds = _MemDataset(20)
    base = dict(letterbox=True, zoom_out=0.5, **JIT)
    off = _two_epochs(TrainLoader(ds, _cfg(**base), seed=3))
    on = _two_epochs(TrainLoader(ds, _cfg(mosaic_prob=0.5, **base), seed=3))
    again = _two_epochs(TrainLoader(ds, _cfg(mosaic_prob=0.5, **base), seed=3))
    other = _two_epochs(TrainLoader(ds, _cfg(mosaic_prob=0.5, **base), seed=4))
    assert len(on) == 6
    plain = mosaics = 0
    for a, b, b2 in zip(off, on, again):
        assert "mosaic" not in a and b["mosaic"].shape == (6, 4, 9) and b["mosaic"].dtype == np.int32
        assert b["mosaic_index"].shape == (6, 4) and b["mosaic_index"].dtype == np.int64
        for k in ("index", "aug", "color", "window"):
            assert np.array_equal(a[k], b[k]), k
        for k in ("mosaic", "mosaic_index", "source_aug"):
            assert np.array_equal(b[k], b2[k]), k
        assert all(np.array_equal(x, y) for x, y in zip(b["boxes"], b2["boxes"]))
        for j, t in enumerate(b["mosaic"]):
            if augment.tile_count(t) == 1:                                # a non-mosaic image: today's window, today's boxes, one tile
                plain += 1
                assert np.array_equal(t, augment.one_tile(a["window"][j], t[0, 0])) and np.array_equal(b["boxes"][j], a["boxes"][j])
                assert np.array_equal(b["mosaic_index"][j], [b["index"][j], -1, -1, -1])
            else:
                mosaics += 1
                assert augment.tile_count(t) == 4 and np.all(b["mosaic_index"][j] >= 0) and b["mosaic_index"][j, 0] == b["index"][j]
    assert plain > 5 and mosaics > 5
    assert any(not np.array_equal(x["mosaic"], y["mosaic"]) for x, y in zip(on, other))
    # the fourth stream's key, and its first draws
    rs = np.random.RandomState([3, MOSAIC_STREAM])
    p = next(iter(TrainLoader(ds, _cfg(mosaic_prob=0.5, letterbox=True), seed=3, shuffle=False).plan()))
    u, partners = rs.uniform(), [rs.randint(0, 20) for _ in range(3)]
    assert bool(p["mosaic_draw"]["mosaic"][0]) == (u < 0.5) and p["mosaic_draw"]["partners"][0].tolist() == partners
    assert p["mosaic_draw"]["centre"][0].tolist() == [rs.randint(8, 25), rs.randint(16, 49)]


def test_mosaic_prob_can_be_switched_off_between_epochs():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(12)
    on = TrainLoader(ds, _cfg(mosaic_prob=1.0, letterbox=True), seed=9)
    off = TrainLoader(ds, _cfg(letterbox=True), seed=9)
    e1, o1 = list(on.plan()), list(off.plan())
    assert all("mosaic" in p for p in e1)
    on.mosaic_prob = 0.0
    e2, o2 = list(on.plan()), list(off.plan())
    for a, b in zip(e2, o2):
        assert sorted(a) == sorted(b) and "mosaic" not in a
        assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["aug"], b["aug"]) and np.array_equal(a["window"], b["window"])
        assert all(np.array_equal(x, y) for x, y in zip(a["boxes"], b["boxes"]))
    on.mosaic_prob = 1.5
    with pytest.raises(ValueError):
        list(on.plan())


def test_rank_shards_are_slices_of_the_one_rank_plan():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(20)
    kw = dict(letterbox=True, zoom_out=0.4, mosaic_prob=0.7)
    full = list(TrainLoader(ds, _cfg(**kw), seed=3).plan())
    for world in (2, 3, 4):
        parts = [list(TrainLoader(ds, _cfg(**kw), seed=3, rank=r, world=world).plan()) for r in range(world)]
        for it, ref in enumerate(full):
            for k in ("index", "aug", "mosaic_index", "source_aug", "source_index"):
                assert np.array_equal(np.concatenate([p[it][k] for p in parts]), ref[k]), (world, it, k)
            # the tiles: the same but for the source rows, which count from each rank's own first source
            base, rows = 0, []
            for p in parts:
                t = p[it]["mosaic"].copy()
                t[:, :, 0] = np.where(t[:, :, 0] >= 0, t[:, :, 0] + base, -1)
                rows.append(t)
                base += len(p[it]["source_index"])
            assert np.array_equal(np.concatenate(rows), ref["mosaic"]), (world, it)
            bx = [b for p in parts for b in p[it]["boxes"]]
            assert len(bx) == len(ref["boxes"]) and all(np.array_equal(x, y) for x, y in zip(bx, ref["boxes"]))
            cl = [c for p in parts for c in p[it]["class_ids"]]
            assert all(np.array_equal(x, y) for x, y in zip(cl, ref["class_ids"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# the tile rule and the box rule
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tile_rule_equals_the_plain_loops():
    rs = np.random.RandomState(2)
    overhang = 0
    for _ in range(300):
        H, W = int(rs.randint(4, 200)), int(rs.randint(4, 400))
        d = [(int(rs.randint(1, 300)), int(rs.randint(1, 300))) for _ in range(4)]
        centre = (int(rs.randint(H // 4, H - H // 4 + 1)), int(rs.randint(W // 4, W - W // 4 + 1)))
        z = rs.uniform(0.3, 2.0, 4)
        src = int(rs.randint(0, 50))
        got = augment.mosaic_tiles(d, centre, z, (H, W), src)
        assert got.dtype == np.int32 and got.tolist() == [list(r) for r in mref.tiles_of(d, centre, z, (H, W), src)]
        augment.check_tiles(got[None], 1, src + 4)
        for _s, top, left, h1, w1, y0, x0, y1, x1 in got.tolist():          # rectangle inside canvas and window
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W and top <= y0 and y1 <= top + h1 and left <= x0 and x1 <= left + w1
            overhang += top < 0 or left < 0 or top + h1 > H or left + w1 > W
    assert overhang > 100
    assert augment.one_tile((3, 4, 10, 20), 7).tolist() == [[7, 3, 4, 10, 20, 3, 4, 13, 24]] + [[-1] * 9] * 3


def _random_sources(rs, n_boxes):
    out = []
    for _ in range(4):
        h, w = int(rs.randint(30, 120)), int(rs.randint(30, 120))
        m = int(rs.randint(*n_boxes))
        x1, y1 = rs.uniform(0, w * 0.7, m), rs.uniform(0, h * 0.7, m)
        b = np.stack([x1, y1, x1 + rs.uniform(3, w * 0.5, m), y1 + rs.uniform(3, h * 0.5, m)], 1).astype(np.float32)
        f = np.float32([[2, 2, w - 3, h - 3]]) if rs.uniform() < 0.5 else np.zeros((0, 4), np.float32)
        aug = (int(rs.randint(-h // 4, 3)), int(rs.randint(-w // 8, 3)), int(rs.randint(0, 2)))
        out.append((rs.randint(0, 3, m).astype(np.int64), b, f, (h, w), aug))
    return out


def test_box_rule_equals_the_plain_loops_and_every_branch_is_taken():
    rs = np.random.RandomState(6)
    H, W = 96, 160
    total = {"whole": 0, "clipped": 0, "dropped": 0}
    ignored = kept_n = 0
    for it in range(120):
        sources = _random_sources(rs, (0, 4))
        centre = (int(rs.randint(H // 4, H - H // 4 + 1)), int(rs.randint(W // 4, W - W // 4 + 1)))
        z = rs.uniform(0.5, 2.0, 4)
        d = [(s[0] - a[0], s[1] - a[1]) for _, _, _, s, a in sources]
        rows = mref.tiles_of(d, centre, z, (H, W))
        vis = (0.0, 0.25, 0.6, 1.0)[it % 4]
        for ignore in (False, True):
            c_ref, b_ref, i_ref, counts = mref.boxes_of(sources, rows, vis, ignore)
            c, b, ign, meta = augment.transform_boxes_mosaic(sources, np.array(rows, np.int32), (H, W), vis, ignore)
            assert np.array_equal(c, c_ref) and c.dtype == np.int64 and b.dtype == np.float32 and b.shape == (len(c), 4)
            assert np.array_equal(b.view(np.uint32), b_ref.view(np.uint32)) and np.array_equal(ign.view(np.uint32), i_ref.view(np.uint32))
            assert meta["letterbox"].tolist() == list(rows[0][1:5])
        for k in total:
            total[k] += counts[k]
        ignored += len(i_ref)
        kept_n += len(b_ref)
        # every kept box has area and lies in the rectangle of a tile
        for box in b_ref:
            assert box[0] < box[2] and box[1] < box[3]
            assert any(x0 <= box[0] and box[2] <= x1 - 1 and y0 <= box[1] and box[3] <= y1 - 1 for _, _, _, _, _, y0, x0, y1, x1 in rows)
    print(f"boxes kept whole / clipped and kept / dropped: {total}, ignore boxes {ignored}")
    assert total["whole"] > 20 and total["clipped"] > 20 and total["dropped"] > 20 and ignored > 20 and kept_n == total["whole"] + total["clipped"]


def test_fallback_keeps_an_image_with_objects_from_becoming_object_free():
    """Under the reference alone: an image whose own source has a box while the mosaic keeps none takes the fallback, the one-tile image of
    its own source (all its boxes, its own letterbox window); the loader does the same."""
    from squeezedet_pytorch_amd.annotations import split_flagged
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _FlaggedDataset(40)
    cfg = _cfg(letterbox=True, mosaic_prob=1.0, mosaic_scale=(0.3, 0.6), mosaic_min_visible=1.0, sparse_gt=True, ignore_overlap=0.5)
    loader = TrainLoader(ds, cfg, seed=2)
    fallbacks = mosaics = 0
    for p in list(loader.plan()) + list(loader.plan()):
        for j, t in enumerate(p["mosaic"]):
            own = int(p["index"][j])
            n_own = len(split_flagged(ds.load_annotations(own))[1])
            srcs = p["source_index"][t[0, 0]:t[0, 0] + 4]
            assert len(srcs) == 4 and srcs[0] == own                          # prob 1: every image drew partners and uploads them
            ann = [split_flagged(ds.load_annotations(int(q))) for q in srcs]
            sizes = [ds.images[int(q)].shape[:2] for q in srcs]
            augs = p["source_aug"][t[0, 0]:t[0, 0] + 4]
            if augment.tile_count(t) == 4:
                mosaics += 1
                rows = [tuple(int(v) for v in r) for r in t]
                local = [(r[0] - t[0, 0],) + r[1:] for r in rows]
                d = [(s[0] - int(g[0]), s[1] - int(g[1])) for s, g in zip(sizes, augs)]
                assert local == mref.tiles_of(d, p["mosaic_draw"]["centre"][j], p["mosaic_draw"]["scale"][j], CANVAS)
                _c, b_ref, i_ref, _n = mref.boxes_of([(a[0], a[1], a[2], s, g) for a, s, g in zip(ann, sizes, augs)], local, 1.0, True)
                assert len(b_ref) > 0 or n_own == 0
                assert np.array_equal(p["boxes"][j], b_ref) and np.array_equal(p["ignore_boxes"][j], i_ref)
                assert np.array_equal(p["mosaic_index"][j], srcs)
            else:
                fallbacks += 1
                assert n_own > 0 and len(p["boxes"][j]) == n_own
                assert np.array_equal(t, augment.one_tile(p["window"][j], t[0, 0])) and p["mosaic_index"][j].tolist() == [own, -1, -1, -1]
                # ... and the mosaic it would have been keeps no box, by the reference's loops alone
                d = [(s[0] - int(g[0]), s[1] - int(g[1])) for s, g in zip(sizes, augs)]
                rows = mref.tiles_of(d, p["mosaic_draw"]["centre"][j], p["mosaic_draw"]["scale"][j], CANVAS)
                _c, b_ref, _i, _n = mref.boxes_of([(a[0], a[1], a[2], s, g) for a, s, g in zip(ann, sizes, augs)], rows, 1.0, True)
                assert len(b_ref) == 0
    print(f"fallbacks {fallbacks}, mosaics {mosaics}")
    assert fallbacks > 0 and mosaics > 0


def test_the_yardsticks_block_resize_is_the_oracles():
    import oracle
    rs = np.random.RandomState(0)
    v = rs.standard_normal((7, 11, 3)).astype(np.float32)
    full = oracle.resize_linear_f32(v, (3000, 2000))                          # large enough for the block path
    got = mref.resize_window(v, 3000, 2000, (1490, 1530), (990, 1020))
    assert np.array_equal(got, full[1490:1530, 990:1020])


# ---------------------------------------------------------------------------------------------------------------------------------
# layout, arguments, cfg
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pack_layout_and_write_header_without_tiles_are_byte_identical_to_before():
    rs = np.random.RandomState(1)
    for B in (1, 3, 20):
        sizes = [(int(rs.randint(1, 50)), int(rs.randint(1, 50))) for _ in range(B)]
        aug = rs.randint(-5, 5, (B, 3)).astype(np.int32)
        color = rs.uniform(0.5, 1.5, (B, 3)).astype(np.float32)
        win = rs.randint(0, 9, (B, 4)).astype(np.int32)
        for with_color in (False, True):
            for with_win in (False, True):
                hdr, offsets, total = augment.pack_layout(sizes, with_color, with_win)
                used = 28 * B + (12 * B if with_color else 0) + (16 * B if with_win else 0)
                assert hdr == -(-used // 256) * 256 and total == hdr + sum(h * w * 3 for h, w in sizes)      # the layout as it was
                assert np.array_equal(offsets, np.cumsum([0] + [h * w * 3 for h, w in sizes[:-1]]))
                got = np.full(hdr, 0xAB, np.uint8)
                augment.write_header(got, offsets, sizes, aug, color if with_color else None, win if with_win else None)
                want = np.full(hdr, 0xAB, np.uint8)                           # the blocks written out by hand, where they were
                want[:8 * B] = offsets.astype(np.int64).view(np.uint8)
                want[8 * B:16 * B] = np.asarray(sizes, np.int32).reshape(-1).view(np.uint8)
                want[16 * B:28 * B] = aug.reshape(-1).view(np.uint8)
                o = 28 * B
                if with_color:
                    want[o:o + 12 * B] = color.reshape(-1).view(np.uint8)
                    o += 12 * B
                if with_win:
                    want[o:o + 16 * B] = win.reshape(-1).view(np.uint8)
                assert np.array_equal(got, want), (B, with_color, with_win)
        # the mosaic layout: S source rows, the tile block, the B colour rows
        S, Bo = B, -(-B // 4)
        tiles = rs.randint(-1, 60, (Bo, 4, 9)).astype(np.int32)
        for with_color in (False, True):
            hdr, offsets, total = augment.pack_layout(sizes, with_color, tiles=Bo)
            assert hdr == -(-(28 * S + 144 * Bo + (12 * Bo if with_color else 0)) // 256) * 256 and augment.tiles_offset(S) == 28 * S
            got = np.full(hdr, 0xAB, np.uint8)
            augment.write_header(got, offsets, sizes, aug, color[:Bo] if with_color else None, tiles=tiles)
            assert np.array_equal(got[28 * S:28 * S + 144 * Bo].view(np.int32).reshape(Bo, 4, 9), tiles)
            assert np.array_equal(got[16 * S:28 * S].view(np.int32).reshape(S, 3), aug)
            if with_color:
                assert np.array_equal(got[28 * S + 144 * Bo:28 * S + 156 * Bo].view(np.float32).reshape(Bo, 3), color[:Bo])
            assert np.all(got[28 * S + 144 * Bo + (12 * Bo if with_color else 0):] == 0xAB)
    with pytest.raises(ValueError):
        augment.pack_layout([(3, 3)], window=True, tiles=1)


def test_cfg_fields_and_their_checks():
    from types import SimpleNamespace
    from squeezedet_pytorch_amd.config import check_geometry, check_mosaic
    from squeezedet_pytorch_amd.train_data import TrainLoader
    cfg = sqd.make_cfg(device="cpu")
    assert cfg.mosaic_prob == 0. and tuple(cfg.mosaic_scale) == (0.5, 1.0) and cfg.mosaic_min_visible == 0.25
    assert check_mosaic(SimpleNamespace(), "t") == (0.0, (0.5, 1.0), 0.25)                        # a bare cfg: off
    assert check_geometry(sqd.make_cfg(device="cpu", letterbox=True, mosaic_prob=0.5), "t") == (True, 0.0)      # ... and as it was
    ok = sqd.make_cfg(device="cpu", letterbox=True, mosaic_prob=1.0, mosaic_scale=(0.25, 2.0), mosaic_min_visible=0.0)
    assert check_mosaic(ok, "t") == (1.0, (0.25, 2.0), 0.0)
    ds = _MemDataset(6)
    bad = [dict(mosaic_prob=v) for v in (-0.1, 1.1, float("nan"), float("inf"), "0.5", None, True)]
    bad += [dict(mosaic_prob=0.5, mosaic_scale=v) for v in ((0., 1.), (-1., 1.), (1.2, 1.0), (0.5, 2.5), (0.5,), 0.7, (float("nan"), 1.), None)]
    bad += [dict(mosaic_prob=0.5, mosaic_min_visible=v) for v in (-0.1, 1.5, float("nan"), None)]
    for kw in bad:
        with pytest.raises(ValueError):
            sqd.make_cfg(device="cpu", letterbox=True, **kw)
        cfg = _cfg(letterbox=True)
        for k, v in kw.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError):
            TrainLoader(ds, cfg)
    with pytest.raises(ValueError):
        sqd.make_cfg(device="cpu", mosaic_prob=0.5)                                               # without letterbox
    with pytest.raises(ValueError):
        sqd.make_cfg(device="cpu", mosaic_prob=0.5, forbid_resize=True)
    with pytest.raises(ValueError):
        sqd.make_cfg(device="cpu", mosaic_prob=0.5, forbid_resize=True, letterbox=True)
    cfg = _cfg()
    cfg.mosaic_prob = 0.3                                                                         # set without letterbox
    with pytest.raises(ValueError):
        TrainLoader(ds, cfg)
    sqd.make_cfg(device="cpu", mosaic_scale=(0.5, 1.5), mosaic_min_visible=0.5)                   # off: the other fields alone are fine
    # a reference-style namespace without the fields means off
    cfg = _cfg(letterbox=True)
    for k in ("mosaic_prob", "mosaic_scale", "mosaic_min_visible"):
        delattr(cfg, k)
    assert all("mosaic" not in p for p in TrainLoader(ds, cfg).plan())


def test_launch_u8_knows_the_mosaic_geometry():
    from squeezedet_pytorch_amd.preprocess import entry_name
    assert entry_name("mosaic", aug=True) == "sqd_preprocess_u8_mosaic_aug_fwd"
    assert entry_name("mosaic", aug=True, color=True) == "sqd_preprocess_u8_mosaic_aug_color_fwd"
    with pytest.raises(ValueError):
        entry_name("mosaic", aug=False)
    with pytest.raises(ValueError):
        entry_name("mosaic", aug=False, color=True)


def test_entry_points_are_declared_and_refuse_bad_arguments_on_the_host():
    import __graft_entry__ as ge
    ge.build()
    from squeezedet_pytorch_amd import _native as nat
    lib = nat.lib()
    null = ctypes.c_void_p(0)
    keep = (ctypes.c_ulonglong * 8)()               # a non-null, 8-byte aligned host address; never dereferenced (no launch happens)
    p = ctypes.c_void_p(ctypes.addressof(keep))
    mean, std = (ctypes.c_float * 3)(1., 2., 3.), (ctypes.c_float * 3)(4., 5., 6.)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    header = open(os.path.join(root, "include", "sqd_hip.h")).read()
    # (src, offsets, sizes, aug, tiles, [color, sums,] out, mean, std, B, S, H, W, stream): every pointer is required
    cases = {"sqd_preprocess_u8_mosaic_aug_fwd": [p] * 6, "sqd_preprocess_u8_mosaic_aug_color_fwd": [p] * 8}
    for name, ptrs in cases.items():
        assert hasattr(lib, name) and name in nat._SIGNATURES and name in integration and name in header, name
        fn = getattr(lib, name)
        for k in range(len(ptrs)):
            args = list(ptrs)
            args[k] = null
            assert fn(*args, mean, std, 1, 1, 8, 8, null) == 1, (name, k)
        for B, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 65536, 8), (1, 8, 0), (1, 8, -3), (1, 8, 65536)):
            assert fn(*ptrs, mean, std, B, max(B, 1), H, W, null) == 1, (name, B, H, W)
        for B, S in ((1, 0), (1, -2), (1, 5), (3, 13), (65535, 4 * 65535 + 1)):
            assert fn(*ptrs, mean, std, B, S, 8, 8, null) == 1, (name, B, S)
        assert fn(*ptrs, mean, (ctypes.c_float * 3)(4., 0., 6.), 1, 1, 8, 8, null) == 1           # a zero std
        assert fn(*ptrs, None, std, 1, 1, 8, 8, null) == 1 and fn(*ptrs, mean, None, 1, 1, 8, 8, null) == 1


def test_preprocess_train_batch_checks_its_mosaic_arguments():
    im = [np.zeros((8, 8, 3), np.uint8)]
    args = (im, [np.zeros(0, np.int64)], [np.zeros((0, 4), np.float32)], (16, 16), None)
    tiles = augment.one_tile((0, 0, 16, 16))[None]
    with pytest.raises(ValueError):
        augment.preprocess_train_batch(*args, device="cpu", tiles=tiles)                            # without letterbox
    with pytest.raises(ValueError):
        augment.preprocess_train_batch(*args, device="cpu", letterbox=True, sources=[[0, -1, -1, -1]])      # sources without tiles
    bad = tiles.copy()
    bad[0, 0, 0] = 1
    with pytest.raises(ValueError):
        augment.preprocess_train_batch(*args, device="cpu", letterbox=True, tiles=bad, aug=[(0, 0, 0)])     # a source that is not there
