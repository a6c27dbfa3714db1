"""Letterbox and zoom-out, host side (CPU tier; DESIGN.md 6b "Letterbox and zoom-out"): the integer window rule, the box transform
and its way home through ``boxes_postprocess``, the zoom draws of ``TrainLoader.plan`` (a stream of their own, rank shards), the
upload layout, the argument checks of the three entry points and the ``cfg`` fields."""
import ctypes
import os

import numpy as np
import pytest

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment
from squeezedet_pytorch_amd import boxes as host_boxes

import letterbox_ref as lref

CANVASES = [(384, 1248), (64, 96), (61, 517), (96, 64)]


# ---------------------------------------------------------------------------------------------------------------------------------
# the window rule
# ---------------------------------------------------------------------------------------------------------------------------------
def _float_window(size, canvas):
    """float64: scale by min(H / Hd, W / Wd), round half up."""
    hd, wd = size
    H, W = canvas
    s = min(H / hd, W / wd)
    h1, w1 = max(1, int(np.floor(hd * s + 0.5))), max(1, int(np.floor(wd * s + 0.5)))
    return (H - h1) // 2, (W - w1) // 2, h1, w1


def _is_tie(size, canvas):
    """Whether the free side's exact value lies on a .5 boundary (where float64 rounding may fall either way)."""
    hd, wd = size
    H, W = canvas
    num, den = (wd * H, hd) if H * wd <= W * hd else (hd * W, wd)
    return (2 * num) % (2 * den) == den


@pytest.mark.parametrize("canvas", CANVASES)
def test_window_rule_equals_float64_round_half_up(canvas):
    """Two grids on which the float64 form cannot differ from the integer rule.  (a) Hd and Wd both powers of two, 1 .. 4096 (169
    pairs): H / Hd, W / Wd and both products are exact in float64, ties included.  (b) every size 1 .. 64 x 1 .. 64 whose free side is
    not an exact tie: it is then at least 1 / 128 away from the boundary, against a float64 error below 2^-40."""
    pows = [1 << k for k in range(13)]
    for hd in pows:
        for wd in pows:
            assert host_boxes.letterbox_window((hd, wd), canvas) == _float_window((hd, wd), canvas), (hd, wd)
    checked = 0
    for hd in range(1, 65):
        for wd in range(1, 65):
            if not _is_tie((hd, wd), canvas):
                assert host_boxes.letterbox_window((hd, wd), canvas) == _float_window((hd, wd), canvas), (hd, wd)
                checked += 1
    assert checked > 3500


@pytest.mark.parametrize("canvas", CANVASES)
def test_window_rule_invariants(canvas):
    H, W = canvas
    sizes = [(h, w) for h in range(1, 65) for w in range(1, 65)] + [(33, 3001), (1, 3001), (3001, 1), (500, 375), (375, 1242), (40, 3000)]
    for hd, wd in sizes:
        top, left, h1, w1 = host_boxes.letterbox_window((hd, wd), canvas)
        assert (top, left, h1, w1) == lref.window((hd, wd), canvas)
        assert 1 <= h1 <= H and 1 <= w1 <= W and (h1 == H or w1 == W), (hd, wd)
        assert top == (H - h1) // 2 and left == (W - w1) // 2 and top >= 0 and left >= 0
        # the free side is the exact aspect-preserving size rounded to an integer (or the floor of 1)
        if h1 == H and H * wd <= W * hd:
            assert w1 == 1 or abs(w1 - wd * H / hd) <= 0.5
        else:
            assert h1 == 1 or abs(h1 - hd * W / wd) <= 0.5
    assert host_boxes.letterbox_window((192, 624), (384, 1248)) == (0, 0, 384, 1248)
    assert host_boxes.letterbox_window((375, 1242), (384, 1248)) == (3, 0, 377, 1248)       # not an exact fit: h1 = 377
    with pytest.raises(ValueError):
        host_boxes.letterbox_window((0, 5), canvas)


def test_letterbox_meta_is_the_padding_in_original_pixels():
    m = host_boxes.letterbox_meta((500, 375), (0, 480, 384, 288), (384, 1248))
    s, sh, pad = lref.scales_shifts_padding((500, 375), (0, 480, 384, 288), (384, 1248))
    assert m["scales"].dtype == np.float32 and m["padding"].dtype == np.float32 and m["letterbox"].dtype == np.int32
    assert np.array_equal(m["scales"], s) and np.array_equal(m["padding"], pad) and m["letterbox"].tolist() == [0, 480, 384, 288]
    assert np.array_equal(-m["padding"][[0, 2]], sh)                     # what the detect kernels add
    with pytest.raises(ValueError):
        host_boxes.letterbox_meta((500, 375), (0, 1000, 384, 288), (384, 1248))


# ---------------------------------------------------------------------------------------------------------------------------------
# boxes: there and back
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def _gold_boxes(gold):
    """Every (boxes, image size, draw) of the fixture tests/test_augment_host.py uses: drifts of both signs, flipped and not."""
    for c in range(int(gold["n"])):
        for k, (h, w, _s) in enumerate(gold[f"c{c}_images"]):
            yield gold[f"c{c}_i{k}_boxes_in"], (int(h), int(w)), gold[f"c{c}_aug"][k]


@pytest.mark.parametrize("canvas", [(384, 1248), (96, 64)])
def test_boxes_round_trip_through_boxes_postprocess(gold, canvas):
    """``boxes_postprocess(transform_boxes(b, letterbox=True), meta)`` is ``clip_boxes(b)`` within 2^-9 px: four float32 operations
    (scale, shift, divide, subtract), each at most half an ulp of a value below 2^13 = 2^-11.  Centred and zoomed windows."""
    n, flips, signs = 0, set(), set()
    for b, size, aug in _gold_boxes(gold):
        hd, wd = size[0] - int(aug[0]), size[1] - int(aug[1])
        centred = host_boxes.letterbox_window((hd, wd), canvas)
        zoomed = augment.draw_zoom(np.random.RandomState(n), [centred], canvas, 0.5)[0]
        for win in (None, zoomed):
            tb, meta = augment.transform_boxes(b, size, aug, canvas, letterbox=True, window=win)
            assert tb.dtype == np.float32 and meta["letterbox"].tolist() == list(centred if win is None else win)
            want = augment.clip_boxes(b, size)
            assert want.max() < 8192
            back = host_boxes.boxes_postprocess(tb.copy(), meta)
            assert np.abs(back.astype(np.float64) - want).max() <= 2.0 ** -9, (size, aug, win)
            # the forward transform, op for op: clip, drift, flip, then x * sx + left, y * sy + top in float32
            ref, _ = augment.transform_boxes(b, size, aug, (hd, wd), forbid_resize=True)      # same size: no padding, no crop
            sy, sx = meta["scales"]
            top, left = np.float32(meta["letterbox"][0]), np.float32(meta["letterbox"][1])
            assert np.array_equal(tb, np.stack([ref[:, 0] * sx + left, ref[:, 1] * sy + top, ref[:, 2] * sx + left, ref[:, 3] * sy + top], 1))
            # the scale / padding terms through the pinned restatement of the reference's boxes_postprocess: the same array
            part = {k: meta[k] for k in ("scales", "padding")}
            mine = host_boxes.boxes_postprocess(tb.copy(), part)
            theirs = oracle.boxes_unpad_uncrop(oracle.boxes_postprocess(tb, meta["scales"]), meta["padding"], np.zeros(4, np.float32))
            assert np.array_equal(mine, theirs)
        n += 1
        flips.add(bool(aug[2])); signs.add((np.sign(aug[0]), np.sign(aug[1])))
    assert n >= 8 and flips == {True, False} and len(signs) >= 3


def test_transform_boxes_refuses_two_geometries_and_keeps_the_old_paths():
    b = np.array([[3., 4., 30., 20.]], np.float32)
    with pytest.raises(ValueError):
        augment.transform_boxes(b, (40, 70), (0, 0, 0), (32, 64), True, True)
    for forbid in (False, True):
        old, m = augment.transform_boxes(b, (40, 70), (2, -3, 1), (32, 64), forbid)
        assert "letterbox" not in m and ("scales" in m) == (not forbid)


# ---------------------------------------------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------------------------------------------
def test_draw_zoom_is_three_draws_per_image_in_order():
    canvas = (64, 96)
    wins = np.array([[0, 8, 64, 80], [16, 0, 32, 96], [0, 47, 64, 1]], np.int32)
    got = augment.draw_zoom(np.random.RandomState(9), wins, canvas, 0.5)
    rs = np.random.RandomState(9)
    for w, g in zip(wins, got):
        z = rs.uniform(0.5, 1.0)
        h1, w1 = max(1, int(np.floor(w[2] * z + 0.5))), max(1, int(np.floor(w[3] * z + 0.5)))
        top = rs.randint(0, 64 - h1 + 1)
        left = rs.randint(0, 96 - w1 + 1)
        assert g.tolist() == [top, left, h1, w1]
    assert got.dtype == np.int32 and wins[0].tolist() == [0, 8, 64, 80]      # the input is not written
    for bad in (0., 1., -0.1, float("nan")):
        with pytest.raises(ValueError):
            augment.draw_zoom(np.random.RandomState(0), wins, canvas, bad)


class _MemDataset:
    """Mixed portrait / landscape images over the reference's dataset protocol."""

    def __init__(self, n, seed=0, sizes=((40, 70), (66, 37), (45, 81), (90, 30))):
        rs = np.random.RandomState(seed)
        self.images, self.ann = [], []
        for i in range(n):
            h, w = sizes[i % len(sizes)]
            self.images.append(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
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


JIT = dict(brightness_jitter=0.4, contrast_jitter=0.3, saturation_jitter=0.5)


def _cfg(**kw):
    return sqd.make_cfg(input_size=(32, 64), device="cpu", batch_size=6, **kw)


def _two_epochs(loader):
    return list(loader.plan()) + list(loader.plan())


def test_zoom_draws_leave_every_other_draw_alone_and_stay_on_the_canvas():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(20)
    off = _two_epochs(TrainLoader(ds, _cfg(**JIT), seed=3))
    box = _two_epochs(TrainLoader(ds, _cfg(letterbox=True, **JIT), seed=3))
    zoom = _two_epochs(TrainLoader(ds, _cfg(letterbox=True, zoom_out=0.5, **JIT), seed=3))
    again = _two_epochs(TrainLoader(ds, _cfg(letterbox=True, zoom_out=0.5, **JIT), seed=3))
    assert len(zoom) == 6
    shrunk = 0
    for a, b, z, z2 in zip(off, box, zoom, again):
        assert "window" not in a
        for k in ("index", "aug", "color"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], z[k]), k
        assert np.array_equal(z["window"], z2["window"]) and all(np.array_equal(x, y) for x, y in zip(z["boxes"], z2["boxes"]))
        wz, wb = np.asarray(z["window"]), np.asarray(b["window"])
        assert wz.dtype == np.int32 and wz.shape == (6, 4)
        assert np.all(wz[:, 2:] >= 1) and np.all(wz[:, :2] >= 0) and np.all(wz[:, 0] + wz[:, 2] <= 32) and np.all(wz[:, 1] + wz[:, 3] <= 64)
        assert np.all(wz[:, 2:] <= wb[:, 2:]) and np.all(2 * wz[:, 2:] + 1 >= wb[:, 2:])          # z in [0.5, 1)
        shrunk += int(np.sum(wz[:, 2] < wb[:, 2]))
        for i, (idx, g, w) in enumerate(zip(b["index"], b["aug"], wb)):                           # zoom off: the centred window
            h, wd = ds.images[int(idx)].shape[:2]
            assert tuple(w) == lref.window((h - g[0], wd - g[1]), (32, 64))
            assert z["metas"][i]["letterbox"].tolist() == wz[i].tolist()
    assert shrunk > 20
    other = _two_epochs(TrainLoader(ds, _cfg(letterbox=True, zoom_out=0.5, **JIT), seed=4))
    assert not np.array_equal(other[0]["window"], zoom[0]["window"])


def test_rank_shards_are_slices_of_the_one_rank_plan():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _MemDataset(20)
    kw = dict(letterbox=True, zoom_out=0.4)
    full = list(TrainLoader(ds, _cfg(**kw), seed=3).plan())
    for world in (2, 3, 4):
        parts = [list(TrainLoader(ds, _cfg(**kw), seed=3, rank=r, world=world).plan()) for r in range(world)]
        for it, ref in enumerate(full):
            for k in ("index", "aug", "window"):
                assert np.array_equal(np.concatenate([p[it][k] for p in parts]), ref[k]), (world, it, k)
            bx = [b for p in parts for b in p[it]["boxes"]]
            assert len(bx) == len(ref["boxes"]) and all(np.array_equal(x, y) for x, y in zip(bx, ref["boxes"]))


# ---------------------------------------------------------------------------------------------------------------------------------
# layout, arguments, cfg
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pack_layout_without_a_window_is_byte_identical_to_before():
    rs = np.random.RandomState(1)
    for B in (1, 3, 9, 10, 20, 64):
        sizes = [(int(rs.randint(1, 50)), int(rs.randint(1, 50))) for _ in range(B)]
        aug = rs.randint(-5, 5, (B, 3)).astype(np.int32)
        color = rs.uniform(0.5, 1.5, (B, 3)).astype(np.float32)
        win = rs.randint(0, 9, (B, 4)).astype(np.int32)
        for with_color in (False, True):
            hdr, offsets, total = augment.pack_layout(sizes, with_color)
            assert hdr == -(-(28 * B + (12 * B if with_color else 0)) // 256) * 256                # the layout as it was
            assert total == hdr + sum(h * w * 3 for h, w in sizes) and offsets[0] == 0
            old = np.full(hdr, 0xAB, np.uint8)
            augment.write_header(old, offsets, sizes, aug, color if with_color else None)
            hdr_w, offsets_w, total_w = augment.pack_layout(sizes, with_color, window=True)
            assert np.array_equal(offsets, offsets_w) and total_w - hdr_w == total - hdr
            assert hdr_w == -(-(44 * B + (12 * B if with_color else 0)) // 256) * 256
            new = np.full(hdr_w, 0xAB, np.uint8)
            augment.write_header(new, offsets_w, sizes, aug, color if with_color else None, win)
            used = 28 * B + (12 * B if with_color else 0)
            assert np.array_equal(new[:used], old[:used]) and np.all(old[used:] == 0xAB)           # the old blocks where they were
            off = augment.window_offset(B, with_color)
            assert off == used and np.array_equal(new[off:off + 16 * B].view(np.int32).reshape(B, 4), win)
            assert np.all(new[off + 16 * B:] == 0xAB)


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
    # (src, offsets, sizes, [aug,] win, [color, sums,] out, scales, shifts, mean, std, B, H, W, stream); required pointers by position
    cases = {"sqd_preprocess_u8_letterbox_fwd": ([p, p, p, null, p, null, null], [0, 1, 2, 4]),
             "sqd_preprocess_u8_letterbox_aug_fwd": ([p, p, p, p, null, p, null, null], [0, 1, 2, 3, 5]),
             "sqd_preprocess_u8_letterbox_aug_color_fwd": ([p, p, p, p, null, p, p, p, null, null], [0, 1, 2, 3, 5, 6, 7])}
    for name, (ptrs, required) in cases.items():
        assert hasattr(lib, name) and name in nat._SIGNATURES and name in integration, name
        fn = getattr(lib, name)
        for k in required:
            args = list(ptrs)
            args[k] = null
            assert fn(*args, mean, std, 1, 8, 8, null) == 1, (name, k)
        for B, H, W in ((0, 8, 8), (-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 65536, 8), (1, 8, 0), (1, 8, -3)):
            assert fn(*ptrs, mean, std, B, H, W, null) == 1, (name, B, H, W)
        assert fn(*ptrs, mean, (ctypes.c_float * 3)(4., 0., 6.), 1, 8, 8, null) == 1                 # a zero std
        assert fn(*ptrs, None, std, 1, 8, 8, null) == 1 and fn(*ptrs, mean, None, 1, 8, 8, null) == 1


def test_cfg_fields_and_their_checks():
    from squeezedet_pytorch_amd.train_data import TrainLoader
    cfg = sqd.make_cfg(device="cpu")
    assert cfg.letterbox is False and cfg.zoom_out == 0.
    assert sqd.make_cfg(device="cpu", letterbox=True, zoom_out=0.5).zoom_out == 0.5
    with pytest.raises(ValueError):
        sqd.make_cfg(device="cpu", letterbox=True, forbid_resize=True)
    ds = _MemDataset(6)
    for bad in (1.0, -0.1, float("nan"), float("inf"), 1.5):
        with pytest.raises(ValueError):
            sqd.make_cfg(device="cpu", letterbox=True, zoom_out=bad)
        cfg = _cfg(letterbox=True)
        cfg.zoom_out = bad
        with pytest.raises(ValueError):
            TrainLoader(ds, cfg)
    cfg = _cfg()
    cfg.zoom_out = 0.3                                  # set without letterbox
    with pytest.raises(ValueError):
        TrainLoader(ds, cfg)
    cfg = _cfg(letterbox=True)
    cfg.forbid_resize = True
    with pytest.raises(ValueError):
        TrainLoader(ds, cfg)
    bare = _cfg()
    del bare.letterbox, bare.zoom_out                   # a cfg without the fields (the reference's own): off
    ld = TrainLoader(ds, bare, seed=1)
    assert ld.letterbox is False and "window" not in next(iter(ld.plan()))


def test_stream_image_meta_under_letterbox():
    import types
    from squeezedet_pytorch_amd import lanes
    fake = types.SimpleNamespace(cfg=types.SimpleNamespace(input_size=(384, 1248)), forbid=False, letterbox=True)
    sizes = np.array([[375, 1242], [500, 375]], np.int32)
    for m, (h, w) in zip(lanes.DetectStream._image_meta(fake, sizes, ["a", "b"]), sizes):
        win = lref.window((h, w), (384, 1248))
        s, _sh, pad = lref.scales_shifts_padding((h, w), win, (384, 1248))
        assert np.array_equal(m["scales"], s) and np.array_equal(m["padding"], pad) and m["letterbox"].tolist() == list(win)
        assert "crops" not in m and m["orig_size"].tolist() == [h, w, 3]
