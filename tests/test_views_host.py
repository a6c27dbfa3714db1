"""CPU tier of the pooled views (DESIGN.md section 3 "Pooled views"): the numpy reference's self-checks, the planner's geometry (round
trip of boxes through every builder's windows, tile coverage), the packed upload, the C ABI's refusals and the cfg / Detector checks."""
import ctypes

import numpy as np
import pytest

import nms_ref
import views_ref

F = np.float32
NMS, THR = 0.4, 0.3


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def _same_rows(a, b):
    assert np.array_equal(a['anchor_idx'], b['anchor_idx'])
    assert np.array_equal(a['class_ids'], b['class_ids'])
    assert np.array_equal(_bits(a['scores']), _bits(b['scores']))
    assert np.array_equal(_bits(a['boxes']), _bits(b['boxes']))


# ---- the reference -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,agnostic', [('hard', False), ('linear', False), ('gaussian', True)])
def test_ref_one_identity_view_is_soft_filter(mode, agnostic):
    cls, sc, bx = nms_ref.make_case(3, 2, 150, 3)
    for b in range(2):
        got = views_ref.pooled_filter(cls[b][None], sc[b][None], bx[b][None], views_ref.IDENTITY[None], 64, NMS, THR, 3, mode, 0.5, agnostic)
        exp = nms_ref.soft_filter(cls[b], sc[b], bx[b], 64, NMS, THR, 3, mode, 0.5, agnostic)
        assert len(exp['scores']) > 0
        _same_rows(got, exp)


def test_ref_two_identical_views_keep_view_zero():
    A, K = 150, 256
    cls, sc, bx = nms_ref.make_case(4, 2, A, 3)
    xf = np.stack([views_ref.IDENTITY] * 2)
    for b in range(2):
        assert 2 * int((sc[b] > F(THR)).sum()) <= K                  # the whole pool is taken
        got = views_ref.pooled_filter(np.stack([cls[b]] * 2), np.stack([sc[b]] * 2), np.stack([bx[b]] * 2), xf, K, NMS, THR, 3, 'hard')
        exp = nms_ref.soft_filter(cls[b], sc[b], bx[b], K, NMS, THR, 3, 'hard')
        assert len(exp['scores']) > 0 and np.all(got['anchor_idx'] < A)      # ties go to view 0, whose copy suppresses view 1's (IoU 1)
        _same_rows(got, exp)


def test_ref_map_boxes_is_the_stated_expression():
    b = np.array([[10.5, 3.25, 40.0, 30.0]], F)
    xf = np.array([0.5, 0.75, -7.0, 2.5, 1.0, 99.0], F)
    x1, x2 = F(F(10.5) / F(0.75)) + F(2.5), F(F(40.0) / F(0.75)) + F(2.5)
    y1, y2 = F(F(3.25) / F(0.5)) + F(-7.0), F(F(30.0) / F(0.5)) + F(-7.0)
    got = views_ref.map_boxes(b, xf)
    assert np.array_equal(_bits(got), _bits([[F(99.0) - x2, y1, F(99.0) - x1, y2]]))
    assert np.array_equal(_bits(views_ref.map_boxes(b, views_ref.IDENTITY)), _bits(b))


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
def _sizes(rs, n):
    fixed = [(9, 17), (2160, 3840), (17, 9), (375, 1242)]
    return fixed + [(int(rs.randint(9, 2161)), int(rs.randint(17, 3841))) for _ in range(n - len(fixed))]


def _builders(size, canvas):
    from squeezedet_pytorch_amd import views
    H, W = canvas
    out = [views.tta_views(), views.tta_views(flip=False, zooms=(1.0, 0.75, 1.5)), views.tta_views(flip=True, zooms=(0.5, 2.0)),
           views.tile_views(size, (H, W), (H // 4, W // 4)), views.tile_views(size, (max(1, size[0] // 2), max(1, size[1] // 3)), 0)]
    return out


@pytest.mark.parametrize('letterbox', [False, True])
def test_planner_round_trip(letterbox):
    """Boxes inside the part of the image a view shows go forward with ``augment.transform_boxes`` (the view's window and aug) and come
    back with ``views_ref.map_boxes`` within 8 * 2^-24 * M, M the largest coordinate magnitude met on the way."""
    from squeezedet_pytorch_amd import augment, views
    rs = np.random.RandomState(11)
    canvas = (384, 1248)
    worst = 0.0
    for size in _sizes(rs, 12):
        for vlist in _builders(size, canvas):
            plan = views.plan_views([size], vlist, canvas, letterbox=letterbox)
            assert plan.V == len(vlist) and plan.view_xf.shape == (len(vlist), 6) and plan.view_xf.dtype == np.float32
            for k, v in enumerate(vlist):
                win = tuple(int(t) for t in plan.windows[k])
                assert win == views.view_window(size, v, canvas, letterbox)
                assert tuple(plan.tiles[k, 0]) == (plan.tiles[k, 0, 0],) + win + (0, 0) + canvas and plan.tiles[k, 1, 0] < 0
                aug = plan.src_aug[plan.tiles[k, 0, 0]]
                assert tuple(aug) == (0, 0, int(v.flip)) and plan.src_image[plan.tiles[k, 0, 0]] == 0
                y0, x0, y1, x1 = views.visible_rect(size, win, canvas, v.flip)
                assert y1 >= y0 and x1 >= x0
                n = 16
                xs = np.sort(rs.uniform(x0, x1, (n, 2)), 1)
                ys = np.sort(rs.uniform(y0, y1, (n, 2)), 1)
                boxes = np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], 1).astype(F)
                fwd, meta = augment.transform_boxes(boxes, size, aug, canvas, False, True, win, overhang=True)
                xf = plan.view_xf[k]
                assert np.array_equal(xf[:2], meta['scales']) and xf[2] == -meta['padding'][0] and xf[3] == -meta['padding'][2]
                assert xf[4] == float(v.flip) and xf[5] == size[1] - 1
                back = views_ref.map_boxes(fwd, xf)
                unshift = np.abs(fwd.astype(np.float64) - np.array([win[1], win[0], win[1], win[0]]))        # x * sx before the shift
                M = max(np.abs(boxes).max(), np.abs(fwd).max(), unshift.max(), (np.abs(fwd)[:, [0, 2]] / xf[1]).max(),
                        (np.abs(fwd)[:, [1, 3]] / xf[0]).max(), np.abs(back).max(), abs(float(xf[2])), abs(float(xf[3])), float(xf[5]),
                        abs(win[0]), abs(win[1]))
                err = np.abs(back.astype(np.float64) - boxes.astype(np.float64)).max()
                worst = max(worst, err / (2.0 ** -24 * M))
                assert err <= 8 * 2.0 ** -24 * M, (size, v, win, err, M)
    print(f'worst round-trip error: {worst:.2f} x 2^-24 M')


def test_tiles_cover_the_frame_and_overlap():
    from squeezedet_pytorch_amd import views
    rs = np.random.RandomState(5)
    cases = [((200, 300), (64, 96), 16), ((2160, 3840), (384, 1248), 64), ((50, 3000), (384, 1248), (0, 100)), ((64, 96), (64, 96), 8),
             ((65, 97), (64, 96), 63)]
    cases += [((int(rs.randint(9, 700)), int(rs.randint(17, 900))), (int(rs.randint(8, 200)), int(rs.randint(8, 300))), 0) for _ in range(6)]
    for size, tile, overlap in cases:
        if np.ndim(overlap) == 0:
            overlap = min(int(overlap), tile[0] - 1, tile[1] - 1)
        oy, ox = (overlap, overlap) if np.ndim(overlap) == 0 else overlap
        vs = views.tile_views(size, tile, overlap)
        seen = np.zeros(size, np.int32)
        for v in vs:
            ry, rx, rh, rw = v.rect
            assert v.zoom == 1.0 and not v.flip and rh == min(tile[0], size[0]) and rw == min(tile[1], size[1])
            assert 0 <= ry and ry + rh <= size[0] and 0 <= rx and rx + rw <= size[1]
            seen[ry:ry + rh, rx:rx + rw] += 1
        assert seen.min() >= 1, (size, tile, overlap)
        ys, xs = sorted({v.rect[0] for v in vs}), sorted({v.rect[1] for v in vs})
        assert len(vs) == len(ys) * len(xs)
        rh, rw = vs[0].rect[2:]
        assert all(a + rh - b >= oy for a, b in zip(ys, ys[1:])) and all(a + rw - b >= ox for a, b in zip(xs, xs[1:])), (size, tile, overlap)
    with pytest.raises(ValueError):
        views.tile_views((100, 100), (64, 64), 64)


def test_native_tile_is_seen_at_scale_one():
    """A tile of the canvas' size is shown 1 : 1 and its top-left pixel lands on the canvas' corner."""
    from squeezedet_pytorch_amd import views
    for letterbox in (False, True):
        plan = views.plan_views([(200, 300)], views.tile_views((200, 300), (64, 96), 16), (64, 96), letterbox=letterbox)
        for v, win, xf in zip(plan.views[0], plan.windows, plan.view_xf):
            assert tuple(win) == (-v.rect[0], -v.rect[1], 200, 300)
            assert tuple(xf) == (1.0, 1.0, float(v.rect[0]), float(v.rect[1]), 0.0, 299.0)


def test_upload_stores_every_image_once():
    from squeezedet_pytorch_amd import augment, views
    rs = np.random.RandomState(2)
    sizes = [(20, 31), (9, 17), (40, 25)]
    images = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in sizes]
    vlist = views.tta_views(flip=True, zooms=(1.0, 0.75))
    plan = views.plan_views(sizes, vlist, (64, 96))
    buf, hdr, offsets = views.pack_views(images, plan)
    S, BV = 6, 12
    assert len(plan.src_image) == S and plan.tiles.shape == (BV, 4, 9)
    assert hdr == augment.pack_layout([sizes[i] for i in plan.src_image], tiles=BV)[0]
    assert buf.shape == (hdr + sum(h * w * 3 for h, w in sizes),)
    off = buf[:8 * S].view(np.int64)
    assert np.array_equal(off, offsets)
    assert off[0] == off[1] == 0 and off[2] == off[3] == 20 * 31 * 3 and off[4] == off[5] == off[2] + 9 * 17 * 3
    assert np.array_equal(buf[8 * S:16 * S].view(np.int32).reshape(S, 2), np.repeat(np.array(sizes, np.int32), 2, 0))
    assert np.array_equal(buf[16 * S:28 * S].view(np.int32).reshape(S, 3), [[0, 0, 0], [0, 0, 1]] * 3)
    t0 = augment.tiles_offset(S)
    assert np.array_equal(buf[t0:t0 + 4 * 36 * BV].view(np.int32).reshape(BV, 4, 9), plan.tiles)
    for im, o in zip(images, off[::2]):
        assert np.array_equal(buf[hdr + o:hdr + o + im.size], im.reshape(-1))
    assert 1 <= S <= 4 * BV
    # an image none of whose views is flipped has one source row
    plan1 = views.plan_views(sizes[:1], views.tta_views(flip=False), (64, 96))
    assert len(plan1.src_image) == 1 and views.pack_views(images[:1], plan1)[0].shape[0] == views.pack_views(images[:1], plan1)[1] + 20 * 31 * 3


def test_planner_refusals():
    from squeezedet_pytorch_amd import views
    with pytest.raises(ValueError):
        views.plan_views([(20, 30)], views.tta_views(), (64, 96), forbid_resize=True)
    with pytest.raises(ValueError):
        views.plan_views([(20, 30), (20, 30)], [views.tta_views(), views.tta_views(flip=False)], (64, 96))      # unequal view counts
    with pytest.raises(ValueError):
        views.view_window((20, 30), views.View(1.0, False, (0, 0, 21, 30)), (64, 96))
    for bad in ((), (0.0,), (float('nan'),), (-1.0,), (17.0,)):
        with pytest.raises(ValueError):
            views.tta_views(zooms=bad)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_detect_views_status_codes_without_gpu():
    """Status 1 / 2 are decided on the host, nothing is launched (there is no GPU here)."""
    from squeezedet_pytorch_amd import _native as nat
    lib = nat.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    odd = ctypes.c_void_p(p.value + 4)
    null = ctypes.c_void_p(0)

    def det(B=1, V=2, A=4, C=3, K=4, thr=0.3, ws=8, mode=0, sigma=0.5, agn=0, pred=p, xf=p, keys=p, box=p):
        return lib.sqd_detect_views_fwd(pred, p, xf, keys, p, p, p, box, p, B, V, A, C, 64, 64, K, 0.4, thr, ws, mode, sigma, agn, null)
    assert det(pred=null) == nat.ERR_BAD_ARG and det(xf=null) == nat.ERR_BAD_ARG and det(keys=null) == nat.ERR_BAD_ARG
    assert det(V=0) == nat.ERR_BAD_ARG and det(V=-1) == nat.ERR_BAD_ARG
    assert det(ws=7) == nat.ERR_BAD_ARG and det(keys=odd) == nat.ERR_BAD_ARG and det(box=odd) == nat.ERR_BAD_ARG
    assert det(A=5, V=3, ws=23) == nat.ERR_BAD_ARG                       # 3 x ceil4(5) = 24 words
    assert det(mode=3) == nat.ERR_BAD_ARG and det(mode=2, sigma=0.0) == nat.ERR_BAD_ARG and det(mode=2, sigma=float('nan')) == nat.ERR_BAD_ARG
    assert det(thr=-0.1) == nat.ERR_BAD_ARG and det(K=0) == nat.ERR_BAD_ARG and det(B=0) == nat.ERR_BAD_ARG
    assert det(V=(1 << 18) + 1, ws=1 << 30) == nat.ERR_UNSUPPORTED         # V * ceil4(A) = 2^20 + 4
    assert det(V=1 << 18, A=5, ws=1 << 30) == nat.ERR_UNSUPPORTED          # ceil4: 2^18 * 8
    assert det(K=1025, ws=1 << 20) == nat.ERR_UNSUPPORTED and det(C=257) == nat.ERR_UNSUPPORTED
    assert det(B=1 << 12, V=1 << 10, A=1 << 10, ws=1 << 30) == nat.ERR_UNSUPPORTED      # 2^32 workspace words


def test_detect_views_argument_checks_without_gpu():
    import torch
    from squeezedet_pytorch_amd import ops
    pred = torch.zeros(4, 8, 8)
    with pytest.raises(ValueError):
        ops.detect_views(pred, torch.zeros(8, 4), (64, 64), 3, 2, torch.zeros(4, 6))          # not on the device
    with pytest.raises(ValueError):
        ops.detect_views(pred, torch.zeros(8, 4), (64, 64), 3, 2, torch.zeros(4, 6), nms_mode='nope')


# ---- cfg and Detector ----------------------------------------------------------------------------------------------------------------
def test_make_cfg_tta_fields():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd.config import check_tta
    cfg = sqd.make_cfg(device='cpu')
    assert cfg.tta_flip is False and cfg.tta_zooms is None and check_tta(cfg, 't') == (False, None, False)
    assert check_tta(sqd.make_cfg(device='cpu', tta_flip=True), 't') == (True, None, True)
    assert check_tta(sqd.make_cfg(device='cpu', tta_zooms=[1, 0.75]), 't') == (False, (1.0, 0.75), True)
    for bad in ({'tta_flip': 1}, {'tta_zooms': ()}, {'tta_zooms': (0.0,)}, {'tta_zooms': 'x'}, {'tta_zooms': (float('inf'),)},
                {'tta_flip': True, 'forbid_resize': True}, {'tta_zooms': (1.0,), 'forbid_resize': True}):
        with pytest.raises(ValueError):
            sqd.make_cfg(device='cpu', **bad)


def test_detector_refuses_what_it_cannot_pool():
    import torch
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import views
    from squeezedet_pytorch_amd.detector import Detector
    images = [np.zeros((20, 30, 3), np.uint8)]
    det = Detector(torch.nn.Identity(), sqd.make_cfg(device='cpu', forbid_resize=True))
    with pytest.raises(ValueError):
        det.detect_images(images, views=views.tta_views())
    for kw in ({'tta_flip': True}, {'tta_zooms': (1.0, 0.75)}):
        det = Detector(torch.nn.Identity(), sqd.make_cfg(device='cpu', **kw))
        assert len(det._default_views()) == 2
        with pytest.raises(NotImplementedError):
            det.detect_dataset([])
        with pytest.raises(NotImplementedError):
            next(iter(det.detect_stream([images])))
        with pytest.raises(NotImplementedError):
            det.stream()
    assert Detector(torch.nn.Identity(), sqd.make_cfg(device='cpu'))._default_views() is None
