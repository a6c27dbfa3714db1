"""Pooled views on the MI355X (DESIGN.md section 3 "Pooled views"): ``ops.detect_views`` against the dense composition it replaces --
``ops.decode`` / ``ops.decode_many`` of every view, the fp32 mapping in torch on the device, ``cat``, ``ops.filter_dense_nms`` -- bit for
bit, and against the numpy reference tests/views_ref.py; V = 1 with the identity transform against ``ops.detect_nms``; the planner,
the one mosaic input launch and ``Detector.detect_images(views=...)`` end to end for test-time augmentation and for tiles; and the
default path left as it was."""
import numpy as np
import pytest
import torch

import nms_ref
import views_ref
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import augment, ops, synthetic, views

pytestmark = pytest.mark.gpu

F = np.float32
SIZE = (240, 400)              # canvas of the rule tests
NMS, THR = 0.4, 0.05
RULES = [('hard', False), ('linear', False), ('gaussian', False), ('hard', True)]
KS = (1, 64, 100, 1024)


def make_inputs(seed, B, V, A, C):
    """pred [B*V, A, C+5], anchors [A, 4], view_xf [B*V, 6].  Anchors in three clusters (heavy overlap); class 0 favoured (a class with
    more than 64 candidates); scales in [0.3, 3], shifts in [-50, 50], every second view flipped (V = 1: the second image);
    V >= 3: the first third of view 0's rows is copied into view 2 (exact score ties across views), and in image 0 view 2 also has view
    0's transform, so that the tied candidates are the same box twice."""
    rs = np.random.RandomState(seed)
    H, W = SIZE
    centres = np.stack([rs.uniform(80, W - 80, 3), rs.uniform(70, H - 70, 3)], 1)
    pick = rs.randint(0, 3, A)
    anchors = np.concatenate([centres[pick] + rs.normal(0, 6.0, (A, 2)), rs.uniform(60, 100, (A, 2))], 1).astype(F)
    pred = np.empty((B * V, A, C + 5), F)
    pred[..., :C] = rs.normal(0, 2.0, (B * V, A, C))
    pred[..., 0] += 1.5
    pred[..., C] = rs.normal(0, 1.5, (B * V, A))
    pred[..., C + 1:C + 3] = rs.normal(0, 0.05, (B * V, A, 2))
    pred[..., C + 3:] = rs.normal(0, 0.1, (B * V, A, 2))
    xf = np.empty((B * V, 6), F)
    xf[:, :2] = rs.uniform(0.3, 3.0, (B * V, 2))
    xf[:, 2:4] = rs.uniform(-50, 50, (B * V, 2))
    xf[:, 4] = [(r % V) % 2 if V > 1 else r % 2 for r in range(B * V)]
    xf[:, 5] = rs.randint(300, 900, B * V)
    if V >= 3:
        n = max(1, A // 3)
        for b in range(B):
            pred[b * V + 2, :n] = pred[b * V, :n]
        xf[2] = xf[0]
    return pred, anchors, xf


def decode_fn(C):
    return ops.decode if C <= 16 else ops.decode_many


def map_on_device(bx, xf):
    """The fp32 mapping of the rule in torch, one op at a time: bx [R, A, 4], xf [R, 6] -> [R, A, 4]."""
    sy, sx, dy, dx, flip, mirror = (xf[:, i].reshape(-1, 1) for i in range(6))
    x1, y1 = bx[..., 0] / sx + dx, bx[..., 1] / sy + dy
    x2, y2 = bx[..., 2] / sx + dx, bx[..., 3] / sy + dy
    f = flip != 0
    return torch.stack([torch.where(f, mirror - x2, x1), y1, torch.where(f, mirror - x1, x2), y2], -1).contiguous()


def compose(ids, sc, mapped, B, V, C, K, thr, mode, agnostic, sigma=0.5):
    """The hand composition: per-view dense tensors -> cat over the views -> ``ops.filter_dense_nms``."""
    A = sc.shape[1]
    return ops.filter_dense_nms(ids.reshape(B, V * A), sc.reshape(B, V * A), mapped.reshape(B, V * A, 4), C, K, NMS, thr,
                                nms_mode=mode, nms_sigma=sigma, nms_agnostic=agnostic)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, F)).view(np.uint32)


def _assert_same(got, want, tag):
    gc, gl, gs, gb, gi = got
    wc, wl, ws, wb, wi = want
    assert np.array_equal(gc, wc), (tag, gc, wc)
    for b in range(len(gc)):
        n = int(gc[b])
        assert np.array_equal(gl[b, :n], wl[b, :n]), (tag, b, 'class')
        assert np.array_equal(gi[b, :n], wi[b, :n]), (tag, b, 'index')
        assert np.array_equal(_bits(gs[b, :n]), _bits(ws[b, :n])), (tag, b, 'score bits')
        assert np.array_equal(_bits(gb[b, :n]), _bits(wb[b, :n])), (tag, b, 'box bits')


@pytest.mark.parametrize('C', [3, 20])
@pytest.mark.parametrize('A', [37, 216, 1501])
@pytest.mark.parametrize('V', [1, 3])
def test_device_rule_equals_the_dense_composition(V, A, C):
    """Count, class, score bits, box bits and pooled index against the composition of launches that existed before this one, and
    against tests/views_ref.py on the host, for every K and every suppression rule.  A = 37 puts pad words inside the pooled row,
    1501 x 3 is more than 1024 quads (a thread sweeps more than one).  Every case must emit a row; every case with more than one
    candidate slot (K > 1: at K = 1 there is one candidate and nothing to suppress) must suppress or decay one."""
    B = 2
    pred_h, anchors_h, xf_h = make_inputs(100 + 7 * A + V + C, B, V, A, C)
    pred, anchors, xf = (torch.from_numpy(t).cuda() for t in (pred_h, anchors_h, xf_h))
    ids, sc, bx = decode_fn(C)(pred, anchors, SIZE, C)
    mapped = map_on_device(bx, xf)
    ids_h, sc_h, bx_h, mapped_h = _np((ids, sc, bx, mapped))
    pooled = []
    for b in range(B):
        c, s, m = views_ref.pool(ids_h[b * V:(b + 1) * V], sc_h[b * V:(b + 1) * V], bx_h[b * V:(b + 1) * V], xf_h[b * V:(b + 1) * V])
        assert np.array_equal(_bits(m), _bits(mapped_h[b * V:(b + 1) * V].reshape(-1, 4)))        # torch's mapping is the stated one
        pooled.append((c, s, m))
    M = [int((s > F(THR)).sum()) for _, s, _ in pooled]
    print(f'V={V} A={A} C={C}: above-threshold candidates per image {M}')
    if V >= 3:
        n = max(1, A // 3)
        for b in range(B):                                                     # the ties across views happened
            tied = (sc_h[b * V, :n] > F(THR))
            assert tied.sum() >= 2 and np.array_equal(_bits(sc_h[b * V, :n]), _bits(sc_h[b * V + 2, :n]))
    rel = set()
    for K in KS:
        rel |= {'above' if m > K else 'below' if m < K else 'equal' for m in M}
        if A == 1501 and K == 1024:                                            # a class with more than 64 candidates
            for c, s, _ in pooled:
                cand = nms_ref.candidates(s, K, THR)
                assert np.bincount(c[cand], minlength=C).max() > 64
        for mode, agnostic in RULES:
            tag = (V, A, C, K, mode, agnostic)
            got = _np(ops.detect_views(pred, anchors, SIZE, C, V, xf, K, NMS, THR, nms_mode=mode, nms_agnostic=agnostic))
            want = _np(compose(ids, sc, mapped, B, V, C, K, THR, mode, agnostic))
            _assert_same(got, want, tag)
            for b in range(B):
                c, s, m = pooled[b]
                n = int(got[0][b])
                rows = {'class_ids': got[1][b, :n], 'scores': got[2][b, :n], 'boxes': got[3][b, :n], 'anchor_idx': got[4][b, :n]}
                assert nms_ref.verify_replay(rows, c, s, m, K, NMS, THR, C, mode, 0.5, agnostic) == n
                ref = views_ref.pooled_filter(ids_h[b * V:(b + 1) * V], sc_h[b * V:(b + 1) * V], bx_h[b * V:(b + 1) * V],
                                              xf_h[b * V:(b + 1) * V], K, NMS, THR, C, mode, 0.5, agnostic)
                assert n >= 1 and len(ref['scores']) >= 1, tag
                if K > 1:
                    assert (ref['lost'] if mode == 'hard' else ref['total_decays']) >= 1, tag
                if mode != 'gaussian':                                         # (Gaussian: expf vs numpy's exp, held by verify_replay)
                    assert np.array_equal(rows['anchor_idx'], ref['anchor_idx']) and np.array_equal(rows['class_ids'], ref['class_ids']), tag
                    assert np.array_equal(_bits(rows['scores']), _bits(ref['scores'])), tag
                    assert np.array_equal(_bits(rows['boxes']), _bits(ref['boxes'])), tag
                if V >= 3 and b == 0 and mode == 'hard' and K == 1024 and A < 1501:
                    # image 0: views 0 and 2 hold the same boxes with the same scores -- the lower view wins every tie and suppresses its twin
                    twins = rows['anchor_idx'][(rows['anchor_idx'] // A == 2) & (rows['anchor_idx'] % A < max(1, A // 3))]
                    assert twins.size == 0, (tag, twins)
    # the pool is larger than K and smaller than K within every shape, except that 1501 anchors always leave more than 1024
    assert 'above' in rel and (A == 1501 or 'below' in rel), (rel, M)
    if A == 1501:
        assert min(M) > 1024


@pytest.mark.parametrize('C', [3, 20])
@pytest.mark.parametrize('mode', ['hard', 'gaussian'])
def test_one_identity_view_equals_detect_nms(mode, C):
    B, A = 2, 216
    pred_h, anchors_h, _ = make_inputs(5, B, 1, A, C)
    pred, anchors = torch.from_numpy(pred_h).cuda(), torch.from_numpy(anchors_h).cuda()
    xf = torch.from_numpy(np.tile(views_ref.IDENTITY, (B, 1))).cuda()
    for K in (64, 100):
        got = _np(ops.detect_views(pred, anchors, SIZE, C, 1, xf, K, NMS, THR, nms_mode=mode))
        want = _np(ops.detect_nms(pred, anchors, SIZE, C, K, NMS, THR, nms_mode=mode))
        assert got[0].min() >= 1
        _assert_same(got, want, (mode, C, K))


def test_detect_views_checks_its_arguments():
    pred, anchors = torch.zeros(6, 8, 8, device='cuda'), torch.zeros(8, 4, device='cuda')
    xf = torch.zeros(6, 6, device='cuda')
    for bad in (dict(V=4), dict(V=0), dict(view_xf=xf[:5]), dict(view_xf=xf.double()), dict(view_xf=xf.cpu()), dict(keep_top_k=1025),
                dict(score_thresh=-1.0), dict(nms_mode='soft'), dict(out=ops._det_buffers(3, 64, pred.device))):
        kw = dict(V=3, view_xf=xf, keep_top_k=64, nms_thresh=NMS, score_thresh=THR)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.detect_views(pred, anchors, (64, 64), 3, **kw)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
SMALL = (64, 96)
MEAN, STD = np.array([93.877, 98.801, 95.923], F), np.array([78.782, 80.130, 81.200], F)


def _scene_images(sizes, seed):
    rs = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        base = rs.standard_normal((-(-h // 8), -(-w // 8), 3)) * 60 + 100
        out.append(np.clip(np.kron(base, np.ones((8, 8, 1))), 0, 255).astype(np.uint8)[:h, :w])
    return out


def _detector(letterbox):
    """A seeded random-weight detector at 64 x 96 whose threshold is lowered until the plain path returns rows."""
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    cfg = sqd.make_cfg(input_size=SMALL, letterbox=letterbox)
    m = SqueezeDet(cfg)
    m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    det = Detector(m, cfg)
    probe = _scene_images([(80, 120), (64, 96)], 9)
    for thr in (0.3, 0.1, 0.05, 0.02, 0.01, 0.003, 0.001):
        cfg.score_thresh = thr
        if all('boxes' in r for r in det.detect_images(probe)):
            break
    assert all('boxes' in r for r in det.detect_images(probe)), 'the plain detector returns no rows at any threshold tried'
    return det, cfg


@pytest.fixture(scope='module', params=[False, True], ids=['stretch', 'letterbox'])
def small(request):
    return _detector(request.param) + (request.param,)


def _window_canvases(images, wins):
    """``augment.launch`` (letterbox entry, host-given windows inside the canvas) of ``images``: [n, 3, H, W] on the device."""
    sizes = [im.shape[:2] for im in images]
    hdr, offsets, total = augment.pack_layout(sizes, False, True)
    buf = torch.zeros(total, dtype=torch.uint8).pin_memory()
    pk = buf.numpy()
    augment.write_header(pk, offsets, sizes, np.zeros((len(images), 3), np.int32), None, np.asarray(wins, np.int32))
    for im, off in zip(images, offsets):
        pk[hdr + off:hdr + off + im.size] = np.ascontiguousarray(im).reshape(-1)
    out = torch.full((len(images), 3) + SMALL, float('nan'), device='cuda')
    augment.launch(buf.cuda(), len(images), hdr, SMALL, out, False, MEAN, STD, letterbox=True, window=True)
    return out


def _compose_results(det, cfg, canvases, xf_h, n, V):
    """``model.base`` on the reference canvases, pooled through the dense composition -> the five arrays."""
    C, K, A = cfg.num_classes, cfg.keep_top_k, cfg.num_anchors
    with torch.no_grad():
        pred = det.model.base(canvases)
    anchors = det.model.resolver.anchors_on(pred.device)
    ids, sc, bx = ops.decode(pred, anchors, cfg.input_size, C)
    mapped = map_on_device(bx, torch.from_numpy(xf_h).cuda())
    return _np(compose(ids, sc, mapped, n, V, C, K, cfg.score_thresh, 'hard', False)), bx.cpu().numpy()


def _assert_results(res, want, A):
    cnt, cls, sc, bx, idx = want
    total = 0
    for b, r in enumerate(res):
        k = int(cnt[b])
        assert ('boxes' in r) == (k > 0)
        if k:
            assert np.array_equal(r['class_ids'], cls[b, :k]) and np.array_equal(_bits(r['scores']), _bits(sc[b, :k]))
            assert np.array_equal(_bits(r['boxes']), _bits(bx[b, :k]))
            assert np.array_equal(r['view_idx'], idx[b, :k] // A) and np.array_equal(r['anchor_idx'], idx[b, :k] % A)
            assert r['anchor_idx'].max() < A
            total += k
    return total


def test_tta_end_to_end(small):
    """Three images of different sizes, the image, its mirror image and a 0.75 zoom of both: the canvases of the ONE mosaic launch are,
    bit for bit, those of the letterbox launch for the image / the host-mirrored image and the same windows (and view 0 is
    ``preprocess_batch``'s canvas); the results are those of ``model.base`` on these canvases pooled through the dense composition."""
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    det, cfg, letterbox = small
    images = _scene_images([(80, 120), (50, 131), (97, 64)], 4)
    vlist = views.tta_views(flip=True, zooms=(1.0, 0.75))
    V, n = len(vlist), len(images)
    plan = views.plan_views([im.shape[:2] for im in images], vlist, SMALL, letterbox=letterbox)
    canv, xf = views.render_views(images, plan, SMALL, 'cuda', MEAN, STD,
                                  out=torch.full((n * V, 3) + SMALL, float('nan'), device='cuda'))
    assert np.array_equal(xf.cpu().numpy(), plan.view_xf)
    host = [np.ascontiguousarray(np.flip(images[b], 1)) if vlist[v].flip else images[b] for b in range(n) for v in range(V)]
    ref = _window_canvases(host, plan.windows)
    assert not torch.isnan(canv).any() and torch.equal(canv.view(torch.int32), ref.view(torch.int32))
    plain = preprocess_batch(images, SMALL, letterbox=letterbox)[0]
    assert torch.equal(canv[0::V].view(torch.int32), plain.view(torch.int32))                 # view 0 is the plain input
    res = det.detect_images(images, views=vlist)
    want, _ = _compose_results(det, cfg, ref, plan.view_xf, n, V)
    assert _assert_results(res, want, cfg.num_anchors) >= n
    for r, b in zip(res, range(n)):
        assert np.array_equal(r['image_meta']['view_windows'], plan.windows[b * V:(b + 1) * V])
    # the cfg switches are the default views
    cfg.tta_flip, cfg.tta_zooms = True, (1.0, 0.75)
    try:
        again = det.detect_images(images)
    finally:
        cfg.tta_flip, cfg.tta_zooms = False, None
    assert _assert_results(again, want, cfg.num_anchors) >= n


def test_tiles_end_to_end(small):
    """One 200 x 300 frame in 64 x 96 tiles (native resolution): every canvas is ``preprocess_batch``'s of that crop, the results are
    the dense composition's, and a detection wholly inside its tile lies within 1e-3 px of its canvas box moved by the tile's corner.
    A second frame of another size in the same call has another tile count and runs as a pass of its own."""
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    det, cfg, letterbox = small
    frame, other = _scene_images([(200, 300), (100, 150)], 6)
    vlist = views.tile_views((200, 300), SMALL, 16)
    V = len(vlist)
    assert V == 16 and all(v.rect[2:] == SMALL for v in vlist)
    plan = views.plan_views([(200, 300)], vlist, SMALL, letterbox=letterbox)
    canv, _ = views.render_views([frame], plan, SMALL, 'cuda', MEAN, STD, out=torch.full((V, 3) + SMALL, float('nan'), device='cuda'))
    crops = [np.ascontiguousarray(frame[v.rect[0]:v.rect[0] + 64, v.rect[1]:v.rect[1] + 96]) for v in vlist]
    ref = preprocess_batch(crops, SMALL, letterbox=letterbox)[0]
    assert torch.equal(canv.view(torch.int32), ref.view(torch.int32))
    vother = views.tile_views((100, 150), SMALL, 16)
    assert len(vother) != V
    res = det.detect_images([frame, other], views=[vlist, vother])
    want, canvas_boxes = _compose_results(det, cfg, ref, plan.view_xf, 1, V)
    assert _assert_results(res[:1], want, cfg.num_anchors) >= 1
    assert res[1]['image_meta']['view_windows'].shape == (len(vother), 4) and res[1]['image_meta']['index'] == 1
    alone = det.detect_images([other], views=vother)[0]
    assert ('boxes' in alone) == ('boxes' in res[1]) and ('boxes' not in alone or np.array_equal(_bits(alone['boxes']), _bits(res[1]['boxes'])))
    r, inside = res[0], 0
    for box, v, a in zip(r['boxes'], r['view_idx'], r['anchor_idx']):
        ry, rx, rh, rw = vlist[int(v)].rect
        if box[0] >= rx and box[1] >= ry and box[2] <= rx + rw - 1 and box[3] <= ry + rh - 1:
            inside += 1
            moved = canvas_boxes[int(v), int(a)].astype(np.float64) + np.array([rx, ry, rx, ry], np.float64)
            assert np.abs(box.astype(np.float64) - moved).max() <= 1e-3
    assert inside >= 1


def test_defaults_untouched(small):
    """Without views on a cfg without the TTA fields set, ``detect_images`` is ``detect_device`` composed by hand, as before."""
    from squeezedet_pytorch_amd.preprocess import preprocess_batch
    det, cfg, letterbox = small
    assert cfg.tta_flip is False and cfg.tta_zooms is None
    images = _scene_images([(80, 120), (50, 131), (97, 64)], 4)
    res = det.detect_images(images)
    x, aux, _meta = preprocess_batch(images, SMALL, letterbox=letterbox)
    dets = det.detect_device(x, scales=aux[0], shifts=aux[1]) if letterbox else det.detect_device(x, scales=aux)
    cnt, cls, sc, bx, idx = _np(dets)
    assert cnt.sum() >= 1
    for b, r in enumerate(res):
        k = int(cnt[b])
        assert ('boxes' in r) == (k > 0) and 'view_idx' not in r and 'view_windows' not in r['image_meta']
        if k:
            assert np.array_equal(r['class_ids'], cls[b, :k]) and np.array_equal(_bits(r['scores']), _bits(sc[b, :k]))
            assert np.array_equal(_bits(r['boxes']), _bits(bx[b, :k])) and np.array_equal(r['anchor_idx'], idx[b, :k])
