"""GPU tier: Soft-NMS (linear / Gaussian) and class-agnostic NMS in the fused detect launches (csrc/detect_wide.hip
``detect_nms_select_kernel``; ``ops.detect_nms`` / ``ops.filter_dense_nms``; ``cfg.nms_mode`` / ``nms_sigma`` / ``nms_agnostic``).

What each mode is held to: 'hard' and 'linear' equal ``nms_ref.soft_filter`` bit for bit (count, class, anchor, score bits, boxes);
'gaussian' passes ``nms_ref.verify_replay`` (the device's ``expf`` may differ from numpy's ``exp`` in the last bit, so near-ties may
be picked in either order: the device's own order is replayed and every step of the rule is checked).  The generator's cases are
first checked for what makes them worth running -- decays in every image, soft-kept counts that differ from hard-kept, candidates
lost to the threshold after decay -- so none of them passes vacuously.  Shapes are small; they sit on the paths' edges: one
candidate, a group of 63 / 64 / 65 (one wave in registers against a wave striding over LDS, or against the whole workgroup in
agnostic mode), many groups, the many-class decode, the longest single group (1024)."""
import functools

import numpy as np
import pytest
import torch

import nms_ref as ref
from squeezedet_pytorch_amd import ops

pytestmark = pytest.mark.gpu

NMS, THR, SIGMA = 0.4, 0.3, 0.5
RULES = [(m, a) for m in ref.MODES for a in (False, True)]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(seed, B, A, C, quant=None, one_class=None):
    return ref.make_case(seed, B, A, C, quant, one_class)


@functools.lru_cache(maxsize=None)
def _reference(key, K, C, mode, agnostic, nms=NMS, thr=THR, sigma=SIGMA):
    cls, sc, bx = _case(*key)
    return [ref.soft_filter(cls[b], sc[b], bx[b], K, nms, thr, C, mode, sigma, agnostic) for b in range(cls.shape[0])]


def _device(cls, sc, bx, C, K, mode, agnostic, nms=NMS, thr=THR, sigma=SIGMA):
    got = ops.filter_dense_nms(torch.from_numpy(cls).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(bx).cuda(), C, K, nms, thr,
                               nms_mode=mode, nms_sigma=sigma, nms_agnostic=agnostic)
    return tuple(t.cpu().numpy() for t in got)


def _rows(got, b):
    n = int(got[0][b])
    return {'class_ids': got[1][b, :n], 'scores': got[2][b, :n], 'boxes': got[3][b, :n], 'anchor_idx': got[4][b, :n].astype(np.int64)}


def _hold(got, key, K, C, mode, agnostic, nms=NMS, thr=THR, sigma=SIGMA):
    """the device rows of every image against the reference (bitwise) or, in Gaussian mode, the replay"""
    cls, sc, bx = _case(*key)
    want = _reference(key, K, C, mode, agnostic, nms, thr, sigma)
    for b in range(cls.shape[0]):
        r, w = _rows(got, b), want[b]
        case = (key, K, mode, agnostic, b)
        assert 0 <= int(got[0][b]) <= K, case
        if mode == 'gaussian':
            # (no comparison with the reference's rows: a near-tie picked the other way round changes every later decay)
            assert ref.verify_replay(r, cls[b], sc[b], bx[b], K, nms, thr, C, mode, sigma, agnostic) == len(r['scores']), case
            assert (len(r['scores']) > 0) == (len(w['scores']) > 0), case
        else:
            assert len(r['scores']) == len(w['scores']), (case, len(r['scores']), len(w['scores']))
            assert np.array_equal(r['anchor_idx'], w['anchor_idx']), case
            assert np.array_equal(r['class_ids'], w['class_ids']), case
            assert np.array_equal(_bits(r['scores']), _bits(w['scores'])), case
            assert np.array_equal(_bits(r['boxes']), _bits(w['boxes'])), case


def _worth_running(key, K, C, mode, agnostic):
    """decays in every image, soft-kept != hard-kept, candidates lost after decay (suppressed, in hard mode)"""
    want = _reference(key, K, C, mode, agnostic)
    hard = _reference(key, K, C, 'hard', agnostic)
    for w, h in zip(want, hard):
        assert w['lost'] > 0, (key, mode, agnostic)
        if mode != 'hard':
            assert w['total_decays'] >= 30, (key, mode, agnostic, w['total_decays'])
            assert abs(len(w['scores']) - len(h['scores'])) >= 3, (key, mode, agnostic)


@pytest.mark.parametrize('mode,agnostic', RULES)
def test_dense_filter_every_rule(mode, agnostic):
    key, K, C = (0, 3, 300, 3), 64, 3
    _worth_running(key, K, C, mode, agnostic)
    _hold(_device(*_case(*key), C, K, mode, agnostic), key, K, C, mode, agnostic)


@pytest.mark.parametrize('K', (1, 63, 64, 65))
def test_lane_and_word_boundaries(K):
    """A = 300 with one class: the group IS the candidate list -- 63, 64 (one wave, registers), 65 (class-wise: one wave striding
    over LDS; agnostic: the whole workgroup) -- and with three classes."""
    for C, seed in ((1, 1), (3, 0)):
        key = (seed, 3, 300, C)
        for mode, agnostic in RULES:
            if K >= 63:
                _worth_running(key, K, C, mode, agnostic)
            got = _device(*_case(*key), C, K, mode, agnostic)
            _hold(got, key, K, C, mode, agnostic)
            if K == 1:
                assert got[0].tolist() == [1, 1, 1]


@pytest.mark.parametrize('mode,agnostic', RULES)
def test_twenty_classes_keep_200(mode, agnostic):
    key, K, C = (2, 2, 2000, 20), 200, 20
    _worth_running(key, K, C, mode, agnostic)
    _hold(_device(*_case(*key), C, K, mode, agnostic), key, K, C, mode, agnostic)


@pytest.mark.parametrize('mode,agnostic', RULES)
def test_eighty_classes_on_the_many_class_form(mode, agnostic):
    key, K, C = (3, 2, 2000, 80), 128, 80
    assert ops.head_path(C) == 'many'
    want = _reference(key, K, C, mode, agnostic)
    assert all(w['lost'] > 0 for w in want) or not agnostic                 # (class-wise, 128 candidates over 80 classes rarely overlap)
    _hold(_device(*_case(*key), C, K, mode, agnostic), key, K, C, mode, agnostic)


@pytest.mark.parametrize('mode,agnostic', [('gaussian', True), ('linear', True), ('hard', True), ('linear', False), ('gaussian', False)])
def test_the_longest_single_group(mode, agnostic):
    """(A = 4096, K = 1024, C = 1): 1024 candidates in one group -- agnostic on the whole workgroup, class-wise on one wave with 16
    slots per lane."""
    key, K, C = (4, 1, 4096, 1), 1024, 1
    _worth_running(key, K, C, mode, agnostic)
    got = _device(*_case(*key), C, K, mode, agnostic)
    _hold(got, key, K, C, mode, agnostic)
    assert int(got[0][0]) > 32


def test_no_candidate_one_class_and_exact_ties():
    # one image with no candidate (every score at or below the threshold) between two ordinary ones
    cls, sc, bx = (x.copy() for x in _case(0, 3, 300, 3))
    sc[1] = np.minimum(sc[1], np.float32(THR))
    for mode, agnostic in RULES:
        got = _device(cls, sc, bx, 3, 64, mode, agnostic)
        assert int(got[0][1]) == 0 and int(got[0][0]) > 0 and int(got[0][2]) > 0
        for b in (0, 2):
            w = ref.soft_filter(cls[b], sc[b], bx[b], 64, NMS, THR, 3, mode, SIGMA, agnostic)
            r = _rows(got, b)
            if mode == 'gaussian':
                ref.verify_replay(r, cls[b], sc[b], bx[b], 64, NMS, THR, 3, mode, SIGMA, agnostic)
            else:
                assert np.array_equal(r['anchor_idx'], w['anchor_idx']) and np.array_equal(_bits(r['scores']), _bits(w['scores']))
    # every candidate of an image in one class (class 2 of 3: two empty groups before it); scores on a grid of 1/32: many exact ties
    for key, K, C in (((5, 2, 300, 3, None, 2), 64, 3), ((6, 3, 300, 3, 32), 64, 3), ((6, 3, 300, 3, 32), 200, 3)):
        sc_ = _case(*key)[1]
        if key[4]:
            assert len(np.unique(sc_[0])) <= 32
        for mode, agnostic in RULES:
            _hold(_device(*_case(*key), C, K, mode, agnostic), key, K, C, mode, agnostic)


def test_hard_classwise_equals_the_existing_filters():
    for key, K, C, old in (((0, 3, 300, 3), 64, 3, ops.filter_dense), ((0, 3, 300, 3), 64, 3, ops.filter_dense_wide),
                           ((2, 2, 2000, 20), 200, 20, ops.filter_dense_many), ((1, 3, 300, 1), 65, 1, ops.filter_dense_wide)):
        cls, sc, bx = (torch.from_numpy(x).cuda() for x in _case(*key))
        want = tuple(t.cpu().numpy() for t in old(cls, sc, bx, C, K, NMS, THR))
        got = tuple(t.cpu().numpy() for t in ops.filter_dense_nms(cls, sc, bx, C, K, NMS, THR, nms_mode='hard', nms_agnostic=False))
        assert np.array_equal(got[0], want[0]) and int(want[0].sum()) > 0
        for b in range(len(want[0])):
            n = int(want[0][b])
            for g, w in zip(got[1:], want[1:]):
                assert g[b, :n].tobytes() == w[b, :n].tobytes(), (key, K, old.__name__, b)


def _pred_case(C, seed):
    import squeezedet_pytorch_amd as sqd
    cfg = sqd.make_cfg(input_size=(64, 96), num_classes=C)
    rs = np.random.RandomState(seed)
    B, A = 3, cfg.num_anchors
    pred = rs.standard_normal((B, A, C + 5)).astype(np.float32)
    pred[..., :C] *= 3.0                                       # peaked class scores
    pred[..., C] += 1.0                                        # most confidences above one half
    pred[..., C + 1:] *= 0.3                                   # boxes near their anchors: the nine of a cell overlap
    scales = (1.0 + rs.uniform(0.1, 0.9, (B, 2))).astype(np.float32)
    shifts = rs.randint(-9, 10, (B, 2)).astype(np.float32)
    return cfg, torch.from_numpy(pred).cuda(), torch.from_numpy(scales).cuda(), torch.from_numpy(shifts).cuda()


@pytest.mark.parametrize('C', (3, 20))
def test_from_pred_equals_the_dense_filter_on_the_decode(C):
    cfg, pred, scales, shifts = _pred_case(C, 11 + C)
    anchors = torch.from_numpy(cfg.anchors.astype(np.float32)).cuda()
    decode = ops.decode if C <= 16 else ops.decode_many
    ids, sc, bx = decode(pred, anchors, cfg.input_size, C)
    thr = 0.3 if C == 3 else 0.15
    for K in (64, 100):
        for mode, agnostic in (('linear', False), ('hard', True), ('gaussian', True)):
            want = tuple(t.cpu().numpy() for t in ops.filter_dense_nms(ids, sc, bx, C, K, NMS, thr, nms_mode=mode, nms_agnostic=agnostic))
            got = tuple(t.cpu().numpy() for t in ops.detect_nms(pred, anchors, cfg.input_size, C, K, NMS, thr, scales=scales,
                                                                 shifts=shifts, nms_mode=mode, nms_agnostic=agnostic))
            plain = tuple(t.cpu().numpy() for t in ops.filter_dense_nms(ids, sc, bx, C, K, NMS, thr))
            assert np.array_equal(got[0], want[0]) and int(want[0].min()) > 3, (C, K, mode, want[0])
            assert not np.array_equal(want[0], plain[0]) or any(want[4][b, :want[0][b]].tobytes() != plain[4][b, :plain[0][b]].tobytes()
                                                                 for b in range(3)), 'the rule changed nothing: the case is vacuous'
            s_h, t_h = scales.cpu().numpy(), shifts.cpu().numpy()
            for b in range(3):
                n = int(want[0][b])
                for g, w in zip((got[1], got[2], got[4]), (want[1], want[2], want[4])):
                    assert g[b, :n].tobytes() == w[b, :n].tobytes(), (C, K, mode, agnostic, b)
                wb = want[3][b, :n]
                sy, sx, dy, dx = s_h[b, 0], s_h[b, 1], t_h[b, 0], t_h[b, 1]
                exp = np.stack([wb[:, 0] / sx + dx, wb[:, 1] / sy + dy, wb[:, 2] / sx + dx, wb[:, 3] / sy + dy], 1).astype(np.float32)
                assert np.array_equal(_bits(got[3][b, :n]), _bits(exp)), (C, K, mode, agnostic, b)


@pytest.mark.parametrize('A', (5, 6, 7))
def test_keys_ready_reads_arbitrary_pad_words_as_zero(A):
    """With ``keys_ready`` the words A .. ceil4(A)-1 of an image's key row hold whatever ConvDet's launch left there, and the select
    reads them as 0 (3, 2 and 1 pad words here; every Detector-driven case has A divisible by 4).  The scoring launch of a first call
    fills the workspace, the pad words are overwritten with the largest finite key, and a ``keys_ready`` call on that workspace must
    give the first call's five tensors bit for bit.  Image 0 has A candidates (the radix select runs at both K), image 1 two (at K = 4
    every candidate is taken).  ``pred`` and ``anchors`` are views of larger tensors: a select that took a pad word would decode a row
    that exists, and fail here by mismatch."""
    B, C, size = 2, 3, (64, 96)
    rs = np.random.RandomState(40 + A)
    store = (0.3 * rs.standard_normal((B + 1, A, C + 5))).astype(np.float32)
    np.put_along_axis(store[..., :C], rs.randint(0, C, (B + 1, A, 1)), 6.0, axis=2)      # one peaked class per anchor
    store[..., C] += 2.0                                                                  # every score above THR ...
    store[1, 2:, C] = -6.0                                                                # ... but two candidates only in image 1
    anc = np.concatenate([rs.uniform(30, 60, (A + 4, 1)), rs.uniform(20, 40, (A + 4, 3))], 1).astype(np.float32)
    pred, anchors = torch.from_numpy(store).cuda()[:B], torch.from_numpy(anc).cuda()[:A]
    A4 = -(-A // 4) * 4
    for K in (1, 4):
        for mode in ref.MODES:
            ws = torch.zeros(ops.det_workspace_words_wide(B, A, K), device='cuda', dtype=torch.int32)
            first = ops.detect_nms(pred, anchors, size, C, K, NMS, THR, out=ops._det_buffers(B, K, pred.device) + (ws,),
                                   nms_mode=mode, nms_sigma=SIGMA)
            keys = ws.view(B, A4)
            assert (keys[:, :A] != 0).sum(1).tolist() == [A, 2] and not bool(keys[:, A:].any()), (A, K, mode)
            assert first[0].tolist()[0] >= 1 and first[0].tolist()[1] >= 1, (A, K, mode)
            keys[:, A:] = 0x7f7fffff
            second = ops.detect_nms(pred, anchors, size, C, K, NMS, THR, out=ops._det_buffers(B, K, pred.device) + (ws,),
                                    nms_mode=mode, nms_sigma=SIGMA, keys_ready=True)
            for i, (f, s) in enumerate(zip(first, second)):
                assert f.cpu().numpy().tobytes() == s.cpu().numpy().tobytes(), (A, K, mode, i)


def _detector(K=64, **kw):
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    size = (64, 96)
    cfg = sqd.make_cfg(input_size=size, device='cuda:0', keep_top_k=K, score_thresh=0.05, batch_size=2, **kw)
    model = SqueezeDet(cfg)
    model.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    return Detector(model, cfg), cfg, synthetic.make_images(2, size, seed=0).cuda()


def _dense_of(det, cfg, x):
    with torch.no_grad():
        pred = det.model.base(x)
    anchors = det.model.resolver.anchors_on(pred.device)
    return ops.decode(pred, anchors, cfg.input_size, cfg.num_classes)


def _same_dets(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    for b in range(len(want[0])):
        n = int(want[0][b])
        for g, w in zip(got[1:], want[1:]):
            assert g[b, :n].tobytes() == w[b, :n].tobytes(), (what, b)


def test_detector_follows_cfg_and_takes_convdet_keys(monkeypatch):
    """``detect_device`` under every rule equals ``filter_dense_nms`` on ``ops.decode`` of the device's own pred; with
    ``fuse_detect_keys`` and ConvDet on the V-shared Winograd kernel (forced, as tests/test_detect_keys_gpu.py does: the measured table
    sends so small a ConvDet elsewhere) the new launch consumes ConvDet's keys and gives the same rows as the scored form."""
    from squeezedet_pytorch_amd import model as model_mod, tiles
    det, cfg, x = _detector()
    ids, sc, bx = _dense_of(det, cfg, x)
    table_cfg = model_mod.conv3x3_cfg
    N = cfg.anchors_per_grid * (cfg.num_classes + 5)
    ready = []
    real = ops.detect_nms

    def spy(*a, **k):
        ready.append(bool(k.get('keys_ready')))
        return real(*a, **k)
    monkeypatch.setattr(ops, 'detect_nms', spy)
    counts = {}
    for force_vs in (False, True):
        if force_vs:
            monkeypatch.setattr(model_mod, 'conv3x3_cfg',
                                lambda C, Nn, npix, use: (True, tiles.WINO_VS_CFG) if Nn == N else table_cfg(C, Nn, npix, use))
            det.model.base.fuse_detect_keys = False
            ids, sc, bx = _dense_of(det, cfg, x)                            # (another ConvDet kernel: pred differs in the last bits)
        for mode, agnostic in RULES[1:]:
            cfg.nms_mode, cfg.nms_agnostic = mode, agnostic
            want = tuple(t.cpu().numpy() for t in ops.filter_dense_nms(ids, sc, bx, cfg.num_classes, cfg.keep_top_k, cfg.nms_thresh,
                                                                        cfg.score_thresh, nms_mode=mode, nms_agnostic=agnostic))
            assert int(want[0].min()) > 0
            counts[(mode, agnostic)] = want[0].tolist()
            for keys in (True, False):
                det.model.base.fuse_detect_keys = keys
                del ready[:]
                got = tuple(t.cpu().numpy() for t in det.detect_device(x))
                assert ready == [keys and force_vs], (mode, agnostic, keys, force_vs, ready)
                _same_dets(got, want, (mode, agnostic, keys, force_vs))
    assert len({tuple(v) for v in counts.values()}) > 1, counts             # the rules do give different answers here
    # the plain rule never reaches the new launch
    cfg.nms_mode, cfg.nms_agnostic = 'hard', False
    del ready[:]
    det.detect_device(x)
    assert ready == []
    # Detector.filter follows cfg as well
    cfg.nms_mode = 'linear'
    one = det.filter({'class_ids': ids[0], 'scores': sc[0], 'boxes': bx[0]})
    w = tuple(t.cpu().numpy() for t in ops.filter_dense_nms(ids[:1], sc[:1], bx[:1], cfg.num_classes, cfg.keep_top_k, cfg.nms_thresh,
                                                            cfg.score_thresh, nms_mode='linear'))
    n = int(w[0][0])
    assert one['scores'].cpu().numpy().tobytes() == w[2][0, :n].tobytes() and one['anchor_idx'].cpu().numpy().tolist() == w[4][0, :n].tolist()


def test_stream_follows_a_changed_mode_and_ap_takes_the_rows():
    """Changing ``cfg.nms_mode`` between two ``detect_stream`` passes on one Detector: the lanes drop their captured steps (the rule
    is in ``_params_signature``) and match ``detect_images`` both times; ``DetectionAP.update`` accepts the packed output."""
    from squeezedet_pytorch_amd import metrics
    from squeezedet_pytorch_amd.annotations import pack_annotations
    det, cfg, x = _detector()
    rs = np.random.RandomState(5)
    images = [np.clip(np.kron(rs.standard_normal((8, 12, 3)) * 60 + 100, np.ones((8, 8, 1))), 0, 255).astype(np.uint8) for _ in range(2)]
    ex = det.stream()
    seen = {}
    for mode, agnostic in (('hard', False), ('gaussian', False), ('hard', True), ('hard', False)):
        cfg.nms_mode, cfg.nms_agnostic = mode, agnostic
        want = det.detect_images(images)
        got = list(det.detect_stream([images] * 5))                         # 2 lanes: eager, eager, capture, capture, replay
        assert len(got) == 5 and not ex.degraded
        for res in got:
            for r, w in zip(res, want):
                assert ('boxes' in r) == ('boxes' in w)
                for k in ('anchor_idx', 'boxes', 'scores', 'class_ids'):
                    assert np.array_equal(r[k], w[k]) and r[k].dtype == w[k].dtype, (mode, agnostic, k)
        key = tuple(np.concatenate([w['scores'] for w in want]).tobytes() for _ in (0,))
        if (mode, agnostic) in seen:
            assert seen[(mode, agnostic)] == key                            # back on the plain rule: the first answer again
        seen[(mode, agnostic)] = key
    assert len(set(seen.values())) == 3, 'the three rules gave the same rows: the case is vacuous'
    assert ex.replayed_batches >= 4
    cfg.nms_mode, cfg.nms_agnostic = 'gaussian', True
    dets = det.detect_device(x)
    gb, gc, go = pack_annotations([np.array([0, 1]), np.array([2])], [np.array([[4, 4, 40, 40], [30, 10, 90, 60]], np.float32),
                                                                        np.array([[10, 10, 60, 50]], np.float32)])
    ap = metrics.DetectionAP.coco(cfg.num_classes)
    ap.update(dets, torch.from_numpy(gb).cuda(), torch.from_numpy(gc).cuda(), torch.from_numpy(go).cuda())
    out = ap.compute()
    assert out['npos'].tolist() == [1, 1, 1] and out['ap'].shape == (3, 10) and np.all(np.isfinite(out['ap']))


def test_misuse_is_refused_before_any_launch():
    cls, sc, bx = (torch.from_numpy(x).cuda() for x in _case(0, 3, 300, 3))
    cfg, pred, scales, shifts = _pred_case(3, 14)
    anchors = torch.from_numpy(cfg.anchors.astype(np.float32)).cuda()
    out = ops._det_buffers(3, 64, 'cuda:0')
    for t in out:
        t.fill_(7)
    bad_out = ops._det_buffers(3, 32, torch.device('cuda:0'))
    for kw in ({'nms_mode': 'soft'}, {'nms_mode': 2}, {'nms_sigma': 0.0}, {'nms_sigma': -0.5}, {'nms_sigma': float('nan')},
               {'nms_mode': 'gaussian', 'nms_sigma': float('inf')}, {'nms_agnostic': 1}, {'out': bad_out}, {'out': out[:4]}):
        with pytest.raises(ValueError):
            ops.filter_dense_nms(cls, sc, bx, 3, 64, NMS, THR, **dict({'out': tuple(t for t in out)}, **kw))
        with pytest.raises(ValueError):
            ops.detect_nms(pred, anchors, cfg.input_size, 3, 64, NMS, THR, **dict({'out': tuple(t for t in out)}, **kw))
    with pytest.raises(ValueError):
        ops.detect_nms(pred, anchors, cfg.input_size, 3, 64, NMS, THR, keys_ready=True)      # no workspace holds the keys
    with pytest.raises(ValueError):
        ops.filter_dense_nms(cls, sc, bx, 3, 1025, NMS, THR, nms_mode='linear')
    with pytest.raises(ValueError):
        ops.filter_dense_nms(cls, sc, bx, 3, 64, NMS, -0.1, nms_mode='linear')
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out)                             # nothing was written
