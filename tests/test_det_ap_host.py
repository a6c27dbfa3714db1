"""CPU tier of the detection AP (csrc/det_eval.hip, metrics.py): the numpy restatement tests/det_ap_ref.py against cases worked out
by hand, proof that those cases notice each rule being broken, the two entry points' argument checks (no launch is made), and the
host-side packing of ``metrics.evaluate_results``."""
import ctypes
import math

import numpy as np
import pytest

import det_ap_ref as ref
from squeezedet_pytorch_amd import metrics  # noqa: F401  (the module under test)


def _one_class(dets, gts, thresholds=(0.5,), ignore=None):
    """One image, one class: dets = [(score, box)], gts = [box] -> batch tuple."""
    K = max(1, len(dets))
    cls = np.zeros((1, K), np.int64)
    sc = np.zeros((1, K), np.float32)
    bx = np.zeros((1, K, 4), np.float32)
    for k, (s, b) in enumerate(dets):
        sc[0, k], bx[0, k] = s, b
    gb = np.asarray(gts, np.float32).reshape(-1, 4)
    return (np.array([len(dets)], np.int32), cls, sc, bx, gb, np.zeros(len(gts), np.int32), np.array([0, len(gts)], np.int32),
            None if ignore is None else np.asarray(ignore, np.uint8))


def _box(i):
    return [10.0 * i, 0.0, 10.0 * i + 4.0, 4.0]


def test_scalar_and_vector_iou_agree_bit_for_bit():
    rs = np.random.RandomState(0)
    A = (rs.randint(0, 200, (40, 4)) / 4.0).astype(np.float32)
    G = (rs.randint(0, 200, (30, 4)) / 4.0).astype(np.float32)
    A[:, 2:] += A[:, :2]
    G[:, 2:] += G[:, :2]
    M = ref.iou_matrix(A, G)
    for i in range(40):
        for j in range(30):
            assert M[i, j] == ref.iou(A[i], G[j])
    assert ref.iou([0, 0, 2, 1], [0, 0, 2, 2]) == 0.5
    assert ref.iou([0, 0, 1, 1], [5, 5, 6, 6]) == 0.0 and ref.iou([0, 0, 0, 0], [0, 0, 0, 0]) == 0.0


def test_classic_three_gt_five_detections():
    """TP FP TP FP TP against 3 GT: precisions 1, 1/2, 2/3, 1/2, 3/5; envelope at the true positives 1, 2/3, 3/5.
    Area AP = (1 + 2/3 + 3/5) / 3 = 34/45.  11-point: recall 1/3 covers r = 0 .. 0.3 (4 points at 1), 2/3 covers 0.4 .. 0.6 (3 points at
    2/3), 1 covers 0.7 .. 1 (4 points at 3/5): (4 + 2 + 12/5) / 11 = 42/55."""
    far = [100.0, 100.0, 104.0, 104.0]
    dets = [(0.9, _box(0)), (0.8, far), (0.7, _box(1)), (0.6, far), (0.5, _box(2))]
    batch = _one_class(dets, [_box(0), _box(1), _box(2)])
    f, m, npos = ref.match(*batch[:7], (0.5,), 1, batch[7])
    assert f[0, :, 0].tolist() == [1, 0, 1, 0, 1] and m[0, :, 0].tolist() == [0, -1, 1, -1, 2] and npos.tolist() == [3]
    area = ref.dataset([batch], (0.5,), 1, 'area')
    assert abs(area['ap'][0, 0] - 34.0 / 45.0) <= 4e-16
    eleven = ref.dataset([batch], (0.5,), 1, '11point')
    assert abs(eleven['ap'][0, 0] - 42.0 / 55.0) <= 4e-16
    o = ref.order(np.zeros(5, np.int64), batch[2].reshape(-1))
    _, tp, fp, samp = ref.ap(np.zeros(5, np.int64), f.reshape(5, 1)[o], [0, 5], [3], 1)
    assert tp[:, 0].tolist() == [1, 1, 2, 2, 3] and fp[:, 0].tolist() == [0, 1, 1, 2, 2]
    assert samp[0, 0, :11].tolist() == [1.0] * 4 + [2.0 / 3.0] * 3 + [3.0 / 5.0] * 4
    coco = ref.dataset([batch], (0.5,), 1, '101point')          # recall 1/3 reaches k <= 33, 2/3 reaches k <= 66
    want = 0.0
    for k in range(101):
        want += 1.0 if k <= 33 else (2.0 / 3.0 if k <= 66 else 3.0 / 5.0)
    assert coco['ap'][0, 0] == want / 101.0


def test_perfect_detections_give_ap_one_at_every_threshold():
    thr = tuple(round(0.5 + 0.05 * i, 2) for i in range(10))
    gts = [_box(i) for i in range(4)]
    batch = _one_class([(0.9 - 0.1 * i, g) for i, g in enumerate(gts)], gts)
    for mode in ('area', '11point', '101point'):
        r = ref.dataset([batch], thr, 1, mode)
        assert np.all(r['ap'] == 1.0) and np.all(r['map'] == 1.0) and r['map_all'] == 1.0


def test_no_detections_for_a_class_with_gt_gives_zero_and_no_gt_gives_nan():
    """Class 0 has GT and detections, class 1 has GT and no detection (AP 0), class 2 has detections and no GT (NaN, left out of map)."""
    count = np.array([2], np.int32)
    cls = np.array([[0, 2]], np.int64)
    sc = np.array([[0.9, 0.8]], np.float32)
    bx = np.array([[_box(0), _box(1)]], np.float32)
    batch = (count, cls, sc, bx, np.array([_box(0), _box(1)], np.float32), np.array([0, 1], np.int32), np.array([0, 2], np.int32), None)
    for mode in ('area', '11point', '101point'):
        r = ref.dataset([batch], (0.5, 0.75), 3, mode)
        assert r['ap'][0].tolist() == [1.0, 1.0] and r['ap'][1].tolist() == [0.0, 0.0]
        assert math.isnan(r['ap'][2, 0]) and math.isnan(r['ap'][2, 1])
        assert r['map'].tolist() == [0.5, 0.5] and r['map_all'] == 0.5 and r['npos'].tolist() == [1, 1, 0]


def test_hand_batch_matches_its_worked_out_labels():
    batch, thr, C, flags, matched, npos = ref.hand_batch()
    f, m, n = ref.match(*batch[:7], thr, C, batch[7])
    assert np.array_equal(f, flags) and np.array_equal(m, matched) and np.array_equal(n, npos)
    assert ref.iou(batch[3][0, 0], batch[4][0]) == 0.5          # the detection that sits exactly on the threshold
    assert ref.iou(batch[3][0, 4], batch[4][2]) == 0.8


@pytest.mark.parametrize('broken', ['strict', 'claim_ignored', 'rematch_claimed', 'tie_high'])
def test_hand_batch_notices_each_broken_rule(broken):
    """'>' instead of '>=', claiming ignored GT, letting a claimed GT match again, ties broken by the higher index."""
    batch, thr, C, flags, matched, _ = ref.hand_batch()
    f, m, _ = ref.match(*batch[:7], thr, C, batch[7], **{broken: True})
    assert not (np.array_equal(f, flags) and np.array_equal(m, matched))
    where = {'strict': (0, 0, 0), 'claim_ignored': (0, 4, 0), 'rematch_claimed': (0, 1, 0), 'tie_high': (0, 5, 0)}[broken]
    assert (f[where], m[where]) != (flags[where], matched[where])


def test_order_and_ties():
    cls = np.array([1, 0, 1, 2, 0, 1], np.int64)
    sc = np.array([0.5, 0.25, 0.75, 0.1, 0.25, 0.5], np.float32)
    assert ref.order(cls, sc).tolist() == [1, 4, 2, 0, 5, 3]
    assert ref.segments(cls[ref.order(cls, sc)], 2).tolist() == [0, 2, 5]


def test_random_batches_hold_both_kinds_of_ties():
    batch = ref.random_batch(3, 5, 64, 3, [0, 1, 63, 64, 65], True)
    s_ties, i_ties = ref.count_ties(batch, 3)
    assert s_ties > 0 and i_ties > 0


# ---- the library's argument checks: before any launch, so they run here ----
def _match_args(**over):
    p = ctypes.c_void_p(4096)
    a = dict(count=p, class_ids=p, scores=p, boxes=p, gt_boxes=p, gt_class_ids=p, gt_offsets=p, gt_ignore=None, thresholds=p, flags=p,
             matched_gt=p, npos=p, B=2, K=8, total=4, T=2, num_classes=3, stream=None)
    a.update(over)
    return list(a.values())


def _ap_args(**over):
    p = ctypes.c_void_p(4096)
    a = dict(class_ids=p, flags=p, seg_offsets=p, npos=p, ap=p, tp_cum=p, fp_cum=p, prec101=None, N=10, T=2, num_classes=3, mode=0,
             stream=None)
    a.update(over)
    return list(a.values())


MATCH_BAD = [dict(count=None), dict(class_ids=None), dict(scores=None), dict(boxes=None), dict(gt_boxes=None), dict(gt_class_ids=None),
             dict(gt_offsets=None), dict(thresholds=None), dict(flags=None), dict(matched_gt=None), dict(npos=None),
             dict(T=0), dict(T=17), dict(num_classes=0), dict(num_classes=257), dict(K=0), dict(K=1025), dict(B=0), dict(B=-1),
             dict(total=-1)]
AP_BAD = [dict(class_ids=None), dict(flags=None), dict(seg_offsets=None), dict(npos=None), dict(ap=None), dict(tp_cum=None),
          dict(fp_cum=None), dict(T=0), dict(T=17), dict(num_classes=0), dict(num_classes=257), dict(N=-1), dict(mode=3), dict(mode=-1)]


@pytest.mark.parametrize('bad', MATCH_BAD, ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_det_match_rejects_bad_arguments_without_gpu(bad):
    from squeezedet_pytorch_amd import _native as nat
    assert nat.lib().sqd_det_match_fwd(*_match_args(**bad)) == 1


@pytest.mark.parametrize('bad', AP_BAD, ids=lambda d: '%s=%s' % next(iter(d.items())))
def test_det_ap_rejects_bad_arguments_without_gpu(bad):
    from squeezedet_pytorch_amd import _native as nat
    assert nat.lib().sqd_det_ap_fwd(*_ap_args(**bad)) == 1


def test_wrappers_name_the_limit():
    import torch
    from squeezedet_pytorch_amd import metrics, ops
    with pytest.raises(ValueError, match='16'):
        metrics.DetectionAP(3, [0.5] * 17)
    with pytest.raises(ValueError, match='256'):
        metrics.DetectionAP(257)
    with pytest.raises(ValueError, match='mode'):
        metrics.DetectionAP(3, mode='voc')
    det = (torch.zeros(2, dtype=torch.int32), torch.zeros(2, 1025, dtype=torch.int64), torch.zeros(2, 1025), torch.zeros(2, 1025, 4))
    gt = (torch.zeros(0, 4), torch.zeros(0, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='1024'):
        ops.det_match(det, *gt, (0.5,), 3)
    det = tuple(t[:, :4].contiguous() if t.dim() > 1 else t for t in det)
    with pytest.raises(ValueError, match='GPU'):
        ops.det_match(det, *gt, (0.5,), 3)
    with pytest.raises(ValueError, match='int32'):
        ops.det_match(det, gt[0], gt[1].long(), gt[2], (0.5,), 3)
    with pytest.raises(ValueError, match='mode'):
        ops.det_ap(torch.zeros(4, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32),
                   torch.zeros(3, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match='16'):
        ops.det_ap(torch.zeros(4, dtype=torch.int32), torch.zeros(4, 17, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32),
                   torch.zeros(3, dtype=torch.int32), 'area')
    assert metrics.DetectionAP.coco(80).thresholds == (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95)
    assert metrics.DetectionAP.coco(80).mode == '101point' and metrics.DetectionAP.voc07(20).mode == '11point'
    import squeezedet_pytorch_amd as sqd
    assert sqd.DetectionAP is metrics.DetectionAP and sqd.evaluate_results is metrics.evaluate_results


def test_pack_results_ragged_counts_and_empty_images():
    from squeezedet_pytorch_amd import metrics
    rs = np.random.RandomState(1)

    def res(n):
        if n == 0:
            return {'image_meta': {}}
        return {'class_ids': rs.randint(0, 20, n).astype(np.int64), 'scores': rs.rand(n).astype(np.float32),
                'boxes': rs.rand(n, 4).astype(np.float32), 'anchor_idx': np.arange(n), 'image_meta': {}}

    results = [res(3), res(0), res(7), res(1)]
    cnt, cls, sc, bx = metrics.pack_results(results)
    assert cnt.dtype == np.int32 and cls.dtype == np.int64 and sc.dtype == np.float32 and bx.dtype == np.float32
    assert cnt.tolist() == [3, 0, 7, 1] and cls.shape == (4, 7) and sc.shape == (4, 7) and bx.shape == (4, 7, 4)      # K = the maximum count
    for b, r in enumerate(results):
        n = cnt[b]
        if n:
            assert np.array_equal(cls[b, :n], r['class_ids']) and np.array_equal(sc[b, :n], r['scores']) and np.array_equal(bx[b, :n], r['boxes'])
        assert not cls[b, n:].any() and not sc[b, n:].any() and not bx[b, n:].any()
    cnt, cls, sc, bx = metrics.pack_results([res(0), res(0)])
    assert cnt.tolist() == [0, 0] and sc.shape == (2, 1)
    with pytest.raises(ValueError, match='1024'):
        metrics.pack_results([res(1025)])
    with pytest.raises(ValueError):
        metrics.pack_results([])


def test_det_eval_kernels_do_not_spill():
    """Both kernels compiled to ISA with the Makefile's flags: no spilled register, no scratch."""
    import os
    import shutil
    from test_build_spills import HIPCC, _spills
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    k = _spills('det_eval.hip', [], scratch=True)
    assert any('det_match_kernel' in n for n in k) and any('det_ap_kernel' in n for n in k), sorted(k)
    assert all(v == (0, 0) for v in k.values()), k
