"""GPU tier of the detection AP (csrc/det_eval.hip through ops.det_match / ops.det_ap / metrics.DetectionAP) against the numpy float64
restatement tests/det_ap_ref.py.  Bars (derived, DESIGN.md "Detection AP on the device"): everything that is an integer (flags,
matched_gt, npos, tp_cum, fp_cum) and every sampled precision (one float64 division of two integers) is exact; ap is exact in the
11- and 101-point modes and within 1e-12 in the area mode (a sum of at most npos <= 4096 non-negative terms with a total <= 1
after the division: any order differs by at most 4095 * 2^-53 = 4.5e-13)."""
import numpy as np
import pytest
import torch

import det_ap_ref as ref
from squeezedet_pytorch_amd import metrics, ops

pytestmark = pytest.mark.gpu

COCO = metrics.COCO_THRESHOLDS
AREA_BAR = 1e-12


def _dev(batch):
    count, cls, sc, bx, gb, gc, go, gi = batch
    det = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (count, cls, sc, bx))
    gt = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (gb, gc, go))
    return det, gt, None if gi is None else torch.from_numpy(gi).cuda()


def _slice(batch, b0, b1):
    count, cls, sc, bx, gb, gc, go, gi = batch
    g0, g1 = int(go[b0]), int(go[b1])
    return (count[b0:b1], cls[b0:b1], sc[b0:b1], bx[b0:b1], gb[g0:g1], gc[g0:g1], (go[b0:b1 + 1] - g0).astype(np.int32),
            None if gi is None else gi[g0:g1])


def _same_ap(a, b):
    return np.array_equal(a, b, equal_nan=True)


def test_hand_built_batch():
    batch, thr, C, flags, matched, npos = ref.hand_batch()
    det, gt, ign = _dev(batch)
    f, m, n = ops.det_match(det, *gt, thr, C, gt_ignore=ign)
    assert f.dtype == torch.uint8 and m.dtype == torch.int32 and n.dtype == torch.int32
    assert np.array_equal(f.cpu().numpy(), flags), f.cpu().numpy().tolist()
    assert np.array_equal(m.cpu().numpy(), matched), m.cpu().numpy().tolist()
    assert np.array_equal(n.cpu().numpy(), npos)
    for mode in ('area', '11point', '101point'):
        met = metrics.DetectionAP(C, thr, mode)
        met.update(det, *gt, gt_ignore=ign)
        got, want = met.compute(), ref.dataset([batch], thr, C, mode)
        assert np.array_equal(got['npos'], want['npos'])
        if mode == 'area':
            assert np.all(np.abs(got['ap'] - want['ap']) <= AREA_BAR) and np.all(np.abs(got['map'] - want['map']) <= AREA_BAR)
        else:
            assert _same_ap(got['ap'], want['ap']) and np.array_equal(got['map'], want['map']) and got['map_all'] == want['map_all']


GT_EDGES = [0, 1, 63, 64, 65, 300]          # the wave and LDS-chunk edges (a chunk holds 256 GT)


@pytest.mark.parametrize('K', [1, 64, 65, 1024])
def test_match_sweep(K):
    """K x C x T x ignore on B = 5 seeded images with equal scores and equal IoUs.  The thresholds are independent, so the T = 1 case
    (0.5 alone) is held to the first column of the T = 10 reference."""
    B = 5
    s_ties = i_ties = 0
    for ci, C in enumerate([1, 3, 20, 256]):
        for with_ignore in (False, True):
            shift = ci * 2 + int(with_ignore) + K
            gt_counts = [GT_EDGES[(b + shift) % 6] for b in range(B)]
            batch = ref.random_batch(1000 * K + 10 * C + int(with_ignore), B, K, C, gt_counts, with_ignore)
            st, it = ref.count_ties(batch, C)
            s_ties, i_ties = s_ties + st, i_ties + it
            det, gt, ign = _dev(batch)
            want_f, want_m, want_n = ref.match(*batch[:7], COCO, C, batch[7])
            for thr, cols in ((COCO, slice(0, 10)), ((0.5,), slice(0, 1))):
                f, m, npos = ops.det_match(det, *gt, thr, C, gt_ignore=ign)
                f2, m2, npos2 = ops.det_match(det, *gt, thr, C, gt_ignore=ign, npos=npos)       # a second call into the same buffer
                f, m, f2, m2 = (t.cpu().numpy() for t in (f, m, f2, m2))
                tag = f'K={K} C={C} T={len(thr)} ignore={with_ignore}'
                bad = np.argwhere(f != want_f[:, :, cols])
                assert bad.size == 0, (tag, 'flags', bad[:4].tolist())
                bad = np.argwhere(m != want_m[:, :, cols])
                assert bad.size == 0, (tag, 'matched_gt', bad[:4].tolist())
                assert np.array_equal(f2, f) and np.array_equal(m2, m), tag
                assert npos2 is npos and np.array_equal(npos.cpu().numpy(), 2 * want_n), tag
    assert i_ties > 0, 'the inputs hold no IoU tie'
    assert K == 1 or s_ties > 0, 'the inputs hold no score tie'


AP_CHUNK = 1024                              # entries per chunk of the AP kernel
SEG_LENGTHS = [0, 1, 63, 64, 65, AP_CHUNK + 1, 5000]


def _ap_case():
    rs = np.random.RandomState(7)
    C, T = 7, 3
    lengths = [SEG_LENGTHS[i] for i in (3, 0, 6, 1, 5, 2, 4)]      # class 1: GT but no detections; class 5 (63 entries): no GT
    cls = np.concatenate([np.full(n, c, np.int32) for c, n in enumerate(lengths)] + [np.full(37, C, np.int32)])
    N = cls.shape[0]
    flags = rs.choice(np.array([0, 1, 2], np.uint8), size=(N, T), p=[0.45, 0.4, 0.15])
    flags[cls == 2, 0] = rs.choice(np.array([0, 1, 2], np.uint8), size=5000, p=[0.15, 0.78, 0.07])   # (about 3 900 true positives)
    flags[cls == 4, 2] = 2                                          # a segment of ignored entries only: every precision is 0
    flags[cls == C] = 3
    seg = ref.segments(cls, C)
    npos = np.array([int((flags[cls == c] == 1).sum(0).max()) + int(rs.randint(0, 5)) for c in range(C)], np.int32)
    npos[1], npos[5] = 9, 0
    assert npos.max() <= 4096 and seg.tolist()[-1] == N - 37
    return cls, flags, seg, npos


@pytest.fixture(scope='module')
def ap_case():
    return _ap_case()


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_ap_sweep(ap_case, mode):
    cls, flags, seg, npos = ap_case
    want_ap, want_tp, want_fp, want_samp = ref.ap(cls, flags, seg, npos, mode)
    ap, tp, fp, prec = ops.det_ap(*(torch.from_numpy(a).cuda() for a in (cls, flags, seg, npos)), mode, want_prec101=True)
    assert np.array_equal(tp.cpu().numpy(), want_tp) and np.array_equal(fp.cpu().numpy(), want_fp)
    ap = ap.cpu().numpy()
    assert np.array_equal(np.isnan(ap), np.isnan(want_ap)) and np.isnan(ap[5]).all() and not np.isnan(ap[[0, 1, 2, 3, 4, 6]]).any()
    assert np.all(ap[1] == 0.0) and np.all(ap[4, 2] == 0.0)
    if mode == 0:
        err = np.nanmax(np.abs(ap - want_ap))
        print(f'area mode: max |ap - ref| = {err:.3e}')
        assert err <= AREA_BAR
        assert prec is None
    else:
        assert _same_ap(ap, want_ap)
    if mode == 2:
        prec = prec.cpu().numpy()
        assert np.isnan(prec[5]).all() and np.array_equal(np.delete(prec, 5, 0), np.delete(want_samp, 5, 0))


@pytest.fixture(scope='module')
def dataset60():
    rs = np.random.RandomState(11)
    C, K, B = 5, 16, 60
    batch = ref.random_batch(60, B, K, C, rs.randint(0, 7, B), True)
    parts = [_slice(batch, 0, 20), _slice(batch, 20, 53), _slice(batch, 53, 60)]
    thr = (0.5, 0.75)
    return C, thr, batch, parts, ref.dataset([batch], thr, C, 'area')


def _run(C, thr, mode, batches, met=None):
    met = met if met is not None else metrics.DetectionAP(C, thr, mode)
    for b in batches:
        det, gt, ign = _dev(b)
        met.update(det, *gt, gt_ignore=ign)
    return met, met.compute()


def test_detection_ap_batching_and_reset(dataset60):
    C, thr, batch, parts, want = dataset60
    met, one = _run(C, thr, 'area', [batch])
    assert np.array_equal(one['npos'], want['npos']) and np.all(np.abs(one['ap'] - want['ap']) <= AREA_BAR)
    assert np.all(np.abs(one['map'] - want['map']) <= AREA_BAR) and abs(one['map_all'] - want['map_all']) <= AREA_BAR
    assert one['thresholds'] == thr and one['ap'].shape == (C, 2) and one['ap'].dtype == np.float64
    _, three = _run(C, thr, 'area', parts)
    assert _same_ap(three['ap'], one['ap']) and np.array_equal(three['npos'], one['npos'])       # bit-identical
    met.reset()
    _, again = _run(C, thr, 'area', parts, met)
    assert _same_ap(again['ap'], one['ap']) and np.array_equal(again['map'], one['map']) and again['map_all'] == one['map_all']


def test_detection_ap_batch_order_without_ties(dataset60):
    C, thr, batch, _, _ = dataset60
    sc = ((np.random.RandomState(5).permutation(batch[2].size) + 1) / np.float32(batch[2].size + 1)).astype(np.float32).reshape(batch[2].shape)
    assert np.unique(sc).size == sc.size                        # the tie-free variant: every score distinct
    free = batch[:2] + (sc,) + batch[3:]
    parts = [_slice(free, 0, 20), _slice(free, 20, 53), _slice(free, 53, 60)]
    _, fwd = _run(C, thr, 'area', parts)
    _, rev = _run(C, thr, 'area', parts[::-1])
    assert _same_ap(fwd['ap'], rev['ap']) and np.array_equal(fwd['npos'], rev['npos'])
    want = ref.dataset(parts[::-1], thr, C, 'area')
    assert np.all(np.abs(rev['ap'] - want['ap']) <= AREA_BAR)


def test_coco_and_voc07_shorthands(dataset60):
    C, _, batch, parts, _ = dataset60
    for make, thr, mode in ((metrics.DetectionAP.coco, COCO, '101point'), (metrics.DetectionAP.voc07, (0.5,), '11point')):
        met = make(C)
        assert met.thresholds == thr and met.mode == mode
        _, got = _run(C, thr, mode, parts, met)
        want = ref.dataset(parts, thr, C, mode)
        assert _same_ap(got['ap'], want['ap']) and np.array_equal(got['map'], want['map']) and got['map_all'] == want['map_all']
        assert np.array_equal(got['npos'], want['npos'])


def test_update_sparse_equals_update(dataset60):
    C, thr, _, parts, _ = dataset60
    plain = tuple(p[:7] + (None,) for p in parts)               # (a SparseGT carries no ignore marks)
    _, want = _run(C, thr, 'area', plain)
    met = metrics.DetectionAP(C, thr, 'area')
    for p in plain:
        det, (gb, gc, go), _ = _dev(p)
        total = gc.shape[0]
        sgt = ops.SparseGT(torch.zeros(total, dtype=torch.int32, device='cuda'), gb, torch.zeros(total, 4, device='cuda'), gc, go)
        met.update_sparse(det, sgt)
    got = met.compute()
    assert _same_ap(got['ap'], want['ap']) and np.array_equal(got['npos'], want['npos'])


def test_update_does_not_synchronise(dataset60):
    C, thr, _, parts, _ = dataset60
    moved = [_dev(p) for p in parts]
    met = metrics.DetectionAP(C, thr, 'area')
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')                     # any host synchronisation or D2H copy raises
    try:
        for det, gt, ign in moved:
            met.update(det, *gt, gt_ignore=ign)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert met.compute()['ap'].shape == (C, 2)


def test_end_to_end_small_model():
    """The small synthetic model at C = 20: the metric from ``detect_device``'s tuple through ``DetectionAP`` and from
    ``detect_images``' host dicts through ``metrics.evaluate_results``, both against the restatement.  The GT is built from the
    model's own detections (shifted copies of some, so that true positives, duplicates and misses all occur) plus unrelated boxes."""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.annotations import pack_annotations
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    C, size, thr = 20, (64, 96), (0.5, 0.75)
    cfg = sqd.make_cfg(input_size=size, num_classes=C, keep_top_k=64, score_thresh=0.1, batch_size=2)
    m = SqueezeDet(cfg)
    m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234, num_classes=C))
    det = Detector(m, cfg)
    rs = np.random.RandomState(3)

    def gt_from(cnt, cls, bx):
        cl, bl = [], []
        for b in range(len(cnt)):
            n = int(cnt[b])
            pick = [k for k in range(0, n, 3) if bx[b][k][2] - bx[b][k][0] > 2 and bx[b][k][3] - bx[b][k][1] > 2][:6]
            boxes = [bx[b][k] + np.array([0.5, 0.25, 0.0, -0.5], np.float32) for k in pick] + [np.array([1, 1, 9, 7], np.float32)]
            cl.append(np.array([cls[b][k] for k in pick] + [int(rs.randint(0, C))], np.int32))
            bl.append(np.stack(boxes).astype(np.float32))
        return cl, bl

    # the device route: two batches through detect_device
    met = metrics.DetectionAP(C, thr, 'area')
    batches = []
    for seed in (5, 6):
        x = synthetic.make_images(2, size, seed=seed).cuda()
        out = det.detect_device(x)
        cnt, cls, sc, bx = (t.cpu().numpy() for t in out[:4])
        cl, bl = gt_from(cnt, cls, bx)
        gb, gc, go = pack_annotations(cl, bl)
        met.update(out, torch.from_numpy(gb).cuda(), torch.from_numpy(gc).cuda(), torch.from_numpy(go).cuda())
        batches.append((cnt, cls, sc, bx, gb, gc, go, None))
    assert sum(int(b[0].sum()) for b in batches) > 8, 'the synthetic model gave too few detections to test anything'
    got, want = met.compute(), ref.dataset(batches, thr, C, 'area')
    assert want['npos'].sum() > 0 and np.nanmax(want['ap']) > 0
    assert np.array_equal(got['npos'], want['npos']) and np.array_equal(np.isnan(got['ap']), np.isnan(want['ap']))
    assert np.nanmax(np.abs(got['ap'] - want['ap'])) <= AREA_BAR and np.all(np.abs(got['map'] - want['map']) <= AREA_BAR)

    # the host route: detect_images' dicts (original-image coordinates) through evaluate_results
    images = [np.ascontiguousarray(rs.randint(0, 256, (80 + 16 * i, 120, 3)).astype(np.uint8)) for i in range(4)]
    results = det.detect_images(images[:2]) + det.detect_images(images[2:])
    cnt = [0 if 'scores' not in r else len(r['scores']) for r in results]
    cl, bl = gt_from(cnt, [r.get('class_ids') for r in results], [r.get('boxes') for r in results])
    for mode in ('area', '101point'):
        got = metrics.evaluate_results(results, cl, bl, C, thr, mode)
        packed = metrics.pack_results(results)
        want = ref.dataset([packed + pack_annotations(cl, bl) + (None,)], thr, C, mode)
        assert np.array_equal(got['npos'], want['npos']) and np.array_equal(np.isnan(got['ap']), np.isnan(want['ap']))
        if mode == 'area':
            assert np.nanmax(np.abs(got['ap'] - want['ap'])) <= AREA_BAR
        else:
            assert _same_ap(got['ap'], want['ap'])
