"""GPU tier of the IoU-threshold matcher (``ops.anchor_match``, csrc/gt_encode.hip): the two launches against the independent numpy
restatement of tests/anchor_match_ref.py on its case list and on the KITTI grid -- indices, class ids, boxes, offsets, bitmap, overflow
and dx, dy bit for bit, dw and dh within 1 ulp (the encoder's own standard, tests/test_gt_encode_sweep_gpu.py) --, into buffers
pre-filled with garbage, twice; the raw entry's status codes; the matcher's long, padded lists through the masked loss at the bars of
tests/test_ignore_gpu.py; ``TrainLoader`` -> ``Trainer`` eager and captured; and the feature switched off."""
import ctypes

import numpy as np
import pytest
import torch

import anchor_match_ref as M
import fp64_ref as R
import gt_encode_ref as G
import ignore_ref as IR
import iou_loss_ref as Q
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import boxes, ops
import test_fp64_loss_gpu as LG
import test_ignore_gpu as TG

pytestmark = pytest.mark.gpu

ALL = M.cases() + [M.kitti_case()]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _ulps(got, want):
    """Distance in float32 steps between two arrays (finite values of one sign or zero)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(got) - key(want))


def _encode(case):
    """The case on the device through the encoder: (the encoder's SparseGT, anchors64, ignore_in bitmap or None)."""
    offs = np.zeros(len(case['boxes']) + 1, np.int32)
    offs[1:] = np.cumsum([b.shape[0] for b in case['boxes']])
    d_boxes = torch.from_numpy(np.concatenate(case['boxes'], 0)).cuda()
    d_cls = torch.from_numpy(np.concatenate(case['cls'], 0)).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    a64 = torch.from_numpy(case['anchors']).cuda()
    _, idx, deltas = ops.encode_gt(d_boxes, d_cls, d_offs, a64, case['C'], dense=False)
    ign = None if case['ignore_in'] is None else torch.from_numpy(boxes.pack_ignore_bits(case['ignore_in'])).cuda()
    return ops.SparseGT(idx, d_boxes, deltas, d_cls, d_offs), a64, ign


def _garbage(case):
    """Output buffers of the right shapes filled with values no output can hold."""
    B, A = len(case['boxes']), case['anchors'].shape[0]
    T = sum(b.shape[0] for b in case['boxes']) + B * case['max_extra']
    i32 = lambda *s: torch.full(s, -0x5a5a5a5b, dtype=torch.int32, device='cuda')          # noqa: E731
    f32 = lambda *s: torch.full(s, float('nan'), device='cuda')                            # noqa: E731
    return ops.SparseGT(i32(T), f32(T, 4), f32(T, 4), i32(T), i32(B + 1)), i32(B, ops.ignore_words(A)), i32(B)


def _match(case, out=None):
    sgt, a64, ign = _encode(case)
    got = ops.anchor_match(sgt, a64, case['pos_iou'], case['ign_iou'], case['max_extra'], ignore=ign, out=out)
    torch.cuda.synchronize()
    return sgt, got


@pytest.mark.parametrize('case', ALL, ids=lambda c: c['name'])
def test_matcher_equals_the_restatement(case):
    ref = M.reference(case)
    A, B = case['anchors'].shape[0], len(case['boxes'])
    enc, (sgt, ign, overflow) = _match(case, out=_garbage(case))
    # the encoder's own picks are the restatement's (what the primaries of both sides rest on)
    prim_idx, _ = M.primaries(case)
    assert np.array_equal(enc.anchor_idx.cpu().numpy(), np.concatenate(prim_idx).astype(np.int32))
    all_boxes, all_cls = np.concatenate(case['boxes'], 0), np.concatenate(case['cls'], 0)
    pad = ref['box_idx'] < 0
    want_boxes = np.where(pad[:, None], np.float32(0), all_boxes[np.maximum(ref['box_idx'], 0)])
    want_cls = np.where(pad, 0, all_cls[np.maximum(ref['box_idx'], 0)]).astype(np.int32)
    assert np.array_equal(sgt.anchor_idx.cpu().numpy(), ref['anchor_idx'])
    assert np.array_equal(sgt.offsets.cpu().numpy(), ref['offsets'])
    assert np.array_equal(sgt.class_ids.cpu().numpy(), want_cls)
    assert np.array_equal(_bits(sgt.boxes).cpu().numpy(), want_boxes.view(np.int32))
    assert np.array_equal(overflow.cpu().numpy(), ref['overflow'])
    assert np.array_equal(ign.cpu().numpy(), boxes.pack_ignore_bits(ref['ignore']))     # every word, the tail bits of the last one included
    d = sgt.deltas.cpu().numpy()
    assert np.isfinite(d).all(), 'an entry of deltas was left unwritten'
    assert np.array_equal(d[:, :2].view(np.int32), ref['deltas'][:, :2].view(np.int32)), 'dx / dy differ'
    step = _ulps(d[:, 2:], ref['deltas'][:, 2:])
    print(f'{case["name"]}: extras {ref["extras"].tolist()} band {ref["band"].tolist()} overflow {ref["overflow"].tolist()}; '
          f'dw / dh max {int(step.max()) if step.size else 0} ulp')
    assert (step <= 1).all(), 'dw / dh off by more than 1 ulp'
    assert np.array_equal(_bits(sgt.deltas).cpu().numpy()[pad], np.zeros((int(pad.sum()), 4), np.int32))
    # the same operands again, fresh buffers, no out=: the same bits
    _, (sgt2, ign2, overflow2) = _match(case)
    for x, y in zip([*sgt, ign, overflow], [*sgt2, ign2, overflow2]):
        assert torch.equal(_bits(x), _bits(y))
    # distinct anchors per image (the SparseGT contract)
    for b in range(B):
        seg = ref['anchor_idx'][ref['offsets'][b]:ref['offsets'][b + 1]]
        seg = seg[seg < A]
        assert len(set(seg.tolist())) == seg.shape[0]


def test_a_million_anchors():
    """A = 2^20, the limit: 4096 blocks in the count table, 64 of them per lane of the scan.  The reference is the host twin
    ``boxes.anchor_match``, which tests/test_anchor_match_host.py holds to the restatement bit for bit (the restatement walks the anchors
    one by one).  Boxes sit on anchor 0, the last anchor and the middle one among others; image 0 overflows."""
    A = 1 << 20
    rs = np.random.RandomState(5)
    anchors = G._cloud(rs, A, extent=4000.0)
    box_list = [M._around(anchors, rs.choice(A, 5, replace=False), rs, 0.1), M._around(anchors, np.array([0, A - 1, A // 2]), rs, 0.15)]
    case = dict(name='million', anchors=anchors, boxes=box_list, cls=[np.arange(b.shape[0], dtype=np.int32) % 3 for b in box_list], C=3,
                pos_iou=0.5, ign_iou=0.4, max_extra=16, ignore_in=None)
    prim = [G.compute_deltas(b, anchors)[1] for b in box_list]
    idx, box_idx, deltas, offsets, ignore, overflow = boxes.anchor_match(anchors, box_list, prim, 0.5, 0.4, 16)
    assert overflow[0] > 0 and ignore[1].any() and int((idx < A).sum()) > 8 + 16
    enc, (sgt, ign, ovf) = _match(case, out=_garbage(case))
    assert np.array_equal(enc.anchor_idx.cpu().numpy(), np.concatenate(prim).astype(np.int32))
    assert np.array_equal(sgt.anchor_idx.cpu().numpy(), idx) and np.array_equal(sgt.offsets.cpu().numpy(), offsets)
    assert np.array_equal(ovf.cpu().numpy(), overflow) and np.array_equal(ign.cpu().numpy(), boxes.pack_ignore_bits(ignore))
    all_boxes = np.concatenate(box_list, 0)
    assert np.array_equal(sgt.boxes.cpu().numpy(), np.where(box_idx[:, None] < 0, np.float32(0), all_boxes[np.maximum(box_idx, 0)]))
    d = sgt.deltas.cpu().numpy()
    assert np.array_equal(d[:, :2].view(np.int32), deltas[:, :2].view(np.int32)) and (_ulps(d[:, 2:], deltas[:, 2:]) <= 1).all()


def test_total_zero_is_all_padding():
    a64 = torch.from_numpy(G.grid_anchors('64x96')).cuda()
    A = a64.shape[0]
    empty = ops.SparseGT(torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(0, 4, device='cuda'), torch.zeros(0, 4, device='cuda'),
                         torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(3, dtype=torch.int32, device='cuda'))
    bits = torch.from_numpy(boxes.pack_ignore_bits(np.random.RandomState(1).rand(2, A) < 0.3)).cuda()
    sgt, ign, overflow = ops.anchor_match(empty, a64, 0.5, 0.4, 5, ignore=bits)
    torch.cuda.synchronize()
    assert sgt.anchor_idx.tolist() == [A] * 10 and sgt.offsets.tolist() == [0, 5, 10] and overflow.tolist() == [0, 0]
    assert not sgt.boxes.any() and not sgt.deltas.any() and not sgt.class_ids.any() and torch.equal(ign, bits)
    sgt, ign, overflow = ops.anchor_match(empty, a64, 0.5, None, 0)
    torch.cuda.synchronize()
    assert sgt.anchor_idx.shape == (0,) and sgt.offsets.tolist() == [0, 0, 0] and not ign.any() and overflow.tolist() == [0, 0]


def test_status_codes_through_the_raw_entry():
    """Malformed arguments and the limits are refused on the host: the status comes back and no output changes."""
    from squeezedet_pytorch_amd import _native as nat
    case = next(c for c in M.cases() if c['name'] == 'one-image')
    enc, a64, _ = _encode(case)
    out, mask, overflow = _garbage(case)
    before = [t.clone() for t in [*out, mask, overflow]]
    total, A = enc.anchor_idx.shape[0], a64.shape[0]
    ws = torch.empty(A + 1, dtype=torch.int32, device='cuda')

    def call(thr=(case['pos_iou'], case['ign_iou']), total=total, B=1, A=A, cap=case['max_extra'], drop=()):
        t = dict(boxes=enc.boxes, class_ids=enc.class_ids, box_offsets=enc.offsets, anchor_idx=enc.anchor_idx, deltas=enc.deltas, anchors=a64,
                 ignore_in=None, workspace=ws, out_anchor_idx=out.anchor_idx, out_boxes=out.boxes, out_deltas=out.deltas,
                 out_class_ids=out.class_ids, out_offsets=out.offsets, ignore_out=mask, overflow=overflow)
        p = {k: (None if k in drop else nat.ptr(v)) for k, v in t.items()}
        thr_p = None if 'thresholds' in drop else (ctypes.c_double * 2)(*thr)
        return nat.lib().sqd_anchor_match_fwd(p['boxes'], p['class_ids'], p['box_offsets'], p['anchor_idx'], p['deltas'], p['anchors'],
                                              p['ignore_in'], thr_p, p['workspace'], p['out_anchor_idx'], p['out_boxes'], p['out_deltas'],
                                              p['out_class_ids'], p['out_offsets'], p['ignore_out'], p['overflow'], total, B, A, cap,
                                              nat.stream_handle(a64.device))
    for name in ('boxes', 'class_ids', 'box_offsets', 'anchor_idx', 'deltas', 'anchors', 'thresholds', 'workspace', 'out_anchor_idx', 'out_boxes',
                 'out_deltas', 'out_class_ids', 'out_offsets', 'ignore_out', 'overflow'):
        assert call(drop=(name,)) == nat.ERR_BAD_ARG, name
    for thr in ((0.0, 0.0), (0.5, 0.0), (0.5, 0.6), (1.5, 0.5), (float('nan'), 0.5), (0.5, float('nan'))):
        assert call(thr=thr) == nat.ERR_BAD_ARG, thr
    assert call(cap=-1) == nat.ERR_BAD_ARG
    assert call(A=2 ** 20 + 1) == nat.ERR_UNSUPPORTED and call(B=65536) == nat.ERR_UNSUPPORTED
    assert call(total=2 ** 31 - 1, cap=1) == nat.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for x, y in zip([*out, mask, overflow], before):
        assert torch.equal(_bits(x), _bits(y)), 'a refused call wrote an output'
    assert call() == 0                                   # and the well-formed call of the same operands runs
    torch.cuda.synchronize()
    assert np.array_equal(out.anchor_idx.cpu().numpy(), M.reference(case)['anchor_idx'])


# ---- the matcher's lists through the masked loss ---------------------------------------------------------------------------------------------

def _loss_operands(A, C, seed, B=3, max_extra=256):
    """Predictions and anchors of ``LG.random_case`` (a 96 x 64 frame: the anchors overlap one another well), boxes around a few of the
    anchors, image 1 without a box; the matcher's output for them: hundreds of entries per image, most of them padding at A = 33."""
    pred, _, anchors = LG.random_case(B, A, C, seed=seed)
    a64 = anchors.double().numpy()
    rs = np.random.RandomState(seed + 1)
    box_list = [M._around(a64, rs.choice(A, min(A, 5), replace=False), rs, 0.1), M.EMPTY, M._around(a64, rs.choice(A, min(A, 9), replace=False), rs, 0.2)]
    box_list = [np.clip(b, 0, [LG.SIZE[1] - 1, LG.SIZE[0] - 1] * 2).astype(np.float32) for b in box_list]
    box_list = [b[(b[:, 2] - b[:, 0] > 1) & (b[:, 3] - b[:, 1] > 1)] for b in box_list]
    case = dict(anchors=a64, boxes=box_list, cls=[rs.randint(0, C, b.shape[0]).astype(np.int32) for b in box_list], C=C, ignore_in=None)
    enc, d_a64, _ = _encode(case)
    sgt, ign, overflow = ops.anchor_match(enc, d_a64, 0.3, 0.2, max_extra)
    torch.cuda.synchronize()
    assert int((sgt.anchor_idx < A).sum()) > enc.anchor_idx.shape[0] and bool((ign != 0).any())       # extras and a band are there
    return pred, anchors, sgt, ign, overflow


def _check_loss(tag, kind, pred, anchors, sgt, ign, C):
    B, A = pred.shape[:2]
    w = LG.WEIGHTS if kind == 'l2' else LG.WEIGHTS + (kind,)
    p, a = pred.cuda(), anchors.cuda()
    coef = LG.make_coef(B, 3)
    per = (sgt.offsets[1:] - sgt.offsets[:-1]).tolist()
    valid = [int((sgt.anchor_idx[sgt.offsets[b]:sgt.offsets[b + 1]] < A).sum()) for b in range(B)]
    print(f'{tag}: entries per image {per}, positives {valid}')
    assert min(per) >= 200 and valid[0] >= 5 and valid[1] == 0                  # long lists, padding included; image 1 object-free
    losses_m, counts, mean4 = ops.loss_masked_mean_fwd(p, sgt, ign, a, LG.SIZE, C, w)
    losses, counts_p = ops.loss_masked_fwd(p, sgt, ign, a, LG.SIZE, C, w)
    dm = ops.loss_masked_mean_bwd(p, sgt, ign, a, counts, TG.GM(), LG.SIZE, C, w, out=torch.full_like(p, float('nan')))
    dc = ops.loss_masked_bwd(p, sgt, ign, a, counts_p, coef.cuda(), LG.SIZE, C, w, out=torch.full_like(p, float('nan')))
    torch.cuda.synchronize()
    assert torch.equal(_bits(losses), _bits(losses_m)) and torch.equal(_bits(counts), _bits(counts_p))
    gt = ops.sparse_gt_to_dense(sgt, A, C).cpu()
    bits = boxes.unpack_ignore_bits(ign.cpu().numpy(), A)
    if kind == 'l2':
        ref = IR.masked_loss(pred, gt, bits, anchors, LG.SIZE, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=coef)
    else:
        ref = Q.masked_loss(kind, pred, gt, bits, anchors, LG.SIZE, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=coef)
    assert torch.equal(counts.cpu().double(), ref['counts']) and ref['counts'][0].tolist() == [float(v) for v in valid]
    for t in (losses, mean4, dm, dc):
        assert torch.isfinite(t).all(), 'a masked launch left a NaN / an unwritten element'
    res = {'losses': R.bars_nan(losses.cpu(), ref['losses'], 'vec', 2), 'mean4': R.bars_nan(mean4.cpu(), ref['mean4'], 'vec', 2)}
    for name, got in (('dmean', dm.cpu()), ('dcoef', dc.cpu())):
        res[name] = R.bars_nan(got, R.pick(got, ref[name], ref[name + '_alt'], ref['flips']), 'dpred', 2)
        assert bool((_bits(got)[ref['ign']] == 0).all()), 'an ignored row is not +0.0 bit for bit'
    flips = int(ref['flips'].sum())
    for k, b in res.items():
        print(f'matched list {tag:24s} {k:6s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e}) flips {flips}')
    assert all(b['l_ok'] for b in res.values()), (tag, res)
    assert flips <= LG.MAX_FLIPS


@pytest.mark.parametrize('C', [3, 20])
@pytest.mark.parametrize('A', [33, 517])
def test_long_lists_through_the_masked_loss(A, C):
    pred, anchors, sgt, ign, overflow = _loss_operands(A, C, seed=800 + A + C)
    assert overflow.tolist() == [0, 0, 0]
    _check_loss(f'A{A} C{C}', 'l2', pred, anchors, sgt, ign, C)


def test_long_lists_through_the_giou_loss():
    pred, anchors, sgt, ign, _ = _loss_operands(517, 3, seed=77)
    _check_loss('A517 C3 giou', 'giou', pred, anchors, sgt, ign, 3)


# ---- loader -> trainer -----------------------------------------------------------------------------------------------------------------------

class _WideBoxes(IR.FlaggedDataset):
    """Six 70 x 100 images (no resize) with 0..3 boxes of 40..80 x 30..50 pixels: what the wide anchor shapes of neighbouring cells
    overlap by more than a half.  Image 4 has no box."""
    SIZES = [(70, 100)] * 6

    def __init__(self):
        super().__init__('deleted')
        rs = np.random.RandomState(12)
        self.ann = []
        for i in range(6):
            n = 0 if i == 4 else 1 + i % 3
            w, h = rs.uniform(40, 80, n), rs.uniform(30, 50, n)
            x, y = rs.uniform(2, 97 - w), rs.uniform(2, 67 - h)
            self.ann.append((rs.randint(0, 3, n).astype(np.int64), np.stack([x, y, x + w, y + h], 1).astype(np.float32).reshape(-1, 4),
                             np.zeros(n, np.uint8)))


def _match_cfg(**kw):
    return sqd.make_cfg(input_size=(70, 100), dropout_prob=0, sparse_gt=True, match_iou=0.5, match_ignore_iou=0.4, **kw)


def test_loader_to_trainer_eager_and_captured():
    """Two steps of ``Trainer`` on ``TrainLoader`` batches with the matcher on: n_obj per image is the restatement's count on the plan's
    boxes, the bitmap and the overflow are its too, the losses are finite, and the same run as one captured hipGraph ends on the same
    bits."""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    ds = _WideBoxes()
    cfg = _match_cfg()
    A = cfg.num_anchors
    a64 = np.asarray(cfg.anchors, np.float64)
    cfg.batch_size, cfg.num_workers, cfg.device = 3, 0, 'cuda'
    plans = list(TrainLoader(ds, cfg, seed=3, shuffle=False).plan())
    seen = 0
    for batch, p in zip(TrainLoader(ds, cfg, seed=3, shuffle=False), plans):
        assert set(batch) == {'image', 'image_meta', 'gt_sparse', 'gt_ignore', 'gt_match_overflow'}
        sgt, overflow = batch['gt_sparse'], batch['gt_match_overflow']
        assert overflow.is_cuda and overflow.dtype == torch.int32 and tuple(overflow.shape) == (3,)
        prim = [G.compute_deltas(b, a64) for b in p['boxes']]
        ref = M.match(a64, p['boxes'], [q[1] for q in prim], [q[0] for q in prim], 0.5, 0.4, cfg.match_max_extra)
        assert np.array_equal(sgt.anchor_idx.cpu().numpy(), ref['anchor_idx']) and np.array_equal(sgt.offsets.cpu().numpy(), ref['offsets'])
        assert np.array_equal(batch['gt_ignore'].cpu().numpy(), boxes.pack_ignore_bits(ref['ignore']))
        assert np.array_equal(overflow.cpu().numpy(), ref['overflow'])
        n_obj = [int((ref['anchor_idx'][ref['offsets'][b]:ref['offsets'][b + 1]] < A).sum()) for b in range(3)]
        want = [len(p['boxes'][b]) + min(int(ref['extras'][b]), cfg.match_max_extra) for b in range(3)]
        assert n_obj == want
        pred = torch.zeros(3, A, cfg.num_classes + 5, device='cuda')
        weights = (cfg.class_loss_weight, cfg.positive_score_loss_weight, cfg.negative_score_loss_weight, cfg.bbox_loss_weight)
        anchors32 = torch.from_numpy(np.asarray(cfg.anchors, np.float32)).cuda()
        _, counts = ops.loss_masked_fwd(pred, sgt, batch['gt_ignore'], anchors32, (70, 100), cfg.num_classes, weights)
        assert counts[0].tolist() == [float(v) for v in n_obj]
        print(f'loader batch: boxes {[len(b) for b in p["boxes"]]} n_obj {n_obj} band {ref["band"].tolist()}')
        seen += sum(n_obj) - sum(len(b) for b in p['boxes'])
    assert seen >= 5, 'the loader batches hold too few extra positives'
    runs = {}
    for flag in (False, True):
        torch.manual_seed(9)
        c = _match_cfg(graph_step=flag)
        m, tr = TG._trainer(c, 3)
        out = tr.train_epoch(1, TrainLoader(ds, c, seed=3, shuffle=False))
        torch.cuda.synchronize()
        assert all(np.isfinite(out[k]) for k in tr.metrics), out
        assert all(torch.isfinite(q).all() for q in m.parameters())
        runs[flag] = (m, tr, out)
    gs = runs[True][1].graphed_step()
    assert gs.captures == 1 and gs.replays == 1 and gs.eager_steps == 1
    for (n, pa), (_, pb) in zip(runs[True][0].named_parameters(), runs[False][0].named_parameters()):
        assert torch.equal(_bits(pa), _bits(pb)), f'parameter {n} differs between graph_step on and off'
    assert torch.equal(_bits(runs[True][1].optimizer.momentum_flat), _bits(runs[False][1].optimizer.momentum_flat))
    for k in runs[False][1].metrics:
        assert abs(runs[True][2][k] - runs[False][2][k]) <= 1e-5 * abs(runs[False][2][k]), k      # (the device log sums in float64)


def test_feature_off_is_todays_path(monkeypatch):
    """``match_iou = None``: the loader runs the encoder alone, the matcher is never called and the batch has the keys it had."""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    calls = TG._count_calls(monkeypatch, ['anchor_match', 'encode_gt', 'anchor_ignore_mask', 'loss_masked_mean_fwd', 'loss_sparse_mean_fwd',
                                          'loss_sparse_mean_bwd'])
    cfg = sqd.make_cfg(input_size=(70, 100), dropout_prob=0.0, sparse_gt=True)
    m, tr = TG._trainer(cfg, 3)
    ds = IR.FlaggedDataset('deleted')
    loader = TrainLoader(TG._Subset(ds, [0, 1, 2, 4, 6, 0]), cfg, seed=3, shuffle=False)
    steps = 0
    for batch in loader:
        assert set(batch) == {'image', 'image_meta', 'gt_sparse'}
        batch = tr._to_device(batch)
        assert set(batch) == {'image', 'image_meta', 'gt_sparse'}
        before = dict(calls)
        values, _ = tr._iteration(batch, True)
        assert all(np.isfinite(v) for v in values)
        assert calls['loss_sparse_mean_fwd'] == before['loss_sparse_mean_fwd'] + 1
        assert calls['loss_sparse_mean_bwd'] == before['loss_sparse_mean_bwd'] + 1
        steps += 1
    assert steps == 2 and calls['encode_gt'] == 2
    assert calls['anchor_match'] == 0 and calls['anchor_ignore_mask'] == 0 and calls['loss_masked_mean_fwd'] == 0
