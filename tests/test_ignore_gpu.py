"""GPU tier of the ignore regions: the anchor ignore bitmap (``ops.anchor_ignore_mask``, csrc/gt_encode.hip) against the numpy rule
word for word; the masked sparse loss (``ops.loss_masked_*``, csrc/loss.hip) bit-equal to the sparse launches on a zero bitmap and
held to the float64 reference of tests/ignore_ref.py at the bars of fp64_ref (as ``test_sparse_loss_gpu.test_encoder_to_loss``
applies them); ignored rows, determinism, and every layer above: encoder -> ``Loss``, ``TrainLoader`` -> ``Trainer``."""
import numpy as np
import pytest
import torch

import fp64_ref as R
import ignore_ref as IR
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import boxes, ops, synthetic
from squeezedet_pytorch_amd.annotations import anchors_f64_on, encode_annotations
import test_fp64_loss_gpu as LG

pytestmark = pytest.mark.gpu

GM = lambda: torch.tensor([LG.GMEAN], dtype=torch.float32, device='cuda')     # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the bitmap kernel ------------------------------------------------------------------------------------------------------------------

def _anchors_and_regions(A, seed):
    """A anchors (the KITTI grid at A = 16848, else random in a 96 x 64 frame, a few of them without area) and B = 3 images with
    0, 1 and 300 ignore boxes (300 crosses the 256-box chunk the kernel stages)."""
    rs = np.random.RandomState(seed)
    if A == 16848:
        anchors, (H, W) = np.asarray(sqd.make_cfg().anchors, np.float64), (384, 1248)
    else:
        anchors, (H, W) = np.stack([rs.uniform(0, 96, A), rs.uniform(0, 64, A), rs.uniform(1, 40, A), rs.uniform(1, 40, A)], 1), (64, 96)
        anchors[::7, 2] = 1.0
    regions = []
    for n in (0, 1, 300):
        w, h = rs.uniform(2, W / 3, n), rs.uniform(2, H / 3, n)
        x, y = rs.uniform(0, W - 1 - w), rs.uniform(0, H - 1 - h)
        regions.append(np.stack([x, y, x + w, y + h], 1).astype(np.float32).reshape(-1, 4))
    if A != 16848:                                       # the last anchor, the top bit of the tail word: small, in the middle of a region
        r = regions[2][0]
        anchors[-1] = ((r[0] + r[2]) / 2, (r[1] + r[3]) / 2, 2.0, 2.0)
    return anchors, regions


def _device_bitmap(anchors, regions, overlap, prefill=True):
    offs = np.zeros(len(regions) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in regions])
    A = anchors.shape[0]
    out = torch.full((len(regions), ops.ignore_words(A)), -1, dtype=torch.int32, device='cuda') if prefill else None     # 0xFFFFFFFF
    got = ops.anchor_ignore_mask(torch.from_numpy(np.concatenate(regions, 0)).cuda(), torch.from_numpy(offs).cuda(),
                                 torch.from_numpy(np.ascontiguousarray(anchors, np.float64)).cuda(), overlap, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize('overlap', [0.5, 1.0])
@pytest.mark.parametrize('A', [1, 31, 32, 33, 64, 517, 16848])
def test_bitmap_equals_the_numpy_rule(A, overlap):
    anchors, regions = _anchors_and_regions(A, seed=A)
    want = np.stack([boxes.anchor_ignore_mask(anchors, r, overlap) for r in regions])
    got = _device_bitmap(anchors, regions, overlap)
    assert got.shape == (3, (A + 31) // 32) and got.dtype == np.int32
    assert np.array_equal(got, boxes.pack_ignore_bits(want))             # every word, the tail bits of the last one included
    assert not want[0].any() and (A < 500 or not want[2].all()) and (A == 16848 or want[2, A - 1])
    print(f'bitmap A{A} overlap {overlap}: ignored per image {want.sum(1).tolist()}')


@pytest.mark.parametrize('case', IR.boundary_cases(), ids=lambda c: c[0])
def test_bitmap_boundaries(case):
    _, anchors, regions, overlap, want = case
    got = _device_bitmap(anchors, [regions], overlap)
    assert boxes.unpack_ignore_bits(got, len(want))[0].tolist() == want
    assert np.array_equal(got, boxes.pack_ignore_bits(np.array([want])))


def test_bitmap_limits_through_the_raw_entry():
    import ctypes
    from squeezedet_pytorch_amd import _native as nat
    a = torch.zeros(4, 4, dtype=torch.float64, device='cuda')
    offs, out = torch.zeros(2, dtype=torch.int32, device='cuda'), torch.zeros(1, 1, dtype=torch.int32, device='cuda')
    call = lambda ov, total, B, A: nat.lib().sqd_anchor_ignore_fwd(None, nat.ptr(offs), nat.ptr(a), nat.ptr(out),      # noqa: E731
                                                                  ctypes.byref(ctypes.c_double(ov)), total, B, A, nat.stream_handle(a.device))
    assert call(0.5, 0, 1, 4) == 0
    assert call(0.0, 0, 1, 4) == 1 and call(1.5, 0, 1, 4) == 1 and call(float('nan'), 0, 1, 4) == 1 and call(0.5, 3, 1, 4) == 1
    assert call(0.5, 0, 1, 2 ** 20 + 1) == 2 and call(0.5, 0, 65536, 4) == 2
    torch.cuda.synchronize()


# ---- the masked loss ----------------------------------------------------------------------------------------------------------------------

def _dev_bitmap(ign):
    return torch.from_numpy(boxes.pack_ignore_bits(np.asarray(ign))).cuda()


def run_masked(pred, gt, anchors, ign, C, coef=None, size=LG.SIZE, tag=''):
    """All four masked launches on one operand set, each output against ignore_ref.masked_loss at the bars of fp64_ref; the plain and
    the mean forward bitwise equal; counts exact; rows of ign exact zeros.  -> the reference."""
    B, A = pred.shape[:2]
    coef = LG.make_coef(B, 3) if coef is None else coef
    p, a, bm = pred.cuda(), anchors.cuda(), _dev_bitmap(ign)
    sgt = ops.sparse_gt_from_dense(gt.cuda())
    losses, counts = ops.loss_masked_fwd(p, sgt, bm, a, size, C, LG.WEIGHTS)
    losses_m, counts_m, mean4 = ops.loss_masked_mean_fwd(p, sgt, bm, a, size, C, LG.WEIGHTS)
    nan = torch.full_like(p, float('nan'))
    dm = ops.loss_masked_mean_bwd(p, sgt, bm, a, counts_m, GM(), size, C, LG.WEIGHTS, out=nan.clone())
    dc = ops.loss_masked_bwd(p, sgt, bm, a, counts, coef.cuda(), size, C, LG.WEIGHTS, out=nan.clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(losses), _bits(losses_m)) and torch.equal(_bits(counts), _bits(counts_m)), 'plain and mean forward differ'
    ref = IR.masked_loss(pred, gt, ign, anchors, size, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=coef)
    assert torch.equal(counts.cpu().double(), ref['counts']), (counts, ref['counts'])
    for t in (losses, mean4, dm, dc):
        assert torch.isfinite(t).all(), 'a masked launch left a NaN / an unwritten element'
    res = {'losses': R.bars_nan(losses.cpu(), ref['losses'], 'vec', 2), 'mean4': R.bars_nan(mean4.cpu(), ref['mean4'], 'vec', 2)}
    for name, got in (('dmean', dm.cpu()), ('dcoef', dc.cpu())):
        res[name] = R.bars_nan(got, R.pick(got, ref[name], ref[name + '_alt'], ref['flips']), 'dpred', 2)
        assert bool((_bits(got)[ref['ign']] == 0).all()), 'an ignored row is not +0.0 bit for bit'
    flips = int(ref['flips'].sum())
    for k, b in res.items():
        print(f'masked {tag:30s} {k:6s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e}) NaN positions ok={b["nan_ok"]} flips {flips}')
    assert all(b['l_ok'] for b in res.values()), (tag, res)
    assert flips <= LG.MAX_FLIPS
    return ref, losses.cpu(), dm.cpu(), dc.cpu()


@pytest.mark.parametrize('C', [3, 20, 80])
def test_zero_bitmap_is_the_sparse_loss(C):
    A, B = 517, 3
    pred, gt, anchors = LG.random_case(B, A, C, seed=600 + C)
    p, a = pred.cuda(), anchors.cuda()
    sgt = ops.sparse_gt_from_dense(gt.cuda())
    bm = torch.zeros(B, ops.ignore_words(A), dtype=torch.int32, device='cuda')
    coef = LG.make_coef(B, 3).cuda()
    l_s, nobj = ops.loss_sparse_fwd(p, sgt, a, LG.SIZE, C, LG.WEIGHTS)
    lm_s, nobj_m, mean_s = ops.loss_sparse_mean_fwd(p, sgt, a, LG.SIZE, C, LG.WEIGHTS)
    dc_s = ops.loss_sparse_bwd(p, sgt, a, nobj, coef, LG.SIZE, C, LG.WEIGHTS)
    dm_s = ops.loss_sparse_mean_bwd(p, sgt, a, nobj_m, GM(), LG.SIZE, C, LG.WEIGHTS)
    l_k, counts = ops.loss_masked_fwd(p, sgt, bm, a, LG.SIZE, C, LG.WEIGHTS)
    lm_k, counts_m, mean_k = ops.loss_masked_mean_fwd(p, sgt, bm, a, LG.SIZE, C, LG.WEIGHTS)
    dc_k = ops.loss_masked_bwd(p, sgt, bm, a, counts, coef, LG.SIZE, C, LG.WEIGHTS)
    dm_k = ops.loss_masked_mean_bwd(p, sgt, bm, a, counts_m, GM(), LG.SIZE, C, LG.WEIGHTS)
    torch.cuda.synchronize()
    assert float(nobj.min()) > 0
    for name, x, y in (('losses', l_s, l_k), ('losses (mean form)', lm_s, lm_k), ('mean4', mean_s, mean_k), ('dcoef', dc_s, dc_k),
                       ('dmean', dm_s, dm_k), ('n_obj', nobj, counts[0]), ('n_obj (mean form)', nobj_m, counts_m[0])):
        assert torch.equal(_bits(x), _bits(y)), name
    assert torch.equal(counts[1], A - nobj)


@pytest.mark.parametrize('density', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('C', [1, 3, 17, 80])
@pytest.mark.parametrize('A', [1, 33, 517])
def test_against_the_float64_reference(A, C, density):
    """Four images per case (ignore_ref.case_with_ignore): ordinary with positives whose own bit is set, n_obj = 0, n_neg = 0,
    n_obj = 0 with every bit set."""
    pred, gt, anchors, ign = IR.case_with_ignore(LG, A, C, seed=700 + A + C, density=density)
    ref, losses, dm, dc = run_masked(pred, gt, anchors, ign, C, tag=f'A{A} C{C} density {density}')
    assert ref['counts'][0].tolist()[1::2] == [0.0, 0.0] and ref['counts'][1].tolist()[2:] == [0.0, 0.0]
    assert torch.equal(_bits(losses[[0, 2]][:, [1, 3]]), torch.zeros(2, 2, dtype=torch.int32))           # n_obj = 0: class = bbox = 0
    assert float(losses[1, 1]) == float(losses[3, 1])                                                     # ... and pos = 0: score = total
    assert torch.equal(_bits(losses[:, 3]), torch.zeros(4, dtype=torch.int32))                            # n_obj = 0, all ignored: losses == 0
    assert torch.equal(_bits(dm[3]), torch.zeros_like(_bits(dm[3]))) and torch.equal(_bits(dc[3]), torch.zeros_like(_bits(dc[3])))
    if density > 0 and A > 1:
        first = int(torch.nonzero(gt[0, :, 0] > 0)[0])
        assert ign[0, first] and bool((dm[0, first] != 0).any())                                          # a positive wins over its own bit


def test_kitti_anchor_count_against_the_reference():
    A, C = 16848, 3
    pred, gt, anchors = LG.random_case(2, A, C, seed=100 + A, nobj=[60, 0])
    ign = np.random.RandomState(5).rand(2, A) < 0.3
    ign[0, int(torch.nonzero(gt[0, :, 0] > 0)[0])] = True
    run_masked(pred, gt, anchors, ign, C, tag='A16848 B2 C3')


@pytest.mark.parametrize('C', [3, 17])
def test_exact_branch_edges_with_a_bitmap(C):
    """LG.edge_case: the positives sit exactly on clamp bounds, ties and touching edges; a bitmap must not move any of them."""
    pred, gt, anchors = LG.edge_case(C=C)
    ign = np.random.RandomState(9).rand(2, pred.shape[1]) < 0.3
    ref, *_ = run_masked(pred, gt, anchors, ign, C, tag=f'edges C{C}')
    assert int(ref['flips'].sum()) == 0


def test_ignored_rows_unaligned_dpred_and_determinism():
    """Ignored rows that are no positives are +0.0 bit for bit in a dpred pre-filled with NaN, also through the element-wise path an
    unaligned dpred takes (a view one float into its buffer); the same operands twice give the same bits."""
    A, C, B = 517, 3, 4
    pred, gt, anchors, ign = IR.case_with_ignore(LG, A, C, seed=41, density=0.3)
    p, a, bm = pred.cuda(), anchors.cuda(), _dev_bitmap(ign)
    sgt = ops.sparse_gt_from_dense(gt.cuda())
    coef = LG.make_coef(B, 3).cuda()
    rows = torch.from_numpy(ign) & ~(gt[..., 0] > 0)
    assert 0 < int(rows.sum()) < B * A
    outs = []
    for _ in range(2):
        losses, counts, mean4 = ops.loss_masked_mean_fwd(p, sgt, bm, a, LG.SIZE, C, LG.WEIGHTS)
        dm = ops.loss_masked_mean_bwd(p, sgt, bm, a, counts, GM(), LG.SIZE, C, LG.WEIGHTS, out=torch.full_like(p, float('nan')))
        dc = ops.loss_masked_bwd(p, sgt, bm, a, counts, coef, LG.SIZE, C, LG.WEIGHTS, out=torch.full_like(p, float('nan')))
        outs.append((losses, counts, mean4, dm, dc))
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))
    losses, counts, mean4, dm, dc = outs[0]
    buf = torch.full((p.numel() + 1,), float('nan'), device='cuda')
    off = buf[1:].view_as(p)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    for aligned, fn in ((dm, lambda o: ops.loss_masked_mean_bwd(p, sgt, bm, a, counts, GM(), LG.SIZE, C, LG.WEIGHTS, out=o)),
                        (dc, lambda o: ops.loss_masked_bwd(p, sgt, bm, a, counts, coef, LG.SIZE, C, LG.WEIGHTS, out=o))):
        buf.fill_(float('nan'))
        got = fn(off)
        assert got.data_ptr() == off.data_ptr() and torch.isnan(buf[0])
        assert torch.equal(_bits(got), _bits(aligned))
        assert bool((_bits(got).cpu()[rows] == 0).all()) and bool((_bits(aligned).cpu()[rows] == 0).all())
        assert torch.isfinite(got).all()


# ---- encoder -> loss, loader -> trainer ----------------------------------------------------------------------------------------------------

def _model(cfg, C):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234, num_classes=C), strict=True)
    return m.cuda().train()


@pytest.mark.parametrize('C', [3, 20])
def test_encoder_to_loss(C):
    from squeezedet_pytorch_amd.model import Loss
    size, B = (70, 100), 3
    cfg = sqd.make_cfg(input_size=size, num_classes=C, sparse_gt=True, ignore_overlap=0.5)
    A = cfg.num_anchors
    cls_list, box_list = synthetic.make_gt_boxes(B, size, num_classes=C, seed=31 + C, min_boxes=2, max_boxes=4)
    cls_list, box_list = list(cls_list), list(box_list)
    cls_list[2], box_list[2] = np.zeros(0, np.int64), np.zeros((0, 4), np.float32)                 # an object-free image
    ign_list = [np.array([[5, 5, 60, 40], [50, 30, 99, 69]], np.float32), np.zeros((0, 4), np.float32), np.array([[0, 0, 70, 69]], np.float32)]
    sgt, bm = encode_annotations(cls_list, box_list, cfg.anchors, C, dense=False, ignore_boxes_list=ign_list, ignore_overlap=0.5)
    ign = np.stack([boxes.anchor_ignore_mask(cfg.anchors, r, 0.5) for r in ign_list])
    assert np.array_equal(bm.cpu().numpy(), boxes.pack_ignore_bits(ign)) and ign[0].any() and ign[2].any() and not ign[1].any()
    assert sgt.offsets.tolist()[2:] == [sgt.anchor_idx.shape[0]] * 2
    rs = np.random.RandomState(40 + C)
    pred = np.empty((B, A, C + 5), np.float32)
    pred[..., :C] = rs.standard_normal((B, A, C)) * 2
    pred[..., C] = rs.standard_normal((B, A)) * 1.5 - 2
    pred[..., C + 1:] = rs.standard_normal((B, A, 4)) * 0.4
    pred = torch.from_numpy(pred)
    weights = (cfg.class_loss_weight, cfg.positive_score_loss_weight, cfg.negative_score_loss_weight, cfg.bbox_loss_weight)
    loss_mod = Loss(cfg).cuda()
    p = pred.cuda().requires_grad_(True)
    mean, parts = loss_mod.mean_loss(p, sgt, bm)
    mean.backward()
    a = loss_mod.resolver.anchors_on(p.device)
    losses, counts, mean4 = ops.loss_masked_mean_fwd(p.detach(), sgt, bm, a, size, C, weights)
    direct = ops.loss_masked_mean_bwd(p.detach(), sgt, bm, a, counts, torch.ones(1, device='cuda'), size, C, weights)
    assert torch.equal(_bits(p.grad), _bits(direct)) and torch.equal(_bits(mean.detach()), _bits(mean4[3]))
    assert torch.equal(_bits(parts['loss']), _bits(losses[3])) and torch.isfinite(p.grad).all() and float(counts[0, 2]) == 0
    # the per-image form gives the same per-image values
    loss, _ = loss_mod(p.detach().requires_grad_(True), sgt, bm)
    assert torch.equal(_bits(loss.detach()), _bits(losses[3]))
    # and the whole chain holds the bars against float64 on the dense gt the list stands for
    gt = ops.sparse_gt_to_dense(sgt, A, C).cpu()
    ref = IR.masked_loss(pred, gt, ign, a.cpu(), size, C, weights, gmean=1.0)
    res = {'losses': R.bars_nan(losses.cpu(), ref['losses'], 'vec', 2), 'mean4': R.bars_nan(mean4.cpu(), ref['mean4'], 'vec', 2),
           'dmean': R.bars_nan(direct.cpu(), R.pick(direct.cpu(), ref['dmean'], ref['dmean_alt'], ref['flips']), 'dpred', 2)}
    for k, b in res.items():
        print(f'encoder -> masked loss C{C} {k:6s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e})')
    assert all(b['l_ok'] for b in res.values()), res
    assert torch.equal(counts.cpu().double(), ref['counts']) and int(ref['flips'].sum()) <= LG.MAX_FLIPS


def test_batch_without_any_box_encodes():
    """A batch whose box total is 0: a well-formed empty ``SparseGT`` (no encoder launch), an all-zero dense gt, and a masked loss
    that is the negatives' term alone."""
    size, C, B = (70, 100), 3, 2
    cfg = sqd.make_cfg(input_size=size)
    A = cfg.num_anchors
    empty_c, empty_b = [np.zeros(0, np.int64)] * B, [np.zeros((0, 4), np.float32)] * B
    sgt, bm = encode_annotations(empty_c, empty_b, cfg.anchors, C, dense=False, ignore_boxes_list=[np.array([[10, 10, 60, 50]], np.float32), []],
                                 ignore_overlap=0.5)
    assert sgt.anchor_idx.shape == (0,) and sgt.boxes.shape == (0, 4) and sgt.deltas.shape == (0, 4) and sgt.class_ids.shape == (0,)
    assert sgt.offsets.tolist() == [0, 0, 0] and all(t.is_cuda for t in sgt) and sgt.anchor_idx.dtype == torch.int32
    assert torch.equal(encode_annotations(empty_c, empty_b, cfg.anchors, C), torch.zeros(B, A, C + 9, device='cuda'))
    one = encode_annotations([np.array([1]), np.zeros(0, np.int64)], [np.array([[10, 10, 60, 50]], np.float32), empty_b[0]], cfg.anchors, C, dense=False)
    assert one.offsets.tolist() == [0, 1, 1] and 0 <= int(one.anchor_idx[0]) < A
    pred = torch.randn(B, A, C + 5, generator=torch.Generator().manual_seed(1))
    a = torch.from_numpy(np.asarray(cfg.anchors, np.float32))
    ign = boxes.unpack_ignore_bits(bm.cpu().numpy(), A)
    assert ign[0].any() and not ign[1].any()
    run_masked(pred, torch.zeros(B, A, C + 9), a, ign, C, size=size, coef=LG.make_coef(B, 3), tag='no box at all')
    losses, counts = ops.loss_masked_fwd(pred.cuda(), sgt, bm, a.cuda(), size, C, LG.WEIGHTS)
    assert counts[0].tolist() == [0.0, 0.0] and counts[1].tolist() == [float(A - ign[0].sum()), float(A)]
    assert torch.equal(_bits(losses[[0, 2]]), torch.zeros(2, B, dtype=torch.int32, device='cuda')) and bool((losses[3] > 0).all())


def _trainer(cfg, C):
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, Trainer
    cfg.num_iters, cfg.print_interval, cfg.grad_norm, cfg.device = -1, 1000, 5.0, 'cuda'
    cfg.gpus, cfg.chunk_sizes, cfg.batch_size, cfg.num_workers = [0], [3], 3, 0
    m = _model(cfg, C)
    opt = FusedClipSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=cfg.grad_norm, flat_grad=lambda: m.base.last_grad_flat)
    return m, Trainer(m, opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)


def _count_calls(monkeypatch, names):
    calls = dict.fromkeys(names, 0)
    for fn in names:
        def counted(*args, _f=getattr(ops, fn), _k=fn, **kw):
            calls[_k] += 1
            return _f(*args, **kw)
        monkeypatch.setattr(ops, fn, counted)
    return calls


def test_loader_to_trainer_with_ignore_regions(monkeypatch):
    """Two steps of ``Trainer`` + ``FusedClipSGD`` on ``TrainLoader`` batches of the 7-image dataset (image 3: flagged boxes only,
    image 5: no annotation): every logged loss is finite and equals the recomputation from the emitted batch, the weights stay
    finite, and the step ran on the masked launches."""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    calls = _count_calls(monkeypatch, ['loss_masked_mean_fwd', 'loss_masked_mean_bwd', 'loss_sparse_mean_fwd'])
    cfg = sqd.make_cfg(input_size=(70, 100), dropout_prob=0.0, sparse_gt=True, ignore_overlap=0.5)
    m, tr = _trainer(cfg, 3)
    ds = IR.FlaggedDataset('flags')
    loader = TrainLoader(ds, cfg, seed=3, shuffle=False)
    plans = list(TrainLoader(ds, cfg, seed=3, shuffle=False).plan())
    steps = 0
    for batch, p in zip(loader, plans):
        batch = tr._to_device(batch)
        assert isinstance(batch['gt_sparse'], ops.SparseGT) and batch['gt_ignore'].dtype == torch.int32 and batch['gt_ignore'].is_cuda
        want_bits = np.stack([boxes.anchor_ignore_mask(cfg.anchors, r, 0.5) for r in p['ignore_boxes']])
        assert np.array_equal(batch['gt_ignore'].cpu().numpy(), boxes.pack_ignore_bits(want_bits))
        mean, parts = m.forward_mean(batch)                        # the recomputation: the same weights, the same batch
        want = [float(parts[k].detach().double().mean()) for k in tr.metrics]
        before = dict(calls)
        values, n = tr._iteration(batch, True)
        assert n == 3 and all(np.isfinite(v) for v in values)
        assert all(abs(v - w) <= 2e-6 * abs(w) for v, w in zip(values, want)), (values, want)
        assert calls['loss_masked_mean_fwd'] == before['loss_masked_mean_fwd'] + 1
        assert calls['loss_masked_mean_bwd'] == before['loss_masked_mean_bwd'] + 1 and calls['loss_sparse_mean_fwd'] == 0
        assert all(torch.isfinite(q).all() for q in m.parameters())
        steps += 1
    assert steps == 2 and {3, 5} <= {int(i) for p in plans for i in p['index']}


def test_feature_off_is_the_sparse_path(monkeypatch):
    """``ignore_overlap = None`` on the flag-free 2-tuple dataset: the batch has no bitmap, no masked launch runs and the step's losses
    are the sparse launches' own, bit for bit."""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    calls = _count_calls(monkeypatch, ['loss_masked_mean_fwd', 'loss_masked_mean_bwd', 'loss_masked_fwd', 'loss_masked_bwd', 'anchor_ignore_mask'])
    cfg = sqd.make_cfg(input_size=(70, 100), dropout_prob=0.0, sparse_gt=True)
    m, tr = _trainer(cfg, 3)
    weights = (cfg.class_loss_weight, cfg.positive_score_loss_weight, cfg.negative_score_loss_weight, cfg.bbox_loss_weight)
    ds = IR.FlaggedDataset('deleted')
    # images 3 and 5 have no box: they stay out (n_obj = 0 is NaN on the unmasked path, as before)
    loader = TrainLoader(_Subset(ds, [0, 1, 2, 4, 6, 0]), cfg, seed=3, shuffle=False)
    steps = 0
    for batch in loader:
        batch = tr._to_device(batch)
        assert 'gt_ignore' not in batch and isinstance(batch['gt_sparse'], ops.SparseGT)
        mean, parts = m.forward_mean(batch)
        pred = m.base(batch['image']).detach()
        losses, nobj, mean4 = ops.loss_sparse_mean_fwd(pred, batch['gt_sparse'], m.loss.resolver.anchors_on(pred.device), (70, 100), 3, weights)
        assert torch.equal(_bits(parts['loss']), _bits(losses[3])) and torch.equal(_bits(mean.detach()), _bits(mean4[3]))
        values, _ = tr._iteration(batch, True)
        assert all(np.isfinite(v) for v in values)
        steps += 1
    assert steps == 2 and not any(calls.values())


class _Subset:
    def __init__(self, ds, idx):
        self.ds, self.idx = ds, idx
        self.rgb_mean, self.rgb_std = ds.rgb_mean, ds.rgb_std

    def __len__(self):
        return len(self.idx)

    def image_size(self, i):
        return self.ds.image_size(self.idx[i])

    def load_image(self, i):
        return self.ds.load_image(self.idx[i])

    def load_annotations(self, i):
        return self.ds.load_annotations(self.idx[i])


def test_plan_equals_launches_with_ignore_regions():
    from squeezedet_pytorch_amd import plan
    C, size, B = 20, (64, 96), 2
    cfg = sqd.make_cfg(input_size=size, num_classes=C)
    t = _model(cfg, C)
    x = synthetic.make_images(B, size, seed=0).cuda()
    gt = synthetic.make_gt(B, cfg.anchors, size, num_classes=C, seed=1).cuda()
    bm = torch.zeros(B, ops.ignore_words(cfg.num_anchors), dtype=torch.int32, device='cuda')
    batch = {'image': x, 'gt_sparse': ops.sparse_gt_from_dense(gt), 'gt_ignore': bm}

    def step():
        mean, _ = t.forward_mean(batch)
        t.zero_grad()
        mean.backward()
    step()
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        step()
    finally:
        ops.set_timer(None)
    torch.cuda.synchronize()
    got = [(r[0], r[1]) for r in timer.records]
    assert got == plan.training_launch_plan('squeezedet', B, size, num_classes=C, sparse_gt=True, ignore_regions=True)
    assert ('loss_masked_fwd', f'loss A{cfg.num_anchors}') in got and ('loss_masked_bwd', f'lossbwd A{cfg.num_anchors}') in got
