"""CPU tier of the ignore regions: the host rule ``boxes.anchor_ignore_mask`` on hand-checkable cases, the float64 reference of the
masked loss (tests/ignore_ref.py) against float64 autograd of a plain torch statement, ``TrainLoader.plan()`` with flagged boxes, the
``ValueError``s of the new configuration field, and the planner."""
import numpy as np
import pytest
import torch

import fp64_ref as R
import ignore_ref as IR
import oracle
from oracle import squeezedet_oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import annotations, augment, boxes, ops, plan
from squeezedet_pytorch_amd.train_data import TrainLoader
import test_fp64_loss_gpu as LG


@pytest.mark.parametrize('case', IR.boundary_cases(), ids=lambda c: c[0])
def test_host_rule_by_hand(case):
    _, anchors, regions, overlap, want = case
    assert boxes.anchor_ignore_mask(anchors, regions, overlap).tolist() == want


def test_bit_layout():
    m = np.zeros((2, 70), bool)
    m[0, [0, 31, 32, 69]] = True
    w = boxes.pack_ignore_bits(m)
    assert w.dtype == np.int32 and w.shape == (2, 3)
    assert w[0].view(np.uint32).tolist() == [0x80000001, 1, 1 << 5] and w[1].tolist() == [0, 0, 0]
    assert np.array_equal(boxes.unpack_ignore_bits(w, 70), m)


def torch_masked_loss(pred, gt, ign, anchors, size, C, weights):
    """The masked loss as mask tensors and its three conventions written out (any dtype; differentiable in pred).
    -> (total [B], (class, score, bbox) each [B])."""
    w_c, w_p, w_n, w_b = (float(torch.tensor(w, dtype=torch.float32)) for w in weights)
    dt = pred.dtype
    mask = gt[..., :1].to(dt)
    ignm = (ign & ~(gt[..., 0] > 0)).to(dt).unsqueeze(-1)          # a positive wins over its own bit
    negm = (1 - mask) * (1 - ignm)
    _, logp, scores, deltas, bx = oracle.resolve_predictions(pred, anchors.float().numpy(), tuple(size), C, log_softmax=True)
    n_obj, n_neg = mask.sum(dim=[1, 2]), negm.sum(dim=[1, 2])
    iou = squeezedet_oracle._overlaps(gt[..., 1:5].to(dt), bx) * mask

    def over(s, n):                                                # s / n, and 0 where there is nothing to divide by
        return torch.where(n > 0, s / n.clamp_min(1), torch.zeros_like(s))
    cls = over((w_c * mask * gt[..., 9:].to(dt) * (-logp)).sum(dim=[1, 2]), n_obj)
    pos = over((w_p * mask * (iou - scores) ** 2).sum(dim=[1, 2]), n_obj)
    neg = over((w_n * negm * (iou - scores) ** 2).sum(dim=[1, 2]), n_neg)
    bbx = over((w_b * mask * (deltas - gt[..., 5:9].to(dt)) ** 2).sum(dim=[1, 2]), n_obj)
    return cls + pos + neg + bbx, (cls, pos + neg, bbx)


@pytest.mark.parametrize('C', [1, 3, 17])
@pytest.mark.parametrize('A', [1, 33, 517])
def test_reference_against_autograd(A, C):
    pred, gt, anchors, ign = IR.case_with_ignore(LG, A, C, seed=900 + A + C, density=0.3)
    B = pred.shape[0]
    coef = LG.make_coef(B, 5)
    ref = IR.masked_loss(pred, gt, ign, anchors, LG.SIZE, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=coef)
    ignt = torch.from_numpy(ign)
    pos = gt[..., 0] > 0
    assert ref['counts'][0].tolist() == pos.sum(1).tolist()
    assert ref['counts'][1].tolist() == (~pos & ~ignt).sum(1).tolist()
    assert ref['counts'][0, 1] == 0 and ref['counts'][1, 2] == 0 and ref['counts'][:, 3].tolist() == [0, 0]    # the kinds of image
    p = pred.double().requires_grad_(True)
    total, parts = torch_masked_loss(p, gt, ignt, anchors, LG.SIZE, C, LG.WEIGHTS)
    want = torch.stack([*parts, total]).detach()
    assert torch.isfinite(want).all()
    tol = lambda t: 1e-11 * t.abs().max().clamp_min(1e-30)          # noqa: E731  (two float64 evaluations of one expression)
    assert (ref['losses'].ref64 - want).abs().max() <= tol(want)
    assert (ref['mean4'].ref64 - want.mean(1)).abs().max() <= tol(want)
    gm = float(np.float32(LG.GMEAN) / np.float32(B))
    (g_mean,) = torch.autograd.grad(total.sum() * gm, p, retain_graph=True)
    cf = coef.double()
    (g_coef,) = torch.autograd.grad((cf[0] * parts[0] + cf[1] * parts[1] + cf[2] * parts[2]).sum(), p)
    for name, g in (('dmean', g_mean), ('dcoef', g_coef)):
        assert torch.isfinite(g).all()
        assert (ref[name].ref64 - g).abs().max() <= tol(g), name
        assert bool((ref[name].M[ref['ign']] == 0).all()) and bool((g[ref['ign']] == 0).all())      # ignored rows: exact zeros
        assert R.bars(ref[name].ref64, ref[name], 'dpred', 2)['l_ok']
    # images 1 and 3 have no positives: class = bbox = 0 with M = 0; image 3 is all zeros
    assert ref['losses'].ref64[[0, 2]][:, [1, 3]].abs().max() == 0 and ref['losses'].M[[0, 2]][:, [1, 3]].abs().max() == 0
    assert ref['losses'].ref64[:, 3].abs().max() == 0 and ref['dmean'].ref64[3].abs().max() == 0
    assert ref['losses'].ref64[1, 1] > 0 if ref['counts'][1, 1] > 0 else True


_Dataset = IR.FlaggedDataset


def _cfg(**kw):
    cfg = sqd.make_cfg(input_size=(70, 100), **kw)
    cfg.batch_size, cfg.num_workers, cfg.drift_prob, cfg.flip_prob = 3, 0, 1.0, 0.5
    return cfg


@pytest.mark.parametrize('forbid_resize', [False, True])
def test_loader_plan_with_flagged_boxes(forbid_resize):
    cfg = _cfg(sparse_gt=True, ignore_overlap=0.5, forbid_resize=forbid_resize)
    plain = _cfg(forbid_resize=forbid_resize)
    flagged = list(TrainLoader(_Dataset('flags'), cfg, seed=3, drop_last=False).plan())
    dropped = list(TrainLoader(_Dataset('flags'), plain, seed=3, drop_last=False).plan())        # flags, feature off: dropped
    deleted = list(TrainLoader(_Dataset('deleted'), plain, seed=3, drop_last=False).plan())
    assert len(flagged) == len(deleted) == 3
    ds = _Dataset('flags')
    seen = 0
    for pf, pd, px in zip(flagged, dropped, deleted):
        assert set(px) == {'index', 'aug', 'boxes', 'metas', 'class_ids'} and set(pd) == set(px) and set(pf) == set(px) | {'ignore_boxes'}
        for q in (pf, pd):
            assert np.array_equal(q['index'], px['index']) and np.array_equal(q['aug'], px['aug'])
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(q['boxes'], px['boxes']))
            assert all(np.array_equal(a, b) for a, b in zip(q['class_ids'], px['class_ids']))
        for k, i in enumerate(pf['index']):
            _, b, f = ds.ann[int(i)]
            t, _ = augment.transform_boxes(b[f != 0], ds.SIZES[int(i)], pf['aug'][k], cfg.input_size, forbid_resize)
            t = np.array(t, np.float32)
            t[:, [0, 2]] = np.clip(t[:, [0, 2]], 0., 99.)
            t[:, [1, 3]] = np.clip(t[:, [1, 3]], 0., 69.)
            t = t[(t[:, 2] > t[:, 0]) & (t[:, 3] > t[:, 1])]
            assert np.array_equal(pf['ignore_boxes'][k], t) and pf['ignore_boxes'][k].dtype == np.float32
            seen += len(t)
            if int(i) in (3, 5):
                assert pf['boxes'][k].shape == (0, 4) and len(pf['class_ids'][k]) == 0
    assert seen > 0


def test_two_tuple_dataset_plans_as_before():
    """No flags, feature off: the draws are ``augment.draw_augmentation`` on the loader's RandomState and the boxes
    ``augment.transform_boxes``, restated by hand; the plan has the keys it had."""
    cfg = _cfg()
    ds = _Dataset('deleted')
    plans = list(TrainLoader(ds, cfg, seed=3, drop_last=False).plan())
    rng = np.random.RandomState(3)
    order = rng.permutation(len(ds))
    for k, p in enumerate(plans):
        idxs = order[3 * k:3 * k + 3]
        assert set(p) == {'index', 'aug', 'boxes', 'metas', 'class_ids'} and np.array_equal(p['index'], idxs)
        bl = [np.asarray(ds.load_annotations(int(i))[1], np.float32).reshape(-1, 4) for i in idxs]
        aug = augment.draw_augmentation(rng, [ds.SIZES[int(i)] for i in idxs], bl, 1.0, 0.5)
        assert np.array_equal(p['aug'], aug)
        for b, i, a, got in zip(bl, idxs, aug, p['boxes']):
            assert np.array_equal(got, augment.transform_boxes(b, ds.SIZES[int(i)], a, cfg.input_size, False)[0])


def test_value_errors():
    from squeezedet_pytorch_amd.trainer import encode_sparse_batch
    from squeezedet_pytorch_amd.model import Loss
    batch = {'image': torch.zeros(1, 3, 70, 100), 'gt_boxes': [np.array([[5, 5, 30, 30]], np.float32)], 'gt_class_ids': [np.array([0])]}
    with pytest.raises(ValueError, match='sparse_gt'):
        TrainLoader(_Dataset(), _cfg(ignore_overlap=0.5))
    with pytest.raises(ValueError, match='sparse_gt'):
        encode_sparse_batch(batch, _cfg(ignore_overlap=0.5))
    for bad in (0.0, -0.25, 1.5, float('nan'), float('inf'), 'half'):
        with pytest.raises(ValueError, match='ignore'):
            TrainLoader(_Dataset(), _cfg(sparse_gt=True, ignore_overlap=bad))
        with pytest.raises(ValueError, match='ignore'):
            encode_sparse_batch(batch, _cfg(sparse_gt=True, ignore_overlap=bad))
        with pytest.raises(ValueError):
            boxes.anchor_ignore_mask(np.array([[20., 20., 11., 11.]]), np.zeros((0, 4), np.float32), bad)
    assert sqd.make_cfg().ignore_overlap is None
    TrainLoader(_Dataset(), _cfg(sparse_gt=True, ignore_overlap=1.0))         # the closed end of (0, 1]
    TrainLoader(_Dataset(), _cfg(ignore_overlap=None))
    # a bitmap with a dense gt
    cfg = _cfg()
    loss = Loss(cfg)
    A, C = cfg.num_anchors, cfg.num_classes
    pred, gt, ign = torch.zeros(1, A, C + 5), torch.zeros(1, A, C + 9), torch.zeros(1, ops.ignore_words(A), dtype=torch.int32)
    with pytest.raises(ValueError, match='sparse'):
        loss(pred, gt, ign)
    with pytest.raises(ValueError, match='sparse'):
        loss.mean_loss(pred, gt, ign)
    with pytest.raises(ValueError):
        annotations.encode_annotations([np.array([0])], [np.array([[5, 5, 30, 30]], np.float32)], cfg.anchors, C, ignore_overlap=0.5)
    with pytest.raises(ValueError, match='dense'):
        annotations.encode_annotations([np.array([0])], [np.array([[5, 5, 30, 30]], np.float32)], cfg.anchors, C,
                                       ignore_boxes_list=[np.zeros((0, 4))], ignore_overlap=0.5)
    # operand checks of the new wrappers come before the library is touched
    with pytest.raises(ValueError, match='float64'):
        ops.anchor_ignore_mask(torch.zeros(0, 4), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 4), 0.5)
    with pytest.raises(ValueError, match='GPU'):
        ops.anchor_ignore_mask(torch.zeros(0, 4), torch.zeros(2, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.float64), 0.5)
    sgt = ops.sparse_gt_from_dense(torch.zeros(1, 40, 12))
    with pytest.raises(ValueError, match='ignore must be int32'):
        ops.loss_masked_fwd(torch.zeros(1, 40, 8), sgt, torch.zeros(1, 3, dtype=torch.int32), torch.zeros(40, 4), (64, 96), 3, LG.WEIGHTS)
    with pytest.raises(ValueError, match='ignore must be int32'):
        ops.loss_masked_fwd(torch.zeros(1, 40, 8), sgt, torch.zeros(1, 2), torch.zeros(40, 4), (64, 96), 3, LG.WEIGHTS)


def test_planner():
    kw = dict(arch='squeezedet', batch=2, input_size=(64, 96), num_classes=20)
    dense, sparse = plan.training_launch_plan(**kw), plan.training_launch_plan(sparse_gt=True, **kw)
    assert dense == plan.training_launch_plan(ignore_regions=False, **kw)
    assert sparse == plan.training_launch_plan(sparse_gt=True, ignore_regions=False, **kw)
    assert ('loss_fwd', 'loss A216') in dense and ('loss_bwd', 'lossbwd A216') in dense
    assert ('loss_sparse_fwd', 'loss A216') in sparse and ('loss_sparse_bwd', 'lossbwd A216') in sparse
    masked = plan.training_launch_plan(sparse_gt=True, ignore_regions=True, **kw)
    diff = [(a, b) for a, b in zip(sparse, masked) if a != b]
    assert len(masked) == len(sparse) and diff == [(('loss_sparse_fwd', 'loss A216'), ('loss_masked_fwd', 'loss A216')),
                                                   (('loss_sparse_bwd', 'lossbwd A216'), ('loss_masked_bwd', 'lossbwd A216'))]
    assert plan.training_launch_plan() == plan.training_launch_plan(ignore_regions=False)            # the benchmarked step
    with pytest.raises(ValueError):
        plan.training_launch_plan(ignore_regions=True, **kw)
