"""GPU tier of the IoU-family box regression: the loss launches with the box-loss kind 'iou' | 'giou' | 'diou' | 'ciou' behind their weights, called directly
on the crafted operands of tests/test_fp64_loss_gpu.py (clamp bounds, min / max ties, touching and disjoint boxes, saturated logits and
deltas, a ragged last slice) plus two constructions of tests/iou_loss_ref.py, in every ground-truth form -- dense (3 classes: the
<= 16-class kernels; 20: the many-class ones), sparse, masked -- and for both upstream forms, held to the float64 twin of
tests/iou_loss_ref.py element by element.

Every output holds bar L (|err| <= 2^-18 M); counts are exact; the plain and the mean forward are bitwise equal per image; at most
MAX_FLIPS anchors per launch may sit on a branch where float32 and float64 disagree (the operands have none); sparse and dense are
held to the same reference; the masked conventions of tests/test_ignore_gpu.py hold; SQD_BOX_L2 through the six new entries gives
the bits of the old ones; the gt delta columns are not read; an unknown kind raises before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ref as R  # noqa: E402
import ignore_ref as IR  # noqa: E402
import iou_loss_ref as Q  # noqa: E402
import test_fp64_loss_gpu as LG  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = [('dense', 3), ('dense', 20), ('sparse', 3), ('sparse', 20)]
CASE_NAMES = ('edges', 'saturated', 'random')
_CASES, _REFS = {}, {}


def _case(name, C):
    if C not in _CASES:
        _CASES[C] = dict(Q.cases(LG, C))
    return _CASES[C][name]


def _ref(name, C, kind):
    """One reference per operand set and kind, shared by the dense and the sparse form."""
    key = (name, C, kind)
    if key not in _REFS:
        pred, gt, anchors = _case(name, C)
        _REFS[key] = Q.loss(pred, gt, anchors, LG.SIZE, C, LG.WEIGHTS, kind, gmean=LG.GMEAN, coef=LG.make_coef(pred.shape[0], 3))
    return _REFS[key]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _gm():
    return torch.tensor([LG.GMEAN], dtype=torch.float32, device='cuda')


def launch(form, pred, gt, anchors, C, kind, ign=None, coef=None, nan_out=False):
    """The four launches of one form through ops -> (losses, counts, losses of the mean form, counts of it, mean4, dmean, dcoef) on the
    device.  ``gt``: the dense tensor (the list forms take ``ops.sparse_gt_from_dense`` of it); ``ign``: the device bitmap."""
    from squeezedet_pytorch_amd import ops
    B = pred.shape[0]
    coef = (LG.make_coef(B, 3) if coef is None else coef).cuda()
    p, a, g = pred.cuda(), anchors.cuda(), gt.cuda()
    w = LG.WEIGHTS + (kind,)                                    # (ops.split_loss_weights: the kind rides behind the four weights)
    if form == 'dense':
        fwd, mfwd, bwd, mbwd = ops.loss_fns(C)
        losses, n = fwd(p, g, a, LG.SIZE, C, w)
        losses_m, n_m, mean4 = mfwd(p, g, a, LG.SIZE, C, w)
        dm = mbwd(p, g, a, n_m, _gm(), LG.SIZE, C, w)
        dc = bwd(p, g, a, n, coef, LG.SIZE, C, w)
    elif form == 'sparse':
        sgt = ops.sparse_gt_from_dense(g)
        losses, n = ops.loss_sparse_fwd(p, sgt, a, LG.SIZE, C, w)
        losses_m, n_m, mean4 = ops.loss_sparse_mean_fwd(p, sgt, a, LG.SIZE, C, w)
        dm = ops.loss_sparse_mean_bwd(p, sgt, a, n_m, _gm(), LG.SIZE, C, w)
        dc = ops.loss_sparse_bwd(p, sgt, a, n, coef, LG.SIZE, C, w)
    else:
        sgt = ops.sparse_gt_from_dense(g)
        out = (lambda: torch.full_like(p, float('nan'))) if nan_out else (lambda: None)
        losses, n = ops.loss_masked_fwd(p, sgt, ign, a, LG.SIZE, C, w)
        losses_m, n_m, mean4 = ops.loss_masked_mean_fwd(p, sgt, ign, a, LG.SIZE, C, w)
        dm = ops.loss_masked_mean_bwd(p, sgt, ign, a, n_m, _gm(), LG.SIZE, C, w, out=out())
        dc = ops.loss_masked_bwd(p, sgt, ign, a, n, coef, LG.SIZE, C, w, out=out())
    torch.cuda.synchronize()
    return losses, n, losses_m, n_m, mean4, dm, dc


def check(tag, outs, ref, counts):
    """Bitwise agreement of the two forward forms, exact counts, bar L on losses / mean4 / dmean / dcoef, the flip cap."""
    losses, n, losses_m, n_m, mean4, dm, dc = outs
    assert torch.equal(_bits(losses), _bits(losses_m)) and torch.equal(_bits(n), _bits(n_m)), f'{tag}: plain and mean forward differ'
    assert torch.equal(n.cpu().double(), counts), f'{tag}: counts are not exact'
    flips = int(ref['flips'].sum())
    res = {'losses': R.bars_nan(losses.cpu(), ref['losses'], 'vec', 2), 'mean4': R.bars_nan(mean4.cpu(), ref['mean4'], 'vec', 2)}
    for name, got in (('dmean', dm.cpu()), ('dcoef', dc.cpu())):
        res[name] = R.bars_nan(got, R.pick(got, ref[name], ref[name + '_alt'], ref['flips']), 'dpred', 2)
    for k, b in res.items():
        print(f'box loss {tag:40s} {k:6s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e}) NaN positions ok={b["nan_ok"]} flips {flips}')
    assert all(b['l_ok'] for b in res.values()), (tag, {k: b for k, b in res.items() if not b['l_ok']})
    assert flips <= LG.MAX_FLIPS, (tag, flips)


@pytest.mark.parametrize('kind', Q.KINDS)
@pytest.mark.parametrize('form,C', FORMS, ids=[f'{f}-C{c}' for f, c in FORMS])
def test_against_the_float64_twin(form, C, kind):
    for name in CASE_NAMES:
        pred, gt, anchors = _case(name, C)
        ref = _ref(name, C, kind)
        assert int(ref['flips'].sum()) == 0                       # (exact constructions and well-separated random boxes)
        check(f'{kind} {form} C{C} {name}', launch(form, pred, gt, anchors, C, kind), ref, ref['nobj'])


def _dev_bitmap(ign):
    from squeezedet_pytorch_amd import boxes
    return torch.from_numpy(boxes.pack_ignore_bits(np.asarray(ign))).cuda()


@pytest.mark.parametrize('kind', Q.KINDS)
def test_masked_against_the_float64_twin(kind):
    """``ignore_ref.case_with_ignore``: an image with positives and a bitmap that covers some of them, an image without any object, an
    image of positives with every other anchor ignored, an image with every anchor ignored; then the edge constructions under a
    bitmap.  The conventions of tests/test_ignore_gpu.py: finite everywhere, ignored rows +0.0 bit for bit in a NaN-filled dpred,
    class = bbox = 0 without an object, all zeros without an object or a negative."""
    A, C = 200, 3
    pred, gt, anchors, ign = IR.case_with_ignore(LG, A, C, seed=41, density=0.3)
    ref = Q.masked_loss(kind, pred, gt, ign, anchors, LG.SIZE, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=LG.make_coef(4, 3))
    outs = launch('masked', pred, gt, anchors, C, kind, ign=_dev_bitmap(ign), nan_out=True)
    check(f'{kind} masked A{A}', outs, ref, ref['counts'])
    losses, _, _, _, mean4, dm, dc = (t.cpu() for t in outs)
    for t in (losses, mean4, dm, dc):
        assert torch.isfinite(t).all(), 'a masked launch left a NaN / an unwritten element'
    for got in (dm, dc):
        assert bool((_bits(got)[ref['ign']] == 0).all()), 'an ignored row is not +0.0 bit for bit'
    assert ref['counts'][0].tolist()[1::2] == [0.0, 0.0] and ref['counts'][1].tolist()[2:] == [0.0, 0.0]
    assert torch.equal(_bits(losses[[0, 2]][:, [1, 3]]), torch.zeros(2, 2, dtype=torch.int32))           # n_obj = 0: class = bbox = 0
    assert float(losses[1, 1]) == float(losses[3, 1])                                                     # ... and pos = 0: score = total
    assert torch.equal(_bits(losses[:, 3]), torch.zeros(4, dtype=torch.int32))                            # nothing left: losses == 0
    assert torch.equal(_bits(dm[3]), torch.zeros_like(_bits(dm[3]))) and torch.equal(_bits(dc[3]), torch.zeros_like(_bits(dc[3])))
    first = int(torch.nonzero(gt[0, :, 0] > 0)[0])
    assert ign[0, first] and bool((dm[0, first] != 0).any())                                              # a positive wins over its own bit
    pred, gt, anchors = _case('edges', C)
    ign = np.random.RandomState(9).rand(2, pred.shape[1]) < 0.3
    ref = Q.masked_loss(kind, pred, gt, ign, anchors, LG.SIZE, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=LG.make_coef(2, 3))
    assert int(ref['flips'].sum()) == 0
    check(f'{kind} masked edges', launch('masked', pred, gt, anchors, C, kind, ign=_dev_bitmap(ign)), ref, ref['counts'])


# ---- the raw entries ----

def _raw(form, box, pred, gt, anchors, C, ign=None, coef=None, old=False):
    """The launches of one form through the C ABI: the six sqd_loss_box_* entries with the kind ``box``, or (``old``) the sixteen
    entries they stand beside.  -> [losses, counts, losses (mean form), counts, mean4, dmean, dcoef]."""
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd import ops
    lib = nat.lib()
    B, A = pred.shape[:2]
    p, a, g = pred.cuda().contiguous(), anchors.cuda().contiguous(), gt.cuda().contiguous()
    coef = (LG.make_coef(B, 3) if coef is None else coef).cuda().contiguous()
    gm = _gm()
    masked = form == 'masked'
    if form == 'dense':
        mid, lead, stem = [g], (), ('many_' if C > 16 else '')
    else:
        sgt = ops.sparse_gt_from_dense(g)
        mid, lead, stem = list(sgt) + ([ign] if masked else []), (int(sgt.anchor_idx.shape[0]),), form + '_'
    tail = (*lead, B, A, C, LG.SIZE[0], LG.SIZE[1], *[float(w) for w in LG.WEIGHTS], nat.stream_handle(p.device))
    ptrs = lambda *ts: [nat.ptr(t) for t in ts]                # noqa: E731
    ws = torch.empty(B * 16 * (6 if masked else 5), device='cuda')
    new = lambda: (torch.empty(4, B, device='cuda'), torch.empty(*((2,) if masked else ()), B, device='cuda'))      # noqa: E731
    box_name = 'sqd_loss_box_' + ('' if form == 'dense' else stem)
    (l0, n0), (l1, n1), mean4 = new(), new(), torch.empty(4, device='cuda')
    dm, dc = torch.empty_like(p), torch.empty_like(p)
    if old:
        calls = [(f'sqd_loss_{stem}fwd', ptrs(p, *mid, a, ws, l0, n0)), (f'sqd_loss_{stem}mean_fwd', ptrs(p, *mid, a, ws, l1, n1, mean4)),
                 (f'sqd_loss_{stem}mean_bwd', ptrs(p, *mid, a, n1, gm, dm)), (f'sqd_loss_{stem}bwd', ptrs(p, *mid, a, n0, coef, dc))]
    else:
        calls = [(box_name + 'fwd', ptrs(p, *mid, a, ws, l0, n0, None) + [box]), (box_name + 'fwd', ptrs(p, *mid, a, ws, l1, n1, mean4) + [box]),
                 (box_name + 'bwd', ptrs(p, *mid, a, n1, None, gm, dm) + [box]), (box_name + 'bwd', ptrs(p, *mid, a, n0, coef, None, dc) + [box])]
    for entry, args in calls:
        nat.check(getattr(lib, entry)(*args, *tail), entry)
    torch.cuda.synchronize()
    return [l0, n0, l1, n1, mean4, dm, dc]


@pytest.mark.parametrize('form,C', FORMS + [('masked', 3), ('masked', 20)], ids=[f'{f}-C{c}' for f, c in FORMS + [('masked', 3), ('masked', 20)]])
def test_l2_through_the_new_entries_is_the_old_launch(form, C):
    """SQD_BOX_L2: losses, counts, mean4 and dpred of the new entries equal the old entries' bit for bit (NaN rows included: the
    masked case has an image without an object)."""
    if form == 'masked':
        pred, gt, anchors, ign = IR.case_with_ignore(LG, 200, C, seed=43, density=0.3)
        ign = _dev_bitmap(ign)
    else:
        (pred, gt, anchors), ign = LG.random_case(3, 200, C, seed=77, nobj=[9, 0, 31]), None
    for x, y in zip(_raw(form, 0, pred, gt, anchors, C, ign), _raw(form, 0, pred, gt, anchors, C, ign, old=True)):
        assert torch.equal(_bits(x), _bits(y)), (form, C)


@pytest.mark.parametrize('kind', Q.KINDS)
def test_raw_entries_equal_ops_and_gt_deltas_are_not_read(kind):
    """The raw entries give what ops gives; filling the gt delta columns (dense 5..8, the list's ``deltas``) with NaN changes no bit
    of any output of any form."""
    from squeezedet_pytorch_amd import ops
    box = ops.BOX_LOSSES.index(kind)
    for form, C in FORMS + [('masked', 3)]:
        pred, gt, anchors = _case('random', C)
        ign = _dev_bitmap(np.random.RandomState(3).rand(pred.shape[0], pred.shape[1]) < 0.3) if form == 'masked' else None
        want = launch(form, pred, gt, anchors, C, kind, ign=ign)
        poisoned = gt.clone()
        poisoned[..., 5:9] = float('nan')
        for tag, got in (('raw', _raw(form, box, pred, gt, anchors, C, ign)), ('NaN deltas', launch(form, pred, poisoned, anchors, C, kind, ign=ign)),
                         ('raw, NaN deltas', _raw(form, box, pred, poisoned, anchors, C, ign))):
            for i, (x, y) in enumerate(zip(got, want)):
                assert torch.equal(_bits(x), _bits(y)), (kind, form, C, tag, i)
            assert all(torch.isfinite(t).all() for t in got), (kind, form, C, tag)


def test_unknown_kind_raises_before_any_launch(monkeypatch):
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd import ops
    pred, gt, anchors = _case('random', 3)
    p, g, a = pred.cuda(), gt.cuda(), anchors.cuda()
    sgt = ops.sparse_gt_from_dense(g)
    bm = torch.zeros(p.shape[0], ops.ignore_words(p.shape[1]), dtype=torch.int32, device='cuda')
    n, coef = torch.ones(p.shape[0], device='cuda'), LG.make_coef(p.shape[0], 3).cuda()
    counts = torch.ones(2, p.shape[0], device='cuda')

    def no_library():
        raise AssertionError('the library was reached')
    monkeypatch.setattr(nat, 'lib', no_library)
    tail = lambda k: (LG.SIZE, 3, LG.WEIGHTS + (k,))          # noqa: E731
    calls = [lambda k: ops.loss_fwd(p, g, a, *tail(k)), lambda k: ops.loss_mean_fwd(p, g, a, *tail(k)),
             lambda k: ops.loss_bwd(p, g, a, n, coef, *tail(k)), lambda k: ops.loss_mean_bwd(p, g, a, n, _gm(), *tail(k)),
             lambda k: ops.loss_fwd_many(p, g, a, *tail(k)), lambda k: ops.loss_bwd_many(p, g, a, n, coef, *tail(k)),
             lambda k: ops.loss_sparse_fwd(p, sgt, a, *tail(k)), lambda k: ops.loss_sparse_mean_fwd(p, sgt, a, *tail(k)),
             lambda k: ops.loss_sparse_bwd(p, sgt, a, n, coef, *tail(k)),
             lambda k: ops.loss_sparse_mean_bwd(p, sgt, a, n, _gm(), *tail(k)),
             lambda k: ops.loss_masked_fwd(p, sgt, bm, a, *tail(k)), lambda k: ops.loss_masked_mean_fwd(p, sgt, bm, a, *tail(k)),
             lambda k: ops.loss_masked_bwd(p, sgt, bm, a, counts, coef, *tail(k)),
             lambda k: ops.loss_masked_mean_bwd(p, sgt, bm, a, counts, _gm(), *tail(k))]
    for call in calls:
        for bad in ('huber', 'GIOU', 2, None):
            with pytest.raises(ValueError, match='box_loss'):
                call(bad)
        with pytest.raises(ValueError, match='weights must be'):
            ops.split_loss_weights('x', LG.WEIGHTS[:3])
