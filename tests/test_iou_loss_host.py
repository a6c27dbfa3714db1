"""CPU tier of the IoU-family box regression (``cfg.bbox_loss``): the float64 twin of tests/iou_loss_ref.py against hand-derived
values and against ``oracle.multitask_loss``, its analytic chain against float64 autograd, the attainability of bar L in float32,
the teeth of the conventions the GPU tests pin, and the configuration field.  No GPU call is made."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ref as R  # noqa: E402
import iou_loss_ref as Q  # noqa: E402
import oracle  # noqa: E402
import test_fp64_loss_gpu as LG  # noqa: E402

F64 = torch.float64
CASES = Q.cases(LG)
_REFS = {}


def _ref(name, kind, mutant=None):
    key = (name, kind, mutant)
    if key not in _REFS:
        pred, gt, anchors = dict(CASES)[name]
        _REFS[key] = Q.loss(pred, gt, anchors, LG.SIZE, 3, LG.WEIGHTS, kind, gmean=LG.GMEAN, coef=LG.make_coef(pred.shape[0], 3),
                            mutant=mutant)
    return _REFS[key]


def _one_minus_q(g, p, kind):
    return float(1 - Q.box_q(torch.tensor([g], dtype=F64), torch.tensor([p], dtype=F64), kind)[0])


def test_hand_derived_values():
    """g = (0,0,10,10), p = (20,0,30,10): disjoint, the enclosing box is 30 x 10, the centres are 20 apart, the aspect ratios agree:
    iou = 0; giou: (300 - 200) / 300 = 1/3; diou and ciou: 400 / (900 + 100) = 0.4, v = 0."""
    g, p = (0., 0., 10., 10.), (20., 0., 30., 10.)
    assert _one_minus_q(g, p, 'iou') == 1.0
    assert abs(_one_minus_q(g, p, 'giou') - 4.0 / 3.0) <= 1e-12
    assert abs(_one_minus_q(g, p, 'diou') - 1.4) <= 1e-12
    assert abs(_one_minus_q(g, p, 'ciou') - 1.4) <= 1e-12
    # p == g: every penalty is 0 and 1 - iou = eps / (area + eps) <= eps / area; 2^-52 is the rounding of 1 - iou near 1
    for box in ((0., 0., 1., 1.), (0., 0., 10., 10.), (3., 4., 7.5, 40.)):
        for kind in Q.KINDS:
            v = _one_minus_q(box, box, kind)
            assert 0.0 <= v <= 1e-10 + 2.0 ** -52, (box, kind, v)


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_l2_twin_is_the_oracle(name):
    pred, gt, anchors = dict(CASES)[name]
    an = anchors.numpy()
    for dtype in (torch.float32, F64):
        lv, st = Q.twin(pred.to(dtype), gt.to(dtype), an, LG.SIZE, 3, LG.WEIGHTS, 'l2')
        lo, so = oracle.multitask_loss(pred.to(dtype), gt.to(dtype), an, LG.SIZE, 3, *LG.WEIGHTS)
        assert torch.equal(lv, lo) and all(torch.equal(st[k], so[k]) for k in so)


@pytest.mark.parametrize('kind', Q.KINDS)
@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_chain_matches_autograd_and_float32_attains_the_bar(name, kind):
    """On the operands of the GPU tests: every reference is finite, no anchor flips a branch between float32 and float64, the analytic
    chain (where M comes from) equals float64 autograd of the twin within bar L, and the twin in float32 holds bar L: a correct
    float32 kernel can."""
    ref = _ref(name, kind)
    assert int(ref['flips'].sum()) == 0
    for out in ('losses', 'mean4', 'dmean', 'dcoef'):
        r = ref[out]
        assert torch.isfinite(r.ref64).all() and torch.isfinite(r.b32).all() and torch.isfinite(r.M).all(), (name, kind, out)
        b = R.bars(r.b32, r, 'dpred' if out[0] == 'd' else 'vec', 2)
        print(f'{name:10s} {kind:5s} {out:7s} float32 twin max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e})')
        assert b['l_ok'], (name, kind, out, b)
    for out in ('losses', 'dmean', 'dcoef'):
        r, c = ref[out], ref[out + '_chain']
        err = (c.v - r.ref64).abs()
        assert bool((err <= R.BAR_L * r.M).all()), (name, kind, out, float((err / r.M.clamp_min(1e-300)).max()))
        assert bool((err <= 1e-12 * (c.m + r.ref64.abs())).all()), (name, kind, out)      # (in fact to float64 rounding)


def test_iou_has_no_box_gradient_for_disjoint_boxes():
    """The property the other three kinds exist to fix: with w_pos = 0 (no score path) a disjoint positive's deltas get a zero
    gradient under 'iou' and a non-zero one under giou / diou / ciou."""
    pred, gt, anchors = dict(CASES)['edges']
    far = len(LG.EDGES) + 1                                   # image 0, the x construction 'far_disjoint'
    assert list(Q.EXTRA_EDGES)[1] == 'far_disjoint'
    w = (1.0, 0.0, 100.0, 6.0)
    for kind in Q.KINDS:
        _, dm, _ = Q.twin_grads(pred, gt, anchors, LG.SIZE, 3, w, kind, F64, gmean=1.0)
        g = dm[0, far, 4:]
        assert bool((g == 0).all()) if kind == 'iou' else bool((g != 0).any()), (kind, g)


MUTANT_KIND = {'alpha_attached': ('ciou',), 'enclose_no_tie_split': ('giou', 'diou', 'ciou'), 'penalty_detached': ('giou', 'diou', 'ciou'),
               'l2_term_added': Q.KINDS}


@pytest.mark.parametrize('mutant', Q.TWIN_MUTANTS)
def test_wrong_conventions_fail_the_cases(mutant):
    """Teeth of the GPU tests: a kernel with alpha left in the graph, with the enclosing box's ties given to one side, with the penalty
    detached (the IoU part's gradient only) or with the squared error on the deltas still added moves some element of these operands
    beyond bar L -- for every kind the convention concerns.  The twin under that convention stands in for the kernel."""
    for kind in MUTANT_KIND[mutant]:
        moved = []
        for name, _ in CASES:
            ref, mut = _ref(name, kind), _ref(name, kind, mutant)
            for out in ('losses', 'dmean', 'dcoef'):
                if not R.bars(mut[out].ref64, ref[out], 'dpred' if out[0] == 'd' else 'vec', 2)['l_ok']:
                    moved.append((name, out))
        print(mutant, kind, moved)
        assert moved, f'{mutant} / {kind}: no case tells it from the pinned convention'
        if mutant == 'enclose_no_tie_split':
            assert ('edges', 'dmean') in moved


def test_cfg_field():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd.model import Loss
    from squeezedet_pytorch_amd.trainer import step_signature
    cfg = sqd.make_cfg(device='cpu')
    assert cfg.bbox_loss == 'l2' and cfg.bbox_loss_weight == 6.0 and Loss(cfg).bbox_loss == 'l2'
    for kind in ('l2',) + Q.KINDS:
        assert Loss(sqd.make_cfg(device='cpu', bbox_loss=kind)).bbox_loss == kind
    for bad in ('huber', 'GIoU', None, 2):
        with pytest.raises(ValueError, match='bbox_loss'):
            sqd.make_cfg(device='cpu', bbox_loss=bad)
    cfg.bbox_loss = 'huber'
    with pytest.raises(ValueError, match='bbox_loss'):
        Loss(cfg)
    delattr(cfg, 'bbox_loss')                                 # a reference cfg has no such field
    assert Loss(cfg).bbox_loss == 'l2'
    sig = dict(image_shape=(2, 64, 96), form='dense', cap=0, training=True, trainable=('a',), clip_on=True, loss_weights=(1., 3.75, 100., 6.))
    assert step_signature(**sig) == step_signature(**sig, bbox_loss='l2') != step_signature(**sig, bbox_loss='giou')


def test_entry_points_refuse_without_gpu():
    """The six sqd_loss_box_* entries validate before any launch: an unknown kind, both or neither of coef / gmean, a null operand,
    and the limits of the entries they stand beside (257 classes, 2^20 + 1 anchors for the list forms)."""
    import ctypes
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd import ops
    lib = nat.lib()
    null, some = ctypes.c_void_p(0), ctypes.c_void_p(4096)     # never dereferenced
    w = (1.0, 3.75, 100.0, 6.0)
    assert ops.BOX_LOSSES == ('l2', 'iou', 'giou', 'diou', 'ciou')
    for name in ('fwd', 'bwd', 'sparse_fwd', 'sparse_bwd', 'masked_fwd', 'masked_bwd'):
        assert 'sqd_loss_box_' + name in nat._SIGNATURES
    dims = (2, 64, 3, 64, 96)
    for kind in (-1, 5, 99):
        assert lib.sqd_loss_box_fwd(*[some] * 7, kind, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_bwd(*[some] * 4, some, null, some, kind, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_sparse_fwd(*[some] * 11, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_sparse_bwd(*[some] * 8, some, null, some, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_masked_fwd(*[some] * 12, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_masked_bwd(*[some] * 9, some, null, some, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG
    for kind in range(5):
        for coef, gmean in ((some, some), (null, null)):
            assert lib.sqd_loss_box_bwd(*[some] * 4, coef, gmean, some, kind, *dims, *w, null) == nat.ERR_BAD_ARG
            assert lib.sqd_loss_box_sparse_bwd(*[some] * 8, coef, gmean, some, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG
            assert lib.sqd_loss_box_masked_bwd(*[some] * 9, coef, gmean, some, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_fwd(null, *[some] * 6, kind, *dims, *w, null) == nat.ERR_BAD_ARG
        assert lib.sqd_loss_box_masked_fwd(*[some] * 6, null, *[some] * 5, kind, 4, *dims, *w, null) == nat.ERR_BAD_ARG      # the bitmap
        assert lib.sqd_loss_box_fwd(*[some] * 7, kind, 2, 64, 257, 64, 96, *w, null) == nat.ERR_UNSUPPORTED
        assert lib.sqd_loss_box_bwd(*[some] * 4, some, null, some, kind, 2, 64, 257, 64, 96, *w, null) == nat.ERR_UNSUPPORTED
        assert lib.sqd_loss_box_sparse_fwd(*[some] * 11, kind, 4, 2, 2 ** 20 + 1, 3, 64, 96, *w, null) == nat.ERR_UNSUPPORTED
        assert lib.sqd_loss_box_masked_bwd(*[some] * 9, some, null, some, kind, 4, 2, 64, 257, 64, 96, *w, null) == nat.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match='box_loss'):
        ops.box_loss_kind('loss_fwd', 'huber')
    assert [ops.box_loss_kind('x', k) for k in ops.BOX_LOSSES] == [0, 1, 2, 3, 4]
    # the kind rides behind the four weights of every loss_* wrapper; four weights alone are 'l2'
    assert ops.split_loss_weights('x', w) == (w, 0) and ops.split_loss_weights('x', list(w) + ['ciou']) == (w, 4)
    for bad in (w[:3], w + ('giou', 1.0), w + ('huber',), w + (2,)):
        with pytest.raises(ValueError, match='weights must be|box_loss'):
            ops.split_loss_weights('x', bad)
