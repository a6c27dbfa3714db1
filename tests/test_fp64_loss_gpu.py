"""GPU tier: the loss launches (``sqd_loss_fwd``, ``sqd_loss_mean_fwd``, ``sqd_loss_bwd``, ``sqd_loss_mean_bwd``) called directly on
crafted operands and held to float64 (fp64_ref.loss) element by element: losses [4, B], mean4 [4], nobj [B] (exact) and dpred for both
upstream forms.  Anchors are integers with zero dw, dh where a case needs exact arithmetic, so the unclamped box lands exactly on a
clamp bound, a min / max tie or a touching edge in float32 and float64 alike: there the convention of torch 2.10's autograd (clamp
passes inclusively, ties split 0.5 / 0.5, clamp_min passes at 0) is pinned, and tests/test_fp64_coverage.py checks that each wrong
convention moves some element of these cases beyond bar L.  Fixed seeds, a fixed case list.

Every output holds bar L (|err| <= 2^-18 M, NaN positions equal to float64 autograd's); the per-image values of the two forward
forms are bitwise equal; at most 4 anchors per launch may take a branch on which float64 and float32 disagree (either branch's
reference is accepted there)."""
import numpy as np
import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu

SIZE = (64, 96)                       # (H, W): clamp bounds x <= 95, y <= 63
WEIGHTS = (1.0, 3.75, 100.0, 6.0)
GMEAN = 0.37
MAX_FLIPS = 4

# 1-D constructions along one axis (the other axis gets NEUTRAL): (anchor centre, anchor size, delta of the centre, delta of the size,
# gt lo, gt hi); ``hi`` stands for the clamp bound of the axis (95 for x, 63 for y).  Anchor sizes are odd: 0.5 (s - 1) is an integer.
NEUTRAL = (15, 11, 0.0, 0.0, 12.5, 25.25)
EDGES = {
    'lo_bound': (5, 11, 0.0, 0.0, 2.5, 14.25),                        # x1u == 0: the clamp passes
    'lo_out': (5, 11, -2.0 ** -20, 0.0, 2.5, 14.25),                   # x1u just below 0: cut
    'hi_bound': ('hi-5', 11, 0.0, 0.0, 'hi-14.25', 'hi-2.5'),          # x2u == bound: passes
    'hi_out': ('hi-5', 11, 2.0 ** -20, 0.0, 'hi-14.25', 'hi-2.5'),     # just above: cut
    'tie_hi': (25, 11, 0.0, 0.0, 23.5, 30.0),                          # px2 == gx2, unclamped
    'tie_lo': (25, 11, 0.0, 0.0, 20.0, 36.75),                         # px1 == gx1
    'touch_hi': (25, 11, 0.0, 0.0, 30.0, 41.5),                        # lr_raw == 0 (gt starts where the prediction ends)
    'touch_lo': (25, 11, 0.0, 0.0, 8.5, 20.0),
    'disjoint': (25, 11, 0.0, 0.0, 33.0, 44.0),
    'pred_in_gt': (25, 11, 0.0, 0.0, 15.5, 37.25),
    'gt_in_pred': (25, 11, 0.0, 0.0, 22.5, 27.75),
    'inverted': (25, 9, 0.0, -3.0, 20.0, 30.0),                        # w = 9 e^-3 < 1: x1u > x2u
    'zero_area_gt': (25, 11, 0.0, 0.0, 24.5, 24.5),
}


def _hi(v, bound):
    if isinstance(v, str):
        return float(bound) + float(v[2:])
    return float(v)


def _negatives(rs, B, A, C, anchors, W, H):
    """Random negatives everywhere: anchors (integer centres, odd sizes), predictions at the synthetic head's scales."""
    anchors[:, 0] = rs.randint(0, W, A)
    anchors[:, 1] = rs.randint(0, H, A)
    anchors[:, 2] = 2 * rs.randint(1, 20, A) + 1
    anchors[:, 3] = 2 * rs.randint(1, 20, A) + 1
    pred = np.empty((B, A, C + 5), np.float32)
    pred[..., :C] = rs.standard_normal((B, A, C)) * 2
    pred[..., C] = rs.standard_normal((B, A)) * 1.5 - 2
    pred[..., C + 1:] = rs.standard_normal((B, A, 4)) * 0.4
    return pred, np.zeros((B, A, C + 9), np.float32)


def _positive(rs, pred, gt, anchors, b, a, C, x, y, conf=0.3, cls=None):
    """Anchor a of image b: a positive with the 1-D constructions x and y (values already resolved)."""
    (cx, sx, dx, dsx, gx1, gx2), (cy, sy, dy, dsy, gy1, gy2) = x, y
    anchors[a] = (cx, cy, sx, sy)
    pred[b, a, C] = conf
    pred[b, a, C + 1:] = (dx, dy, dsx, dsy)
    c = rs.randint(C) if cls is None else cls
    gt[b, a, 0] = 1.0
    gt[b, a, 1:5] = (gx1, gy1, gx2, gy2)
    gt[b, a, 5:9] = rs.standard_normal(4) * 0.3
    gt[b, a, 9:] = 0.0
    gt[b, a, 9 + c] = 1.0


def _resolve(e, bound):
    return tuple(_hi(v, bound) if i in (0, 4, 5) else v for i, v in enumerate(e))


def edge_case(C=3, A=64, seed=7):
    """Image 0: every construction of EDGES along x, image 1: along y (anchors 0 .. 12 of the image), negatives elsewhere.
    -> (pred, gt, anchors) float32 CPU tensors."""
    H, W = SIZE
    rs = np.random.RandomState(seed)
    anchors = np.zeros((A, 4), np.float32)
    pred, gt = _negatives(rs, 2, A, C, anchors, W, H)
    for i, e in enumerate(EDGES.values()):
        _positive(rs, pred, gt, anchors, 0, i, C, _resolve(e, W - 1), NEUTRAL)
    # image 1 shares the anchors: its y constructions take anchors 13 .. 25
    for i, e in enumerate(EDGES.values()):
        _positive(rs, pred, gt, anchors, 1, len(EDGES) + i, C, NEUTRAL, _resolve(e, H - 1))
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(anchors)


def saturated_case(C=3, A=64, seed=8):
    """Class logits of +-80, conf logits of +-30 (float32's sigmoid gradient is 0) on positives and negatives, and dw / dh up to 80
    (exp still finite; the box is clamped on both sides)."""
    H, W = SIZE
    rs = np.random.RandomState(seed)
    anchors = np.zeros((A, 4), np.float32)
    pred, gt = _negatives(rs, 2, A, C, anchors, W, H)
    for b in range(2):
        for i in range(8):
            _positive(rs, pred, gt, anchors, b, i, C, _resolve(EDGES['pred_in_gt'], W - 1), NEUTRAL,
                      conf=(30.0, -30.0)[i % 2], cls=i % C)
            pred[b, i, :C] = -80.0
            pred[b, i, (i + i // 2) % C] = 80.0                    # the gt class at +80 or at -80
        for i, d in zip(range(8, 12), (20.0, 60.0, 80.0, -2.0)):
            _positive(rs, pred, gt, anchors, b, i, C, (25, 9, 0.1, d, 20.0, 30.0), (15, 11, -0.2, d / 2, 10.0, 22.0))
        pred[b, 12:20, C] = np.array([30.0, -30.0] * 4, np.float32)    # saturated negatives
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(anchors)


def random_case(B, A, C, seed, pos_frac=0.1, nobj=None):
    """Random anchors, predictions and positives (gt boxes near their anchor); ``nobj``: per-image positive counts (None: random,
    at least 1 and at most A - 1 where A > 1)."""
    H, W = SIZE
    rs = np.random.RandomState(seed)
    anchors = np.zeros((A, 4), np.float32)
    pred, gt = _negatives(rs, B, A, C, anchors, W, H)
    for b in range(B):
        if nobj is not None:
            n = nobj[b]
        else:
            n = min(max(1, int(rs.binomial(A, pos_frac))), max(A - 1, 1))
        for a in rs.permutation(A)[:n]:
            ax, ay, aw, ah = anchors[a]
            cx, cy = ax + rs.uniform(-4, 4), ay + rs.uniform(-4, 4)
            w, h = aw * np.exp(rs.uniform(-.5, .5)), ah * np.exp(rs.uniform(-.5, .5))
            gt[b, a, 0] = 1.0
            gt[b, a, 1:5] = (np.clip(cx - w / 2, 0, W - 1), np.clip(cy - h / 2, 0, H - 1),
                             np.clip(cx + w / 2, 0, W - 1), np.clip(cy + h / 2, 0, H - 1))
            gt[b, a, 5:9] = rs.standard_normal(4) * 0.3
            gt[b, a, 9 + rs.randint(C)] = 1.0
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(anchors)


def make_coef(B, seed):
    """[3, B] upstream gradients: distinct per image and component, with zero and negative entries."""
    rs = np.random.RandomState(seed)
    c = rs.uniform(0.25, 2.0, (3, B)).astype(np.float32)
    c[:, ::3] *= -1.0
    c[1, 0] = 0.0
    if B > 1:
        c[:, 1] = (0.0, -0.5, 0.0)
    return torch.from_numpy(c)


def run_loss(pred, gt, anchors, C, weights=WEIGHTS, gmean=GMEAN, coef=None, size=SIZE):
    """All four loss entry points on one operand set, each output against fp64_ref.loss.  -> {output: bars dict} (after asserting
    the bitwise agreement of the two forward forms)."""
    from squeezedet_pytorch_amd import ops
    B = pred.shape[0]
    coef = make_coef(B, 3) if coef is None else coef
    p, g, a = pred.cuda(), gt.cuda(), anchors.cuda()
    losses, nobj = ops.loss_fwd(p, g, a, size, C, weights)
    losses_m, nobj_m, mean4 = ops.loss_mean_fwd(p, g, a, size, C, weights)
    dm = ops.loss_mean_bwd(p, g, a, nobj_m, torch.tensor([gmean], dtype=torch.float32, device='cuda'), size, C, weights)
    dc = ops.loss_bwd(p, g, a, nobj, coef.cuda(), size, C, weights)
    torch.cuda.synchronize()
    assert torch.equal(losses.view(torch.int32), losses_m.view(torch.int32)), 'sqd_loss_fwd and sqd_loss_mean_fwd per-image values differ'
    assert torch.equal(nobj.view(torch.int32), nobj_m.view(torch.int32))
    ref = R.loss(pred, gt, anchors, size, C, weights, gmean=gmean, coef=coef)
    assert torch.equal(nobj.cpu().double(), ref['nobj']), 'n_obj is not exact'
    flips = int(ref['flips'].sum())
    res = {'losses': R.bars_nan(losses.cpu(), ref['losses'], 'vec', 2), 'mean4': R.bars_nan(mean4.cpu(), ref['mean4'], 'vec', 2)}
    for name, got in (('dmean', dm.cpu()), ('dcoef', dc.cpu())):
        res[name] = R.bars_nan(got, R.pick(got, ref[name], ref[name + '_alt'], ref['flips']), 'dpred', 2)
    res['flips'] = flips
    return res


def _report(tag, res):
    bad = []
    for name in ('losses', 'mean4', 'dmean', 'dcoef'):
        b = res[name]
        print(f'loss {tag:34s} {name:7s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e})  P block {b["p_block"]:5.2f}  '
              f'P tensor {b["p_tensor"]:5.2f}  NaN positions ok={b["nan_ok"]}  flips {res["flips"]}')
        if not b['l_ok']:
            bad.append((name, b))
    assert not bad, (tag, bad)
    assert res['flips'] <= MAX_FLIPS, (tag, res['flips'])


@pytest.mark.parametrize('C', [1, 3, 16])
def test_exact_branch_edges(C):
    pred, gt, anchors = edge_case(C=C)
    res = run_loss(pred, gt, anchors, C)
    _report(f'edges C{C}', res)
    assert res['flips'] == 0            # exact constructions: both precisions sit on the same branch


def test_saturation():
    pred, gt, anchors = saturated_case()
    res = run_loss(pred, gt, anchors, 3)
    _report('saturated', res)


@pytest.mark.parametrize('A', [1, 15, 16, 17, 255, 256, 257, 16848, 25000])
def test_anchor_counts(A):
    pred, gt, anchors = random_case(2, A, 3, seed=100 + A)
    _report(f'A{A} B2 C3', run_loss(pred, gt, anchors, 3))


@pytest.mark.parametrize('B', [1, 63, 64, 65, 130])
def test_batch_sizes_both_finalize_forms(B):
    pred, gt, anchors = random_case(B, 300, 3, seed=200 + B)
    _report(f'B{B} A300 C3', run_loss(pred, gt, anchors, 3, coef=make_coef(B, 4 + B)))


@pytest.mark.parametrize('weights', [(0.7, 0.0, 55.0, 2.5), (2.0, 1.5, 0.0, 0.25)])
def test_loss_weights(weights):
    pred, gt, anchors = edge_case(C=3, seed=9)
    _report(f'weights {weights}', run_loss(pred, gt, anchors, 3, weights=weights))


def test_nan_semantics():
    """An image without positives (n_obj = 0) and one of positives only (n_obj = A) next to ordinary ones: NaN exactly where float64
    autograd of the reference has it, the bars everywhere else."""
    pred, gt, anchors = random_case(4, 500, 3, seed=300, nobj=[37, 0, 500, 11])
    res = run_loss(pred, gt, anchors, 3)
    _report('n_obj 0 and A', res)
    from squeezedet_pytorch_amd import ops
    losses, _ = ops.loss_fwd(pred.cuda(), gt.cuda(), anchors.cuda(), SIZE, 3, WEIGHTS)
    nan = torch.isnan(losses.cpu())
    assert nan[:, 1].all() and nan[[1, 3], 2].all() and not nan[[0, 2], 2].any()     # n_obj = 0: all four; n_obj = A: score, total
    assert not nan[:, 0].any() and not nan[:, 3].any()


def test_gmean_is_applied():
    """A backward that ignored gmean (took 1) fails: the 0.37 reference and the 1.0 reference are far apart at bar L."""
    pred, gt, anchors = random_case(2, 300, 3, seed=400)
    from squeezedet_pytorch_amd import ops
    p, g, a = pred.cuda(), gt.cuda(), anchors.cuda()
    _, nobj, _ = ops.loss_mean_fwd(p, g, a, SIZE, 3, WEIGHTS)
    dm = ops.loss_mean_bwd(p, g, a, nobj, torch.tensor([GMEAN], device='cuda'), SIZE, 3, WEIGHTS).cpu()
    r1 = R.loss(pred, gt, anchors, SIZE, 3, WEIGHTS, gmean=1.0)['dmean']
    assert not R.bars(dm, r1, 'dpred', 2)['l_ok']
    r = R.loss(pred, gt, anchors, SIZE, 3, WEIGHTS, gmean=GMEAN)['dmean']
    assert R.bars(dm, r, 'dpred', 2)['l_ok']


def test_seventeen_classes_refused():
    from squeezedet_pytorch_amd import ops
    pred, gt, anchors = random_case(1, 20, 17, seed=500)
    with pytest.raises(RuntimeError, match='bad argument'):
        ops.loss_fwd(pred.cuda(), gt.cuda(), anchors.cuda(), SIZE, 17, WEIGHTS)
    with pytest.raises(RuntimeError, match='bad argument'):
        ops.loss_bwd(pred.cuda(), gt.cuda(), anchors.cuda(), torch.ones(1, device='cuda'), torch.ones(3, 1, device='cuda'), SIZE, 17,
                     WEIGHTS)
