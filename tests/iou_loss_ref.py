"""float64 reference of the IoU-family box regression (``cfg.bbox_loss`` = 'iou' | 'giou' | 'diou' | 'ciou'; helper module of
tests/test_iou_loss_host.py, tests/test_iou_loss_gpu.py and tests/test_iou_loss_model_gpu.py; no project kernels).

The bbox component of the multi-task loss becomes ``w_bbox * sum_a [mask_a != 0] * (1 - q_a) / n_obj`` with, g the gt box, p the
clamped decoded box, inter / uni / iou = inter / (uni + eps) the confidence term's values, eps = 1e-10:

    gw = gx2 - gx1    gh = gy2 - gy1    pw = px2 - px1    ph = py2 - py1
    cw = max(gx2, px2) - min(gx1, px1)  ch = max(gy2, py2) - min(gy1, py1)
    rho2 = ((gx1 + gx2 - px1 - px2)^2 + (gy1 + gy2 - py1 - py2)^2) / 4
    iou : q = iou
    giou: q = iou - (cw*ch - uni) / (cw*ch + eps)
    diou: q = iou - rho2 / (cw^2 + ch^2 + eps)
    ciou: q = diou's - alpha * v, v = (4 / pi^2) * (atan(gw / (gh + eps)) - atan(pw / (ph + eps)))^2,
          alpha = v / (1 - iou + v + eps), detached

* ``twin``: that definition in plain torch on ``oracle.resolve_predictions``' decode, any dtype; torch autograd supplies the
  gradient (``twin_grads``).  'l2' is ``oracle.multitask_loss`` itself.  ``mutant`` (TWIN_MUTANTS): a wrong convention, for the teeth.
* ``loss``: what ``fp64_ref.loss`` returns, for a kind: Ref(ref64 = the twin in float64, M = the analytic chain on magnitudes, b32 =
  the twin in float32) of losses / mean4 / dmean / dcoef, the exact nobj, the flipped anchors and the ``*_alt`` gradients.  The chain
  is ``fp64_ref._loss_chain`` with w_bbox = 0 (class and score terms, the IoU path of the positive score) plus ``_box_chain``, the
  box term in the same value + magnitude algebra: the two gradients add.
* ``masked_loss``: ``ignore_ref.masked_loss`` with this ``loss`` in the place of ``fp64_ref.loss``.
"""
import contextlib
import math
import types

import numpy as np
import torch

import fp64_ref as R
import ignore_ref as IR
import oracle

F64, F32 = torch.float64, torch.float32
KINDS = ('iou', 'giou', 'diou', 'ciou')
TWIN_MUTANTS = ('alpha_attached', 'enclose_no_tie_split', 'penalty_detached', 'l2_term_added')
EPS = 1e-10                       # oracle.squeezedet_oracle.EPSILON
C4PI2 = 4.0 / math.pi ** 2


# ---- the twin ----

def box_q(g, p, kind, mutant=None):
    """q of gt boxes ``g`` [..., 4] and clamped predicted boxes ``p`` [..., 4] (xyxy), the definition op for op -> [...]."""
    gx1, gy1, gx2, gy2 = g.unbind(-1)
    px1, py1, px2, py2 = p.unbind(-1)
    lr = torch.clamp_min(torch.min(gx2, px2) - torch.max(gx1, px1), 0)
    tb = torch.clamp_min(torch.min(gy2, py2) - torch.max(gy1, py1), 0)
    inter = lr * tb
    gw, gh, pw, ph = gx2 - gx1, gy2 - gy1, px2 - px1, py2 - py1
    uni = gw * gh + pw * ph - inter
    iou = inter / (uni + EPS)
    if kind == 'iou':
        return iou
    if mutant == 'enclose_no_tie_split':            # a selection instead of maximum / minimum: a tie's gradient goes to p alone
        cw = torch.where(px2 >= gx2, px2, gx2) - torch.where(px1 <= gx1, px1, gx1)
        ch = torch.where(py2 >= gy2, py2, gy2) - torch.where(py1 <= gy1, py1, gy1)
    else:
        cw = torch.max(gx2, px2) - torch.min(gx1, px1)
        ch = torch.max(gy2, py2) - torch.min(gy1, py1)
    if kind == 'giou':
        pen = (cw * ch - uni) / (cw * ch + EPS)
    else:
        rho2 = ((gx1 + gx2 - px1 - px2) ** 2 + (gy1 + gy2 - py1 - py2) ** 2) / 4
        pen = rho2 / (cw ** 2 + ch ** 2 + EPS)
        if kind == 'ciou':
            v = C4PI2 * (torch.atan(gw / (gh + EPS)) - torch.atan(pw / (ph + EPS))) ** 2
            alpha = v / (1 - iou + v + EPS)
            pen = pen + (alpha if mutant == 'alpha_attached' else alpha.detach()) * v
        elif kind != 'diou':
            raise ValueError(kind)
    return iou - (pen.detach() if mutant == 'penalty_detached' else pen)


def twin(pred, gt, anchors, input_size, C, weights, kind, mutant=None):
    """``oracle.multitask_loss`` with the bbox component of ``kind`` ('l2': the oracle itself), in the dtype of ``pred``.
    ``anchors``: float32 numpy [A, 4].  -> (loss [B], stats dict of [B])."""
    assert mutant is None or mutant in TWIN_MUTANTS
    if kind == 'l2':
        return oracle.multitask_loss(pred, gt, anchors, tuple(input_size), C, *weights)
    assert kind in KINDS, kind
    class_w, pos_w, neg_w, bbox_w = weights
    num_anchors = pred.shape[1]
    mask, gt_boxes, gt_deltas, onehot = gt[..., :1], gt[..., 1:5], gt[..., 5:9], gt[..., 9:]
    _, logp, scores, deltas, boxes = oracle.resolve_predictions(pred, anchors, tuple(input_size), C, log_softmax=True)
    n_obj = mask.sum(dim=[1, 2])
    iou = box_q(gt_boxes, boxes, 'iou').unsqueeze(-1) * mask
    class_loss = (class_w * mask * onehot * (-logp)).sum(dim=[1, 2]) / n_obj
    pos = (pos_w * mask * (iou - scores) ** 2).sum(dim=[1, 2]) / n_obj
    neg = (neg_w * (1 - mask) * (iou - scores) ** 2).sum(dim=[1, 2]) / (num_anchors - n_obj)
    q = box_q(gt_boxes, boxes, kind, mutant)
    term = torch.where(mask[..., 0] != 0, 1 - q, torch.zeros((), dtype=q.dtype))
    bbox = bbox_w * term.sum(dim=1) / n_obj
    if mutant == 'l2_term_added':
        bbox = bbox + (bbox_w * mask * (deltas - gt_deltas) ** 2).sum(dim=[1, 2]) / n_obj
    loss = class_loss + pos + neg + bbox
    return loss, {'loss': loss, 'class_loss': class_loss, 'score_loss': pos + neg, 'bbox_loss': bbox}


def twin_grads(pred, gt, anchors, input_size, C, weights, kind, dtype, coef=None, gmean=None, mutant=None):
    """The twin in ``dtype`` on the host with torch autograd, as ``fp64_ref._oracle_loss``: -> (losses [4, B], dpred for gmean or
    None, dpred for coef or None)."""
    an = anchors.detach().to(F32).cpu().numpy().astype(np.float32)
    wts = [float(torch.tensor(w, dtype=F32)) for w in weights]
    lo, grads = None, {}
    for up in ('mean', 'coef', 'none'):
        if (up == 'mean' and gmean is None) or (up == 'coef' and coef is None) or (up == 'none' and lo is not None):
            continue
        with torch.enable_grad():
            p = pred.detach().cpu().to(dtype).requires_grad_(True)
            lv, st = twin(p, gt.detach().cpu().to(dtype), an, input_size, C, wts, kind, mutant)
            if up == 'mean':
                (lv.mean() * float(torch.tensor(float(gmean), dtype=F32))).backward()
            elif up == 'coef':
                cf = coef.detach().cpu().to(F32).to(dtype)
                (cf[0] * st['class_loss'] + cf[1] * st['score_loss'] + cf[2] * st['bbox_loss']).sum().backward()
        lo = torch.stack([st['class_loss'], st['score_loss'], st['bbox_loss'], lv]).detach()
        grads[up] = p.grad
    return lo, grads.get('mean'), grads.get('coef')


# ---- the box term in the value + magnitude algebra of fp64_ref ----

def _atan(a):
    v = torch.atan(a.v)
    return R._V(v, v.abs() + a.m / (1 + a.v * a.v))


def _w(weight):
    """An exact branch weight (0, 0.5 or 1) as a V."""
    return R._lf(weight)


def _box_chain(kind, pred, gt, anchors, input_size, C, w_bbox, ub, br):
    """[mask != 0] * (1 - q) of every anchor and the gradient of ``w_bbox * sum_a (that) / n_obj`` times the upstream ``ub`` [B] at
    the four deltas, with the branch weights ``br`` (``fp64_ref._branches``: the enclosing box takes 1 - the intersection's weights,
    it compares the same pairs).  -> (term V [B, A], ddelta V [B, A, 4])."""
    _add, _sub, _mul, _div, _neg, _c, _lf, _sel, _exp = R._add, R._sub, R._mul, R._div, R._neg, R._c, R._lf, R._sel, R._exp
    p, g = pred.to(F64), gt.to(F64)
    an = anchors.to(F32).to(F64)
    B, A = p.shape[:2]
    wmax, hmax = float(input_size[1] - 1), float(input_size[0] - 1)
    eps = _c(float(torch.tensor(1e-10, dtype=F32)))
    one, two, half = _c(1.0), _c(2.0), _c(0.5)
    mask = g[..., 0]
    on = (mask != 0).to(F64)
    # decode and IoU: fp64_ref._loss_chain's
    d = [_lf(p[..., C + 1 + j]) for j in range(4)]
    ax, ay, aw, ah = (_lf(an[:, j]) for j in range(4))
    cx, cy = _add(ax, _mul(aw, d[0])), _add(ay, _mul(ah, d[1]))
    w, h = _mul(aw, _exp(d[2])), _mul(ah, _exp(d[3]))
    hw, hh = _mul(half, _sub(w, one)), _mul(half, _sub(h, one))
    clampv = lambda a, hi: R._V(a.v.clamp(0, hi), a.m)                                # noqa: E731
    px1, py1 = clampv(_sub(cx, hw), wmax), clampv(_sub(cy, hh), hmax)
    px2, py2 = clampv(_add(cx, hw), wmax), clampv(_add(cy, hh), hmax)
    gx1, gy1, gx2, gy2 = (_lf(g[..., 1 + j]) for j in range(4))
    vmin = lambda a, b: R._V(torch.minimum(a.v, b.v), torch.maximum(a.m, b.m))        # noqa: E731
    vmax = lambda a, b: R._V(torch.maximum(a.v, b.v), torch.maximum(a.m, b.m))        # noqa: E731
    lr_raw, tb_raw = _sub(vmin(gx2, px2), vmax(gx1, px1)), _sub(vmin(gy2, py2), vmax(gy1, py1))
    lr, tb = R._V(lr_raw.v.clamp_min(0), lr_raw.m), R._V(tb_raw.v.clamp_min(0), tb_raw.m)
    inter = _mul(lr, tb)
    gw, gh, pw, ph = _sub(gx2, gx1), _sub(gy2, gy1), _sub(px2, px1), _sub(py2, py1)
    uni = _sub(_add(_mul(gw, gh), _mul(pw, ph)), inter)
    den = _add(uni, eps)
    iou = _div(inter, den)
    # the penalty and d pen / d (px1, py1, px2, py2)
    ex1, ey1, ex2, ey2 = (_w(1.0 - br[k]) for k in ('maxx', 'maxy', 'minx', 'miny'))   # d min(g1, p1) / d p1, d max(g2, p2) / d p2
    zero = R._V(torch.zeros(B, A, dtype=F64), torch.zeros(B, A, dtype=F64))
    pen, dpen = zero, [zero] * 4
    if kind != 'iou':
        cw, ch = _sub(vmax(gx2, px2), vmin(gx1, px1)), _sub(vmax(gy2, py2), vmin(gy1, py1))
        dcw = [_neg(ex1), None, ex2, None]
        dch = [None, _neg(ey1), None, ey2]
    if kind == 'giou':
        cc = _mul(cw, ch)
        ce = _add(cc, eps)
        pen = _div(_sub(cc, uni), ce)
        dix, diy = _sel(br['plr'], tb), _sel(br['ptb'], lr)                            # d inter / d (lr_raw, tb_raw)
        du = [_add(_neg(ph), _mul(dix, _w(br['maxx']))), _add(_neg(pw), _mul(diy, _w(br['maxy']))),
              _sub(ph, _mul(dix, _w(br['minx']))), _sub(pw, _mul(diy, _w(br['miny'])))]
        dc = [_mul(ch, dcw[0]), _mul(cw, dch[1]), _mul(ch, dcw[2]), _mul(cw, dch[3])]
        k1, k2 = _div(den, _mul(ce, ce)), _div(one, ce)
        dpen = [_sub(_mul(dc[j], k1), _mul(du[j], k2)) for j in range(4)]
    elif kind in ('diou', 'ciou'):
        sx = _sub(_sub(_add(gx1, gx2), px1), px2)
        sy = _sub(_sub(_add(gy1, gy2), py1), py2)
        rho2 = _mul(_add(_mul(sx, sx), _mul(sy, sy)), _c(0.25))
        c2e = _add(_add(_mul(cw, cw), _mul(ch, ch)), eps)
        pen = _div(rho2, c2e)
        k1, k2 = _div(one, c2e), _div(_mul(two, rho2), _mul(c2e, c2e))
        s = [sx, sy, sx, sy]
        cd = [_mul(cw, dcw[0]), _mul(ch, dch[1]), _mul(cw, dcw[2]), _mul(ch, dch[3])]
        dpen = [_sub(_neg(_mul(_mul(half, s[j]), k1)), _mul(cd[j], k2)) for j in range(4)]
        if kind == 'ciou':
            hp = _add(ph, eps)
            rp = _div(pw, hp)
            da = _sub(_atan(_div(gw, _add(gh, eps))), _atan(rp))
            v = _mul(_c(C4PI2), _mul(da, da))
            alpha = _div(v, _add(_add(_sub(one, iou), v), eps))
            pen = _add(pen, _mul(alpha, v))
            dpw = _div(_mul(alpha, _neg(_mul(_c(2.0 * C4PI2), da))), _mul(_add(one, _mul(rp, rp)), hp))
            dph = _neg(_mul(dpw, rp))
            dpen = [_sub(dpen[0], dpw), _sub(dpen[1], dph), _add(dpen[2], dpw), _add(dpen[3], dph)]
    term = _sel(on, _sub(one, _sub(iou, pen)))
    # backward: kq = d (ub * bbox) / d q, through the IoU (fp64_ref._loss_chain's chain with kq for dL_dov) and through -pen
    n = _lf(mask.sum(1).unsqueeze(1))
    u = ub.to(F64).view(B, 1).expand(B, A)
    kq = _neg(_sel(on, _div(_mul(R._V(u, u.abs()), _c(w_bbox)), n)))
    den2 = _mul(den, den)
    dov_dinter = _add(_div(one, den), _div(inter, den2))
    dov_dap = _neg(_div(inter, den2))
    dlr = _sel(br['plr'], _mul(_mul(kq, dov_dinter), tb))
    dtb = _sel(br['ptb'], _mul(_mul(kq, dov_dinter), lr))
    dap = _mul(kq, dov_dap)
    dpx2 = _sel(br['cx2'], _sub(_add(_sel(br['minx'], dlr), _mul(dap, ph)), _mul(kq, dpen[2])))
    dpx1 = _sel(br['cx1'], _sub(_sub(_neg(_sel(br['maxx'], dlr)), _mul(dap, ph)), _mul(kq, dpen[0])))
    dpy2 = _sel(br['cy2'], _sub(_add(_sel(br['miny'], dtb), _mul(dap, pw)), _mul(kq, dpen[3])))
    dpy1 = _sel(br['cy1'], _sub(_sub(_neg(_sel(br['maxy'], dtb)), _mul(dap, pw)), _mul(kq, dpen[1])))
    gd = [_mul(_add(dpx1, dpx2), aw), _mul(_add(dpy1, dpy2), ah),
          _mul(_mul(_sub(dpx2, dpx1), half), w), _mul(_mul(_sub(dpy2, dpy1), half), h)]
    gd = [_sel(on, x) for x in gd]
    return term, R._V(torch.stack([x.v for x in gd], -1), torch.stack([x.m for x in gd], -1))


def chain(kind, pred, gt, anchors, input_size, C, weights, u, br):
    """The loss of ``kind`` and its analytic gradient in the V algebra: ``fp64_ref._loss_chain`` without its bbox component + the
    box term.  ``u`` [3, B].  -> (losses V [4, B], dpred V [B, A, C+5])."""
    w_b = float(torch.tensor(weights[3], dtype=F32))
    gt0 = gt.clone()
    gt0[..., 5:9] = 0                                      # (the deltas' term has the weight 0: no NaN of theirs may enter)
    losses, nobj, dp, _ = R._loss_chain(pred, gt0, anchors, input_size, C, tuple(weights[:3]) + (0.0,), u, br)
    term, dd = _box_chain(kind, pred, gt, anchors, input_size, C, w_b, u[2], br)
    S = R._sum(term, 1, R.SUM_DEPTH_A)
    bbx = R._div(R._mul(R._c(w_b), S), R._lf(nobj))
    lv, lm = losses.v.clone(), losses.m.clone()
    tot = R._add(R._V(lv[3], lm[3]), bbx)
    lv[2], lm[2], lv[3], lm[3] = bbx.v, bbx.m, tot.v, tot.m
    dv, dm = dp.v.clone(), dp.m.clone()
    sm = R._add(R._V(dv[..., C + 1:], dm[..., C + 1:]), dd)
    # a NaN of the score path (n_obj = 0 or A) stays; a row without a box holds an exact zero of the box term
    dv[..., C + 1:], dm[..., C + 1:] = sm.v, sm.m
    return R._V(lv, lm), R._V(dv, dm)


def loss(pred, gt, anchors, input_size, C, weights, kind, gmean=None, coef=None, mutant=None):
    """``fp64_ref.loss`` for the bbox component ``kind`` (same keys; ref64 / b32: the twin's autograd in float64 / float32; M: the
    chain).  ``mutant`` (TWIN_MUTANTS): ref64 from the twin under a wrong convention (the CPU teeth)."""
    pred, gt, anchors = pred.detach().cpu(), gt.detach().cpu(), anchors.detach().cpu()
    B, A = pred.shape[:2]
    wmax, hmax = float(input_size[1] - 1), float(input_size[0] - 1)
    lo64, dm64, dc64 = twin_grads(pred, gt, anchors, input_size, C, weights, kind, F64, coef, gmean, mutant)
    lo32, dm32, dc32 = twin_grads(pred, gt, anchors, input_size, C, weights, kind, F32, coef, gmean)
    mask = gt[..., 0].to(F64)
    out = {'nobj': mask.sum(1)}
    ups = {}
    if gmean is not None:
        ups['dmean'] = (torch.full((3, B), float(torch.tensor(float(gmean), dtype=F32)) / B, dtype=F64), dm64, dm32)
    if coef is not None:
        ups['dcoef'] = (coef.detach().cpu().to(F32).to(F64), dc64, dc32)
    br64 = R._branches(*R._box64(pred, anchors, C), gt, wmax, hmax)
    br32 = R._branches(*R._decode32(pred, anchors, C), gt, wmax, hmax)
    flips = torch.zeros(B, A, dtype=torch.bool)
    for key in br64:
        flips |= (br64[key] != br32[key]) & (mask > 0)
    out['flips'] = flips
    losses = None
    for name, (u, ref64, b32) in ups.items():
        losses, dp = chain(kind, pred, gt, anchors, input_size, C, weights, u, br64)
        _l, dp32b = chain(kind, pred, gt, anchors, input_size, C, weights, u, br32)
        M = torch.where(flips.unsqueeze(-1), torch.maximum(dp.m, dp32b.m), dp.m)
        out[name] = R.Ref(ref64, M, b32)
        out[name + '_alt'] = torch.where(flips.unsqueeze(-1), dp32b.v, ref64)
        out[name + '_chain'] = dp
    if losses is None:
        losses, _ = chain(kind, pred, gt, anchors, input_size, C, weights, torch.zeros(3, B, dtype=F64), br64)
    out['losses'] = R.Ref(lo64, losses.m, lo32)
    out['losses_chain'] = losses
    out['mean4'] = R.Ref(lo64.mean(1), (losses.m.sum(1) + R.SUM_DEPTH_B * losses.v.abs().sum(1)) / B, lo32.mean(1))
    return out


@contextlib.contextmanager
def _loss_of(kind):
    """``ignore_ref`` with ``loss`` of ``kind`` in the place of ``fp64_ref.loss``."""
    proxy = types.SimpleNamespace(**{k: getattr(R, k) for k in dir(R) if not k.startswith('__')})
    proxy.loss = lambda *a, **kw: loss(*a, kind=kind, **kw)
    was = IR.R
    IR.R = proxy
    try:
        yield
    finally:
        IR.R = was


def masked_loss(kind, pred, gt, ign, anchors, input_size, C, weights, gmean=None, coef=None):
    """``ignore_ref.masked_loss`` for the bbox component ``kind``: an image is the unmasked loss of its kept rows; an image without
    positives has class = pos = bbox = 0 whatever the kind."""
    with _loss_of(kind):
        return IR.masked_loss(pred, gt, ign, anchors, input_size, C, weights, gmean=gmean, coef=coef)


# ---- operands ----

# two more 1-D constructions in the notation of test_fp64_loss_gpu.EDGES
EXTRA_EDGES = {
    'same_box': (25, 11, 0.0, 0.0, 20.0, 30.0),                        # px1 == gx1 and px2 == gx2: both edges tie at once
    'far_disjoint': (25, 11, 0.0, 0.0, 70.5, 90.0),                    # no overlap, a wide enclosing box
}


def edge_case(LG, C=3, A=64, seed=7):
    """``LG.edge_case`` (LG = tests/test_fp64_loss_gpu) with EXTRA_EDGES added: image 0 holds every construction along x (anchors
    0 .. 14), image 1 along y (anchors 15 .. 29), negatives elsewhere.  -> (pred, gt, anchors) float32 CPU tensors."""
    H, W = LG.SIZE
    edges = list(LG.EDGES.values()) + list(EXTRA_EDGES.values())
    rs = np.random.RandomState(seed)
    anchors = np.zeros((A, 4), np.float32)
    pred, gt = LG._negatives(rs, 2, A, C, anchors, W, H)
    for i, e in enumerate(edges):
        LG._positive(rs, pred, gt, anchors, 0, i, C, LG._resolve(e, W - 1), LG.NEUTRAL)
    for i, e in enumerate(edges):
        LG._positive(rs, pred, gt, anchors, 1, len(edges) + i, C, LG.NEUTRAL, LG._resolve(e, H - 1))
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(anchors)


def cases(LG, C=3):
    """[(name, (pred, gt, anchors))]: the edge constructions, the saturated logits and deltas, a random batch whose A = 200 leaves
    the last of the 16 slices ragged."""
    return [('edges', edge_case(LG, C=C)), ('saturated', LG.saturated_case(C=C)), ('random', LG.random_case(3, 200, C, seed=900 + C))]
