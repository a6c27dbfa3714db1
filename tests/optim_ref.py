"""Plain float64 reference of the fused AdamW step and of the weight EMA (helper module of tests/test_optim_ref_host.py,
tests/test_fp64_adamw_gpu.py; no project kernels), in the style of ``fp64_ref.clip_sgd``.

``clip_adamw_ema`` is ``clip_grad_norm_`` (as the coefficient ``coef`` the caller formed) + ``torch.optim.AdamW`` (non-amsgrad, decoupled
decay) + ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))`` computed in float64 from float32 snapshots, the
hyper-parameters rounded to float32 first (the kernel reads them from a float table).  Every output comes as a ``fp64_ref.Ref`` whose
``M`` bounds the rounding error of any float32 evaluation (bar L = 2^-18 M):

    M_m = b1 |m| + (1 - b1) |coef g|            M_v = v_new
    M_p = |p| (1 + lr wd) + (lr / bc1) M_m / den + |update|
    M_e = |e| + (1 - d_t) (M_p + |e|)           (on the copying first step: M_p)

``f32_chain`` is the same step as a plain float32 torch chain in the kernel's order (what a correct kernel can reach); ``MUTANTS`` are
wrong variants of the reference (the teeth of the CPU tier)."""
from __future__ import annotations

import math

import torch

from fp64_ref import F32, F64, Ref

MUTANTS = ('no_bias_correction', 't_off_by_one', 'eps_inside_sqrt', 'coupled_l2', 'ema_pre_step', 'lerp_first')


def f32(v):
    """A Python float rounded to float32."""
    return float(torch.tensor(float(v), dtype=F32))


def ema_decay_at(d, n, warmup):
    """The decay of the averaged step after ``n`` averaged steps: d, or with warm-up min(d, (1 + n) / (10 + n))."""
    d = f32(d)
    return min(d, (1.0 + n) / (10.0 + n)) if warmup else d


def clip_coef(norm, max_norm):
    """The kernel's formula for the clip coefficient from the norm the step returned (float32 arithmetic)."""
    if not max_norm > 0:
        return 1.0
    c = torch.tensor(max_norm, dtype=F32) / (torch.tensor(float(norm), dtype=F32) + torch.tensor(1e-6, dtype=F32))
    return min(float(c), 1.0)


def ema_update(e, pref, p_old, n, d, warmup, mutant=None):
    """The EMA after a step whose new parameter is the Ref ``pref`` (``e``: float32 snapshot of the average before the step, ``n``:
    averaged steps so far) -> Ref."""
    e = e.detach().double().cpu().reshape(pref.ref64.shape)
    src, src_m = pref.ref64, pref.M
    if mutant == 'ema_pre_step':
        src = p_old.detach().double().cpu().reshape(e.shape)
        src_m = src.abs()
    if n == 0 and mutant != 'lerp_first':
        return Ref(src.clone(), src_m.clone(), None)
    om = 1.0 - ema_decay_at(d, n, warmup)
    return Ref(e + om * (src - e), e.abs() + om * (src_m + e.abs()), None)


def clip_adamw_ema(params, grads, m, v, ema, t, n, hyper, coef, mutant=None):
    """One step.  ``params`` / ``grads`` / ``m`` / ``v`` / ``ema``: lists of float32 snapshots from before the step (``ema`` None: no
    average); ``t``: the number of this step (1 on the first); ``n``: averaged steps so far; ``hyper``: dict lr, beta1, beta2, eps,
    weight_decay, ema_decay, ema_warmup; ``coef``: the clip coefficient.  -> (ps, ms, vs, es): lists of Ref (es None without ``ema``)."""
    assert mutant is None or mutant in MUTANTS
    lr, b1, b2, eps, wd = (f32(hyper[k]) for k in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay'))
    tt = t - 1 if mutant == 't_off_by_one' else t
    bc1 = 1.0 - b1 ** tt if tt > 0 else 1.0
    bc2 = 1.0 - b2 ** tt if tt > 0 else 1.0
    if mutant == 'no_bias_correction':
        bc1 = bc2 = 1.0
    coef = float(coef)
    ps, ms, vs, es = [], [], [], []
    for i, (p, g, mm, vv) in enumerate(zip(params, grads, m, v)):
        p = p.detach().double().cpu()
        g = g.detach().double().cpu().reshape(p.shape) * coef
        mm = mm.detach().double().cpu().reshape(p.shape)
        vv = vv.detach().double().cpu().reshape(p.shape)
        if mutant == 'coupled_l2':
            g = g + wd * p
            pd = p
        else:
            pd = p - lr * wd * p
        mn = b1 * mm + (1.0 - b1) * g
        vn = b2 * vv + (1.0 - b2) * g * g
        den = torch.sqrt(vn + eps) / math.sqrt(bc2) if mutant == 'eps_inside_sqrt' else torch.sqrt(vn) / math.sqrt(bc2) + eps
        upd = (lr / bc1) * (mn / den)
        Mm = b1 * mm.abs() + (1.0 - b1) * g.abs()
        Mp = p.abs() * (1.0 + lr * wd) + (lr / bc1) * Mm / den + upd.abs()
        ps.append(Ref(pd - upd, Mp, None))
        ms.append(Ref(mn, Mm, None))
        vs.append(Ref(vn, vn.clone(), None))
        if ema is not None:
            es.append(ema_update(ema[i], ps[-1], params[i], n, hyper['ema_decay'], hyper['ema_warmup'], mutant))
    return ps, ms, vs, (es if ema is not None else None)


def f32_chain(params, grads, m, v, ema, t, n, hyper, coef):
    """The same step as a plain float32 torch chain in the kernel's order (the derived scalars lr / bc1, 1 / sqrt(bc2), 1 - d_t are
    evaluated in double and rounded to float32, as the begin launch does) -> (ps, ms, vs, es) lists of float32 tensors."""
    T = lambda x: torch.tensor(x, dtype=F32)          # noqa: E731
    lr, b1, b2, eps, wd = (T(hyper[k]) for k in ('lr', 'beta1', 'beta2', 'eps', 'weight_decay'))
    step = T(float(lr) / (1.0 - float(b1) ** t))
    rbc2 = T(1.0 / math.sqrt(1.0 - float(b2) ** t))
    omd = T(1.0 - ema_decay_at(hyper['ema_decay'], n, hyper['ema_warmup'])) if ema is not None else None
    lrwd, omb1, omb2, c = lr * wd, T(1.0) - b1, T(1.0) - b2, T(float(coef))
    ps, ms, vs, es = [], [], [], []
    for i, (p, g, mm, vv) in enumerate(zip(params, grads, m, v)):
        p = p.detach().to(F32).cpu()
        g = g.detach().to(F32).cpu().reshape(p.shape) * c
        mm = mm.detach().to(F32).cpu().reshape(p.shape)
        vv = vv.detach().to(F32).cpu().reshape(p.shape)
        pd = p - lrwd * p
        mn = b1 * mm + omb1 * g
        vn = b2 * vv + omb2 * (g * g)
        den = torch.sqrt(vn) * rbc2 + eps
        pn = pd - step * (mn / den)
        ps.append(pn); ms.append(mn); vs.append(vn)
        if ema is not None:
            e = ema[i].detach().to(F32).cpu().reshape(p.shape)
            es.append(pn.clone() if n == 0 else e + omd * (pn - e))
    return ps, ms, vs, (es if ema is not None else None)


def worst_ratio(got, r):
    """(max err / M over the elements with M > 0, whether every element is inside bar L, bar as a multiple given by the caller)."""
    err = (got.detach().double().cpu().reshape(r.ref64.shape) - r.ref64).abs()
    pos = r.M > 0
    ratio = float((err[pos] / r.M[pos]).max()) if bool(pos.any()) else 0.0
    return ratio, err
