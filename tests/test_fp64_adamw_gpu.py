"""GPU tier: the fused AdamW step and the weight EMA (``FusedClipAdamW``, ``FusedClipSGD(ema_decay > 0)``: ``sqd_grad_sumsq`` +
``sqd_optim_begin`` + ``sqd_adamw_clip_step_chunked`` / ``sqd_sgd_clip_step_chunked_ema``) held to float64 element by element.

Every element of the new parameter, of both moments and of the EMA must lie within bar L (fp64_ref.BAR_L = 2^-18, times the magnitudes of
optim_ref.clip_adamw_ema) of the float64 step computed from float32 snapshots.  The reference's clip coefficient is formed by the kernel's
formula from the norm the step returned; that norm is held separately to test_fp64_optim_gpu.NORM_BAR against the float64 norm of the
gradient snapshot.  Cases: the flat layouts of test_fp64_optim_gpu.LAYOUTS (scalar path, n & 3 tail, empty sum-of-squares blocks, whole
chunks) with clip on and off; separate gradients on parameters at odd element offsets; EMA off, on, on with warm-up; three steps each
(zero state, carried state, StepLR-halved learning rate); the same sweep for SGD + EMA (fp64_ref.clip_sgd for the parameter and the
momentum); the real 64-tensor model."""
import numpy as np
import pytest
import torch

import fp64_ref as R
import optim_ref as O
from test_fp64_optim_gpu import LAYOUTS, NORM_BAR, flat_values

pytestmark = pytest.mark.gpu

EMA = {'off': dict(ema_decay=0.0), 'on': dict(ema_decay=0.999), 'warmup': dict(ema_decay=0.999, ema_warmup=True)}


def _bar(got, r, tag, bad):
    ratio, err = O.worst_ratio(got, r)
    if not bool((err <= R.BAR_L * r.M).all()):
        bad.append(tag)
    return ratio


def _norm_check(norm, g0, tag, bad):
    tn64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g0)))
    assert np.isfinite(tn64), f'{tag}: the gradient holds non-finite values'
    nr = float('nan')
    if norm is not None:
        nr = abs(float(norm) - tn64) / tn64
        if not nr <= NORM_BAR:
            bad.append((tag, 'norm', float(norm), tn64))
    return tn64, nr


def _snap_adamw(opt):
    c = lambda ts: [t.detach().clone() for t in ts]          # noqa: E731
    return (c(opt.params), c([p.grad for p in opt.params]), c(opt._m), c(opt._v), c(opt._emas) if opt.ema_on else None)


def _check_adamw(opt, snap, norm, t, n, tag):
    """One FusedClipAdamW.step (the t-th; n averaged steps before it) against optim_ref.clip_adamw_ema on the snapshots taken before it."""
    p0, g0, m0, v0, e0 = snap
    bad = []
    tn64, nr = _norm_check(norm, g0, tag, bad)
    coef = O.clip_coef(float(norm), opt.max_norm) if norm is not None else 1.0
    b1, b2 = opt.betas
    hyper = dict(lr=opt.lr, beta1=b1, beta2=b2, eps=opt.eps, weight_decay=opt.weight_decay, ema_decay=opt.ema_decay,
                 ema_warmup=opt.ema_warmup)
    ps, ms, vs, es = O.clip_adamw_ema(p0, g0, m0, v0, e0, t, n, hyper, coef)
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0, 'e': 0.0}
    outs = [('p', opt.params, ps), ('m', opt._m, ms), ('v', opt._v, vs)] + ([('e', opt._emas, es)] if es is not None else [])
    for name, gots, refs in outs:
        for i, (got, r) in enumerate(zip(gots, refs)):
            worst[name] = max(worst[name], _bar(got, r, (tag, name, i), bad))
    print(f'adamw {tag:52s} norm {tn64:.6e} (rel err {nr:.2e}, bar {NORM_BAR:.2e}) coef {coef:.6f}  max err/M  '
          + '  '.join(f'{k} {w:.2e}' for k, w in worst.items()) + f'  (bar {R.BAR_L:.2e})')
    assert not bad, bad
    assert opt.step_counts() == (t, n + 1 if opt.ema_on else 0), (opt.step_counts(), t, n)


def _fill_flat(params, holder, sizes, seed, big_tail):
    flat = flat_values(sum(sizes), seed, big_tail).cuda()
    holder['flat'] = flat
    off = 0
    for p, n in zip(params, sizes):
        p.grad = flat[off:off + n]
        off += n
    return flat


def _params(sizes, seed):
    rs = np.random.RandomState(seed)
    return [torch.nn.Parameter(torch.from_numpy((rs.standard_normal(n) * 0.05).astype(np.float32)).cuda()) for n in sizes]


@pytest.mark.parametrize('ema', list(EMA))
@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('clip', ['on', 'off'])
def test_adamw_flat_layouts(layout, clip, ema):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW
    sizes = LAYOUTS[layout]
    if layout == 'mixed':
        assert any((4 * o) % 16 for o in np.cumsum([0] + sizes[:-1])), 'no tensor of the layout takes the scalar path'
    params = _params(sizes, 10)
    holder = {}
    opt = FusedClipAdamW(params, lr=1e-3, weight_decay=1e-2, flat_grad=lambda: holder.get('flat'), **EMA[ema])
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    for it in range(3):
        flat = _fill_flat(params, holder, sizes, 20 + it, layout == 'tail_big')
        if clip == 'on':
            opt.param_groups[0]['max_norm'] = 0.5 * float(flat.double().norm())
        assert opt._flat_base([p.grad for p in params]) is not None
        snap = _snap_adamw(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        assert (norm is None) == (clip == 'off')
        _check_adamw(opt, snap, norm, it + 1, it, f'flat {layout} clip {clip} ema {ema} step {it} lr {opt.lr:g}')
        sched.step()
    assert opt.lr == 5e-4


@pytest.mark.parametrize('ema', list(EMA))
@pytest.mark.parametrize('clip', ['on', 'off'])
def test_adamw_separate_gradients_unaligned_params(clip, ema):
    """Separate gradients (by address, torch's foreach norm in a device scalar), parameters that are views at odd element offsets of one
    storage: the scalar fallback."""
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW
    sizes = LAYOUTS['mixed']
    rs = np.random.RandomState(30)
    storage = torch.from_numpy((rs.standard_normal(sum(sizes) + 4 * len(sizes)) * 0.05).astype(np.float32)).cuda()
    params, off = [], 1
    for n in sizes:
        params.append(torch.nn.Parameter(storage[off:off + n]))
        off += n + 2                                         # odd offsets: 1, 8, ...
    assert any(p.data_ptr() % 16 for p in params), 'no parameter takes the scalar path'
    opt = FusedClipAdamW(params, lr=1e-3, weight_decay=1e-2, **EMA[ema])
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    for it in range(3):
        for i, p in enumerate(params):
            p.grad = flat_values(p.numel(), 40 + 7 * it + i).cuda()
        if clip == 'on':
            opt.param_groups[0]['max_norm'] = 0.5 * float(torch.cat([p.grad for p in params]).double().norm())
        snap = _snap_adamw(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        assert (norm is None) == (clip == 'off')
        _check_adamw(opt, snap, norm, it + 1, it, f'separate clip {clip} ema {ema} step {it} lr {opt.lr:g}')
        sched.step()


@pytest.mark.parametrize('ema', ['on', 'warmup'])
@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('clip', ['on', 'off'])
def test_sgd_ema_flat_layouts(layout, clip, ema):
    """FusedClipSGD(ema_decay > 0): the parameter and the momentum against fp64_ref.clip_sgd, the EMA against the EMA bar."""
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    sizes = LAYOUTS[layout]
    params = _params(sizes, 10)
    holder = {}
    opt = FusedClipSGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, flat_grad=lambda: holder.get('flat'), **EMA[ema])
    sched = torch.optim.lr_scheduler.StepLR(opt, 2, 0.5)
    for it in range(3):
        flat = _fill_flat(params, holder, sizes, 20 + it, layout == 'tail_big')
        if clip == 'on':
            opt.param_groups[0]['max_norm'] = 0.5 * float(flat.double().norm())
        c = lambda ts: [t.detach().clone() for t in ts]      # noqa: E731
        p0, g0, b0, e0 = c(params), c([p.grad for p in params]), c(opt._bufs), c(opt._emas)
        norm = opt.step()
        torch.cuda.synchronize()
        tag = f'sgd flat {layout} clip {clip} ema {ema} step {it} lr {opt.lr:g}'
        bad = []
        tn64, nr = _norm_check(norm, g0, tag, bad)
        _, coef, refp, refb = R.clip_sgd(p0, g0, b0, opt.lr, opt.momentum, opt.weight_decay, opt.max_norm)
        worst = {'p': 0.0, 'buf': 0.0, 'e': 0.0}
        for i, (p, b, e, rp, rb) in enumerate(zip(params, opt._bufs, opt._emas, refp, refb)):
            re = O.ema_update(e0[i], rp, p0[i], it, opt.ema_decay, opt.ema_warmup)
            for name, got, r in (('p', p, rp), ('buf', b, rb), ('e', e, re)):
                worst[name] = max(worst[name], _bar(got, r, (tag, name, i), bad))
        print(f'{tag:56s} norm {tn64:.6e} (rel err {nr:.2e}) coef {coef:.6f}  max err/M  '
              + '  '.join(f'{k} {w:.2e}' for k, w in worst.items()) + f'  (bar {R.BAR_L:.2e})')
        assert not bad, bad
        assert opt.step_counts() == (0, it + 1)
        sched.step()


class _Recorder:
    """A wrapper around the native library that records the entry points called."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_sgd_without_ema_is_unchanged(monkeypatch):
    """FusedClipSGD with the EMA off makes the library calls of the parent commit's code paths and keeps its state_dict keys; with the
    EMA on, the parameters and the momentum keep those bits (one source expression)."""
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    rec = _Recorder(nat.lib())
    monkeypatch.setattr(nat, 'lib', lambda: rec)
    launches = lambda: [c for c in rec.calls if c not in ('sqd_sgd_chunk_elems', 'sqd_grad_sumsq_parts')]      # noqa: E731
    sizes = LAYOUTS['mixed']
    sides = {}
    for name, kw in (('arg', {}), ('dev', {}), ('ema', dict(ema_decay=0.999))):
        params, holder = _params(sizes, 10), {}
        opt = FusedClipSGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=1.0, flat_grad=lambda h=holder: h.get('flat'), **kw)
        if name == 'dev':
            opt.hyper_on_device = True
        sides[name] = (params, opt, holder)
    assert set(sides['arg'][1].state_dict()) == {'momentum_flat', 'lr', 'momentum', 'weight_decay', 'max_norm', 'initial_lr'}
    want = {'arg': ['sqd_grad_sumsq', 'sqd_sgd_clip_step_chunked'], 'dev': ['sqd_grad_sumsq', 'sqd_sgd_clip_step_chunked_dev'],
            'ema': ['sqd_grad_sumsq', 'sqd_optim_begin', 'sqd_sgd_clip_step_chunked_ema']}
    for it in range(2):
        for name, (params, opt, holder) in sides.items():
            _fill_flat(params, holder, sizes, 20 + it, False)
            del rec.calls[:]
            opt.step()
            fills = {'arg': 0, 'dev': 1, 'ema': 2}[name] if it == 0 else 0
            assert launches() == ['sqd_fill_f32x4'] * fills + want[name], (name, it, rec.calls)
        torch.cuda.synchronize()
        for name in ('dev', 'ema'):
            for i, (a, b) in enumerate(zip(sides['arg'][0], sides[name][0])):
                assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), (name, it, 'parameter', i)
            assert torch.equal(sides['arg'][1].momentum_flat.view(torch.int32), sides[name][1].momentum_flat.view(torch.int32)), (name, it)
    # separate gradients without clipping: the batched launch alone
    params = _params([5, 7], 3)
    opt = FusedClipSGD(params, lr=0.01, momentum=0.9)
    for p in params:
        p.grad = torch.randn_like(p)
    del rec.calls[:]
    opt.step()
    assert launches() == ['sqd_sgd_clip_step']


def test_adamw_ema_real_model():
    """The 64-tensor model at the size of tests/test_graph_step_gpu.py: one forward / backward, two steps on its gradient."""
    import test_graph_step_gpu as G
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, find_base
    torch.manual_seed(3)
    cfg = G.make_cfg()
    model = G.make_model(cfg)
    base = find_base(model)
    opt = FusedClipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2, max_norm=5.0, ema_decay=0.999,
                         ema_warmup=True, flat_grad=lambda: base.last_grad_flat)
    assert len(opt.params) == 64
    loss, _ = model.forward_mean(G.make_batch(cfg, 'dense', 2, seed=7))
    opt.zero_grad()
    loss.backward()
    assert opt._flat_base([p.grad for p in opt.params]) is not None, 'the gradients are not views of the flat buffer'
    tn = float(torch.cat([p.grad.reshape(-1) for p in opt.params]).double().norm())
    opt.param_groups[0]['max_norm'] = 0.5 * tn                  # clip on
    for it in range(2):
        snap = _snap_adamw(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        _check_adamw(opt, snap, norm, it + 1, it, f'squeezedet {G.SIZE} 64 tensors step {it}')
