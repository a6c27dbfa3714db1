"""CPU tier of the fused AdamW + EMA step: the float64 reference (tests/optim_ref.py) against torch, the attainability of bar L by a plain
float32 chain in the kernel's order, the teeth of the bar against wrong variants of the reference, and the host logic of the optimizers
(state_dict round trips, refusals, the launches of the unchanged SGD path) through a fake native layer."""
import ctypes

import numpy as np
import pytest
import torch

import fp64_ref as R
import optim_ref as O

HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, ema_decay=0.999, ema_warmup=False)


# ---- 1. the reference against torch -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('clip', [True, False])
@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_reference_equals_torch_adamw_and_averaged_model(clip, wd):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    rs = np.random.RandomState(0)
    sizes = [7, 33, 129]
    hyper = dict(HYPER, weight_decay=wd)
    h32 = {k: O.f32(v) for k, v in hyper.items() if k != 'ema_warmup'}

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n) * 0.05).float().double())
                                              for n in sizes])
    model = Holder()
    params = list(model.ps)
    opt = torch.optim.AdamW(params, lr=h32['lr'], betas=(h32['beta1'], h32['beta2']), eps=h32['eps'], weight_decay=h32['weight_decay'])
    avg = AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(h32['ema_decay']))
    m = [torch.zeros(n) for n in sizes]
    v = [torch.zeros(n) for n in sizes]
    e = [torch.zeros(n) for n in sizes]
    for t in range(1, 5):
        grads = [torch.from_numpy(rs.standard_normal(n) * 0.01).float() for n in sizes]
        p0 = [p.detach().clone() for p in params]
        for p, g in zip(params, grads):
            p.grad = g.double().clone()
        tn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
        max_norm = 0.5 * tn if clip else 0.0
        coef = min(1.0, max_norm / (tn + 1e-6)) if clip else 1.0
        if clip:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        opt.step()
        avg.update_parameters(model)
        ps, ms, vs, es = O.clip_adamw_ema(p0, grads, m, v, e, t, t - 1, hyper, coef)
        for i, p in enumerate(params):
            st = opt.state[p]
            for name, got, r in (('p', p, ps[i]), ('m', st['exp_avg'], ms[i]), ('v', st['exp_avg_sq'], vs[i]),
                                 ('e', list(avg.module.ps)[i], es[i])):
                err = (got.detach() - r.ref64).abs()
                assert bool((err <= 1e-12 * r.M + 1e-300).all()), (t, i, name, float(err.max()))
        m = [r.ref64 for r in ms]; v = [r.ref64 for r in vs]; e = [r.ref64 for r in es]


def test_warmup_rule():
    d = O.f32(0.999)
    assert O.ema_decay_at(0.999, 0, True) == 0.1 and O.ema_decay_at(0.999, 5, True) == 6.0 / 15.0
    assert O.ema_decay_at(0.999, 10 ** 6, True) == d and O.ema_decay_at(0.999, 3, False) == d
    n_switch = next(n for n in range(20000) if (1.0 + n) / (10.0 + n) >= d)
    assert O.ema_decay_at(0.999, n_switch - 1, True) < d == O.ema_decay_at(0.999, n_switch, True)
    # the reference with warm-up is the lerp with d_t
    p0, g, z, e0 = torch.full((4,), 0.5), torch.full((4,), 0.01), torch.zeros(4), torch.full((4,), 0.25)
    for n in (1, 4, 50):
        ps, _, _, es = O.clip_adamw_ema([p0], [g], [z], [z], [e0], 1, n, dict(HYPER, ema_warmup=True), 1.0)
        want = e0.double() + (1.0 - min(d, (1.0 + n) / (10.0 + n))) * (ps[0].ref64 - e0.double())
        assert torch.equal(es[0].ref64, want)
    ps, _, _, es = O.clip_adamw_ema([p0], [g], [z], [z], [e0], 1, 0, dict(HYPER, ema_warmup=True), 1.0)
    assert torch.equal(es[0].ref64, ps[0].ref64)            # the first averaged step copies


# ---- 2. attainability and teeth -----------------------------------------------------------------------------------------------------

N = 300000
STEPS = 5


def _inputs():
    rs = np.random.RandomState(1)
    p = torch.from_numpy((rs.standard_normal(N) * 0.05).astype(np.float32))
    gs = []
    for _ in range(STEPS):
        g = (rs.standard_normal(N) * 0.01).astype(np.float32)
        g[1000:3000] = 0.0                 # exact-zero gradients: eps decides
        g[5000:9000] *= 1e-6               # a tiny block
        gs.append(torch.from_numpy(g))
    return p, gs


@pytest.fixture(scope='module')
def chain():
    """The float32 chain over STEPS steps and, per step, the snapshots it started from."""
    p, gs = _inputs()
    m, v, e = torch.zeros(N), torch.zeros(N), p.clone() * 0.5
    out = []
    for s, g in enumerate(gs):
        coef = 0.5 if s % 2 == 0 else 1.0
        ps, ms, vs, es = O.f32_chain([p], [g], [m], [v], [e], s + 1, s, HYPER, coef)
        out.append(dict(p0=p, g=g, m0=m, v0=v, e0=e, coef=coef, got=(ps[0], ms[0], vs[0], es[0])))
        p, m, v, e = ps[0], ms[0], vs[0], es[0]
    return out


def _ratios(step, s, mutant=None):
    refs = O.clip_adamw_ema([step['p0']], [step['g']], [step['m0']], [step['v0']], [step['e0']], s + 1, s, HYPER, step['coef'], mutant)
    return [O.worst_ratio(got, r[0])[0] / R.BAR_L for got, r in zip(step['got'], refs)]


def test_bar_is_attainable(chain):
    worst = [0.0] * 4
    for s, step in enumerate(chain):
        worst = [max(a, b) for a, b in zip(worst, _ratios(step, s))]
    print('float32 chain, worst err / (BAR_L M) on p, m, v, e:', ' '.join(f'{w:.3f}' for w in worst))
    assert max(worst) <= 0.25, worst


@pytest.mark.parametrize('mutant', O.MUTANTS)
def test_teeth(chain, mutant):
    if mutant == 'lerp_first':
        assert max(_ratios(chain[0], 0, mutant)) > 1.0
        return
    per_step = [max(_ratios(step, s, mutant)) for s, step in enumerate(chain)]
    print(mutant, [f'{r:.3g}' for r in per_step])
    assert max(per_step) > 1.0, (mutant, per_step)


# ---- 3. host logic through a fake native layer --------------------------------------------------------------------------------------

class FakeLib:
    """Records the entry points called; the launches do nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('sqd_'):
            raise AttributeError(name)

        def fn(*a):
            self.calls.append(name)
            return {'sqd_sgd_chunk_elems': 4096, 'sqd_grad_sumsq_parts': 256}.get(name, 0)
        return fn


@pytest.fixture
def fake(monkeypatch):
    from squeezedet_pytorch_amd import _native as nat
    lib = FakeLib()
    monkeypatch.setattr(nat, 'lib', lambda: lib)
    monkeypatch.setattr(nat, 'stream_handle', lambda device=None: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True), raising=False)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    return lib


LAUNCHES = ('sqd_grad_sumsq', 'sqd_sgd_clip_step', 'sqd_sgd_clip_step_chunked', 'sqd_sgd_clip_step_chunked_dev', 'sqd_fill_f32x4',
            'sqd_optim_begin', 'sqd_adamw_clip_step_chunked', 'sqd_sgd_clip_step_chunked_ema', 'sqd_param_swap')


def _params(sizes=(5, 4096, 3), seed=0):
    rs = np.random.RandomState(seed)
    return [torch.nn.Parameter(torch.from_numpy((rs.standard_normal(n) * 0.05).astype(np.float32))) for n in sizes]


def _flat_grads(params, holder):
    flat = torch.randn(sum(p.numel() for p in params))
    holder['flat'] = flat
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()]; off += p.numel()


def test_adamw_state_dict_round_trip(fake):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW
    a = FusedClipAdamW(_params(), lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05, max_norm=3.0, ema_decay=0.99, ema_warmup=True)
    assert set(a.state[a.params[0]]) == {'exp_avg', 'exp_avg_sq', 'ema'}
    assert all(torch.equal(e, p.detach()) for e, p in zip(a._emas, a.params))       # the average starts at the parameters
    a.exp_avg_flat.normal_(); a.exp_avg_sq_flat.uniform_(); a.ema_flat.normal_()
    a._set_step_counts(7, 5)
    torch.optim.lr_scheduler.StepLR(a, 1, 0.5)
    sd = a.state_dict()
    assert sd['t'] == 7 and sd['n'] == 5
    b = FusedClipAdamW(_params(seed=1), lr=1.0, ema_decay=0.5)
    b.load_state_dict(sd)
    assert b.step_counts() == (7, 5)
    for k in ('exp_avg_flat', 'exp_avg_sq_flat', 'ema_flat'):
        assert torch.equal(getattr(a, k), getattr(b, k))
    assert b._hyper_values() == a._hyper_values() == (2e-3, 0.8, 0.99, 1e-7, 0.05, 3.0, 0.99, 1.0)
    assert b.param_groups[0]['initial_lr'] == 2e-3
    assert torch.equal(b.state[b.params[1]]['exp_avg'], a.exp_avg_flat[5:5 + 4096])    # the registered state: views of the flat buffers


def test_adamw_loads_a_torch_adamw_state(fake):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW
    ps = _params()
    ref = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=3e-3, betas=(0.85, 0.98), eps=1e-6, weight_decay=0.02)
    for _ in range(2):
        for p in ref.param_groups[0]['params']:
            p.grad = torch.randn_like(p)
        ref.step()
    a = FusedClipAdamW(ps, lr=1.0, max_norm=2.0, ema_decay=0.9)
    a.load_state_dict(ref.state_dict())
    assert a.step_counts() == (2, 0)
    for rp, m, v in zip(ref.param_groups[0]['params'], a._m, a._v):
        assert torch.equal(m, ref.state[rp]['exp_avg']) and torch.equal(v, ref.state[rp]['exp_avg_sq'])
    assert a._hyper_values() == (3e-3, 0.85, 0.98, 1e-6, 0.02, 2.0, 0.9, 0.0)


def test_sgd_without_ema_is_todays_optimizer(fake):
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    holder = {}
    params = _params()
    opt = FusedClipSGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=5.0, flat_grad=lambda: holder.get('flat'))
    assert set(opt.state_dict()) == {'momentum_flat', 'lr', 'momentum', 'weight_decay', 'max_norm', 'initial_lr'}
    assert set(opt.state[params[0]]) == {'momentum_buffer'} and opt.hyper_on_device is False
    _flat_grads(params, holder)
    opt.step()
    assert [c for c in fake.calls if c in LAUNCHES] == ['sqd_grad_sumsq', 'sqd_sgd_clip_step_chunked']
    assert opt._table.shape == (3, 4)                      # the 4-word descriptor of the existing kernels
    del fake.calls[:]
    opt.hyper_on_device = True
    opt.step(); opt.step()
    assert [c for c in fake.calls if c in LAUNCHES] == ['sqd_fill_f32x4', 'sqd_grad_sumsq', 'sqd_sgd_clip_step_chunked_dev',
                                                        'sqd_grad_sumsq', 'sqd_sgd_clip_step_chunked_dev']
    del fake.calls[:]
    sep = FusedClipSGD(_params(), lr=0.01, momentum=0.9)
    for p in sep.params:
        p.grad = torch.randn_like(p)
    sep.step()
    assert [c for c in fake.calls if c in LAUNCHES] == ['sqd_sgd_clip_step']


def test_launch_sequences_with_ema(fake):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, FusedClipSGD
    holder = {}
    params = _params()
    opt = FusedClipSGD(params, lr=0.01, momentum=0.9, max_norm=5.0, flat_grad=lambda: holder.get('flat'), ema_decay=0.999)
    assert opt.hyper_on_device is True and opt.state_dict().keys() >= {'ema_flat', 'n', 'ema_decay', 'ema_warmup'}
    _flat_grads(params, holder)
    opt.step(); opt.step()
    step = ['sqd_grad_sumsq', 'sqd_optim_begin', 'sqd_sgd_clip_step_chunked_ema']
    assert [c for c in fake.calls if c in LAUNCHES] == ['sqd_fill_f32x4', 'sqd_fill_f32x4'] + step + step      # no host write at step 2
    assert opt._table.shape == (3, 6)
    del fake.calls[:]
    params = _params()
    adam = FusedClipAdamW(params, lr=1e-3, max_norm=5.0, flat_grad=lambda: holder.get('flat'))
    _flat_grads(params, holder)
    adam.step(); adam.step()
    step = ['sqd_grad_sumsq', 'sqd_optim_begin', 'sqd_adamw_clip_step_chunked']
    assert [c for c in fake.calls if c in LAUNCHES] == ['sqd_fill_f32x4', 'sqd_fill_f32x4'] + step + step
    del fake.calls[:]
    adam.param_groups[0]['lr'] = 5e-4                      # a schedule: the table is rewritten once
    adam.step()
    assert [c for c in fake.calls if c in LAUNCHES] == ['sqd_fill_f32x4', 'sqd_fill_f32x4'] + step


def test_refusals(fake):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, FusedClipSGD
    holder = {}
    params = _params()
    opt = FusedClipSGD(params, lr=0.01, momentum=0.9, max_norm=5.0, flat_grad=lambda: holder.get('flat'), ema_decay=0.999)
    _flat_grads(params, holder)
    opt.hyper_on_device = False
    with pytest.raises(RuntimeError, match='launch-argument path'):
        opt.step()
    opt.hyper_on_device = True
    for p in params:
        p.grad = torch.randn_like(p)                       # separate gradients
    with pytest.raises(RuntimeError, match='launch-argument path'):
        opt.step()
    assert not [c for c in fake.calls if c.endswith('_ema') or c == 'sqd_optim_begin']
    with opt.averaged_weights():
        with pytest.raises(RuntimeError, match='nested'):
            with opt.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match='averaged_weights'):
            opt.step()
    assert fake.calls.count('sqd_param_swap') == 2 and opt._averaging is False
    off = FusedClipAdamW(_params(), lr=1e-3)
    with pytest.raises(RuntimeError, match='EMA is off'):
        with off.averaged_weights():
            pass
    with pytest.raises(RuntimeError, match='EMA is off'):
        off.ema_state_dict(torch.nn.Module())
    with pytest.raises(ValueError, match='ema_decay'):
        FusedClipAdamW(_params(), lr=1e-3, ema_decay=1.0)
    import squeezedet_pytorch_amd as sqd
    cfg = sqd.make_cfg(device='cpu')
    assert (cfg.optimizer, cfg.ema_decay, cfg.ema_warmup, cfg.ema_eval) == ('sgd', 0.0, False, False)
    assert sqd.FusedClipAdamW is FusedClipAdamW
