"""GPU tier: gradient clipping + SGD with momentum (``FusedClipSGD``: ``sqd_grad_sumsq`` + ``sqd_sgd_clip_step_chunked`` on the flat
gradient buffer, foreach norm + ``sqd_sgd_clip_step`` on separate gradients) held to float64 (fp64_ref.clip_sgd) element by element.

The returned norm must be within 2^-18 of the float64 norm of the float32 gradient snapshot, every parameter and momentum element
within bar L (2^-18 M, M = |p| + lr (momentum |buf| + coef |g| + wd |p|), the bracket alone for a buffer).  Cases: the benchmarked
training step of both models (bench.py's seeds), flat layouts whose tensor offsets are not 16-byte aligned (the chunked kernel's scalar
path) or whose totals leave a tail (n & 3) or empty sum-of-squares blocks, separate gradients with parameters at odd element offsets
(the batched kernel's scalar path), and a hyper-parameter grid with the learning rate set through StepLR."""
import numpy as np
import pytest
import torch

import fp64_ref as R

pytestmark = pytest.mark.gpu

INPUT = (384, 1248)
STEPS = (('squeezedet', 20), ('squeezedetplus', 16))
NORM_BAR = 2.0 ** -18

# flat layouts (tensor sizes, consecutive in one buffer): offsets 5, 4101, ... are not multiples of 4 elements, total = 3 mod 4; 1021:
# the last of the 256 sum-of-squares blocks holds no quad, only the tail; 3: every block empty, the tail alone; an exact multiple of
# 4096 (whole chunks, no tail); a tail of large values
LAYOUTS = {'mixed': [5, 4096, 3, 4097, 1, 12289, 262147, 1], 'n1021': [1021], 'n3': [3], 'x4096': [4096, 8192],
           'tail_big': [4093, 6]}
TAIL_BIG = LAYOUTS['tail_big']


def flat_values(n, seed, big_tail=False):
    """Gradient values of a flat buffer of n elements (float32, CPU); ``big_tail``: the n & 3 tail holds large values."""
    rs = np.random.RandomState(seed)
    g = (rs.standard_normal(n) * 0.01).astype(np.float32)
    if big_tail:
        g[4 * (n >> 2):] = 3.0
    return torch.from_numpy(g)


def _check_step(opt, p0, g0, b0, norm, tag):
    """One FusedClipSGD.step against R.clip_sgd on the snapshots taken before it."""
    tn64, coef, refp, refb = R.clip_sgd(p0, g0, b0, opt.lr, opt.momentum, opt.weight_decay, opt.max_norm)
    assert np.isfinite(tn64), f'{tag}: the gradient holds non-finite values'
    worst_p = worst_b = 0.0
    bad = []
    for i, (p, b, rp, rb) in enumerate(zip(opt.params, opt._bufs, refp, refb)):
        for name, got, r in (('p', p, rp), ('buf', b, rb)):
            got = got.detach().double().cpu().reshape(r.ref64.shape)
            err = (got - r.ref64).abs()
            if not bool((err <= R.BAR_L * r.M).all()):
                bad.append((tag, name, i))
            pos = r.M > 0
            ratio = float((err[pos] / r.M[pos]).max()) if bool(pos.any()) else 0.0
            if name == 'p':
                worst_p = max(worst_p, ratio)
            else:
                worst_b = max(worst_b, ratio)
    nr = float('nan')
    if norm is not None:
        nr = abs(float(norm) - tn64) / tn64
        if not nr <= NORM_BAR:
            bad.append((tag, 'norm', float(norm), tn64))
    print(f'optim {tag:44s} norm {tn64:.6e} (rel err {nr:.2e}, bar {NORM_BAR:.2e})  coef {coef:.6f}  '
          f'param max err/M {worst_p:.2e}  buf max err/M {worst_b:.2e}')
    assert not bad, bad
    return tn64


def _snap(opt):
    return ([p.detach().clone() for p in opt.params], [p.grad.detach().clone() for p in opt.params], [b.clone() for b in opt._bufs])


@pytest.mark.parametrize('arch,batch', STEPS)
def test_benchmark_step(arch, batch):
    """bench.py's training step (make_train_step, fused optimizer, seeds 1234 / 0 / 1) run by hand: two steps at cfg.grad_norm (a zero,
    then a carried momentum buffer), then, each from the initial weights and a zero buffer again, one with max_norm at half the first
    norm (clip on) and one at twice it (clip off).  (Unclipped steps from the trained-on weights diverge within two steps at lr 0.01.)"""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.trainer import make_train_step
    torch.manual_seed(0)
    cfg = sqd.make_cfg(arch=arch, device='cuda')
    sd = synthetic.make_state_dict(arch, seed=1234)
    x = synthetic.make_images(batch, INPUT, seed=0).cuda()
    parts = {}
    make_train_step(cfg, sd, x, 0, 1, None, fused_optimizer=True, parts=parts)
    model, opt = parts['model'], parts['optimizer']
    batch_d = {'image': x, 'gt': synthetic.make_gt(batch, cfg.anchors, cfg.input_size, cfg.num_classes, seed=1).cuda()}
    assert opt.max_norm == cfg.grad_norm
    first = None
    init = [p.detach().clone() for p in opt.params]
    for it, mn in enumerate([None, None, 'half', 'twice']):
        if mn is not None:
            opt.param_groups[0]['max_norm'] = first / 2 if mn == 'half' else first * 2
            with torch.no_grad():
                for p, v in zip(opt.params, init):
                    p.copy_(v)
                opt.momentum_flat.zero_()
        loss, _ = model.forward_mean(batch_d)
        opt.zero_grad()
        loss.backward()
        assert opt._flat_base([p.grad for p in opt.params]) is not None, 'the gradients are not views of the flat buffer'
        p0, g0, b0 = _snap(opt)
        if it == 0:
            assert all(float(b.abs().max()) == 0.0 for b in b0)
        norm = opt.step()
        torch.cuda.synchronize()
        tn64 = _check_step(opt, p0, g0, b0, norm, f'{arch} b{batch} step {it} max_norm {opt.max_norm:.4g}')
        if it == 0:
            first = tn64
            print(f'{arch} b{batch}: initial gradient norm {tn64:.6g} (clip at {cfg.grad_norm}: {"on" if tn64 > cfg.grad_norm else "off"})')


def _flat_opt(sizes, seed, momentum, wd, max_norm):
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    rs = np.random.RandomState(seed)
    params = [torch.nn.Parameter(torch.from_numpy((rs.standard_normal(n) * 0.05).astype(np.float32)).cuda()) for n in sizes]
    holder = {}
    opt = FusedClipSGD(params, lr=0.01, momentum=momentum, weight_decay=wd, max_norm=max_norm, flat_grad=lambda: holder.get('flat'))
    return params, opt, holder


def _fill_flat(params, holder, sizes, seed, big_tail):
    flat = flat_values(sum(sizes), seed, big_tail).cuda()
    holder['flat'] = flat
    off = 0
    for p, n in zip(params, sizes):
        p.grad = flat[off:off + n]
        off += n
    return flat


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('clip', ['on', 'off'])
def test_flat_layouts(layout, clip):
    """Gradients as consecutive views of one flat buffer (the backward's layout): sqd_grad_sumsq + the chunked step when clipping,
    the batched step when not.  Two steps, the second with a carried momentum buffer and the StepLR-halved learning rate."""
    sizes = LAYOUTS[layout]
    offs = np.cumsum([0] + sizes[:-1])
    if layout == 'mixed':
        assert any((4 * o) % 16 for o in offs), 'no tensor of the layout takes the scalar path'
    if layout in ('n1021', 'n3'):
        assert sum(sizes) >> 2 < 256            # sum-of-squares blocks without a quad
    params, opt, holder = _flat_opt(sizes, 10, 0.9, 1e-4, 0.0)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
    for it in range(2):
        flat = _fill_flat(params, holder, sizes, 20 + it, layout == 'tail_big')
        if clip == 'on':
            opt.param_groups[0]['max_norm'] = 0.5 * float(flat.double().norm())
        assert opt._flat_base([p.grad for p in params]) is not None
        p0, g0, b0 = _snap(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        _check_step(opt, p0, g0, b0, norm, f'flat {layout} clip {clip} step {it} lr {opt.lr:g}')
        sched.step()
    assert opt.lr == 0.0025


@pytest.mark.parametrize('wd', [0.0, 1e-4])
@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('clip', ['on', 'off'])
def test_separate_gradients_unaligned_params(wd, momentum, clip):
    """Separate gradients (torch's foreach norm + sqd_sgd_clip_step), parameters that are views at odd element offsets of one storage:
    the batched kernel's scalar fallback."""
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    sizes = LAYOUTS['mixed']
    rs = np.random.RandomState(30)
    storage = torch.from_numpy((rs.standard_normal(sum(sizes) + 4 * len(sizes)) * 0.05).astype(np.float32)).cuda()
    params, off = [], 1
    for n in sizes:
        params.append(torch.nn.Parameter(storage[off:off + n]))
        off += n + 2                                         # odd offsets: 1, 8, ...
    assert any(p.data_ptr() % 16 for p in params), 'no parameter takes the scalar path'
    assert all(p.data_ptr() == storage.data_ptr() + 4 * o for p, o in zip(params, np.cumsum([1] + [n + 2 for n in sizes[:-1]])))
    opt = FusedClipSGD(params, lr=0.01, momentum=momentum, weight_decay=wd, max_norm=0.0)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, 0.5)
    for it in range(2):
        for i, p in enumerate(params):
            p.grad = flat_values(p.numel(), 40 + 7 * it + i).cuda()
        if clip == 'on':
            opt.param_groups[0]['max_norm'] = 0.5 * float(torch.cat([p.grad for p in params]).double().norm())
        p0, g0, b0 = _snap(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        assert (norm is None) == (clip == 'off')
        _check_step(opt, p0, g0, b0, norm, f'separate wd {wd:g} mom {momentum:g} clip {clip} step {it} lr {opt.lr:g}')
        sched.step()
