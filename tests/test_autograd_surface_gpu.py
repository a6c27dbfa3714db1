"""GPU tier: the ``nn.Module`` training surface (``SqueezeDetWithLoss`` / ``SqueezeDetBase`` / ``Loss`` behind hand-written
``torch.autograd.Function``s) held to torch autograd's semantics.  Every scenario of tests/autograd_twin.py runs on the HIP model and
on the float64 twin and the resulting ``p.grad`` are compared

* against the twin at the project's own bars (``_check_grads_flip_aware``: ConvDet 2e-4 of the tensor's scale, elsewhere 5e-2 max and
  2e-2 relative L2; ``rtol=1e-4`` on loss values); for the foreign upstream gradients a bar the float32 twin alone exceeds becomes
  4x its measured error (none does at these operands: the printed lines carry the figures);
* bit for bit against isolated HIP runs (the training step is deterministic run to run, asserted first): accumulation is the fp32 add
  AccumulateGrad performs, a backward uses its own forward's dropout mask, a trainable parameter's gradient does not depend on who
  else trains, a power-of-two scale of the loss is a power-of-two scale of every gradient.

The misuses torch refuses are refused here too, by a ``RuntimeError`` that names the cause, before any launch: a parameter updated in
place between forward and backward, a second backward through the same forward (also with ``retain_graph=True``: the activations are
freed after the first), an image that requires grad."""
import functools

import numpy as np
import pytest
import torch

import fp64_ref as R
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import boxes, ops, synthetic

import autograd_twin as T

pytestmark = pytest.mark.gpu
SIZE = T.SIZE
SEED = 21                                     # torch.manual_seed of the tests with dropout (the device stream derives from it)


@functools.lru_cache(maxsize=None)
def _setup(arch='squeezedet', C=3, ignore_density=None):
    cfg = sqd.make_cfg(arch=arch, input_size=SIZE, num_classes=C)
    sd = synthetic.make_state_dict(arch, seed=1234, num_classes=C)
    return cfg, sd, T.make_cases(cfg, C, ignore_density)


def _hip(arch='squeezedet', C=3, dropout=0.0, form='dense', ignore_density=None):
    """-> (HIP model in train mode, its batches A (2 images) and B (1 image) on the device)."""
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    _, sd, cases = _setup(arch, C, ignore_density)
    cfg = sqd.make_cfg(arch=arch, input_size=SIZE, num_classes=C, dropout_prob=dropout, sparse_gt=(form != 'dense'))
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(sd, strict=True)
    batches = []
    for c in cases:
        b = {'image': c['image'].cuda()}
        if form == 'dense':
            b['gt'] = c['gt'].cuda()
        else:
            b['gt_sparse'] = ops.sparse_gt_from_dense(c['gt'].cuda())
            assert torch.equal(ops.sparse_gt_to_dense(b['gt_sparse'], cfg.num_anchors, C).cpu(), c['gt'])     # the twin's dense equivalent
            if form == 'masked':
                b['gt_ignore'] = torch.from_numpy(boxes.pack_ignore_bits(np.asarray(c['ign']))).cuda()
        batches.append(b)
    return m.cuda().train(), batches


class HipHelpers:
    """How a scenario talks to the HIP model.  Before every train-mode forward with dropout the mask that forward will apply is read
    back through the stand-alone kernel (``ops.dropout_mask``: a function of seed, step and element index) for the twin."""

    def __init__(self, arch='squeezedet'):
        self.masks = []
        self.channels = synthetic.convdet_in_channels(arch)

    def _record(self, model, batch):
        base = model.base
        if base.training and base.dropout is not None:
            d = base.drop_state(batch['image'].device)
            n = batch['image'].shape[0]
            self.masks.append(ops.dropout_mask(d, (n, 4, 6, self.channels)).permute(0, 3, 1, 2).contiguous().cpu())

    def forward(self, model, batch):
        self._record(model, batch)
        return model(batch)

    def forward_mean(self, model, batch):
        self._record(model, batch)
        return model.forward_mean(batch)

    def pred(self, model, batch):
        self._record(model, batch)
        return model.base(batch['image'])


def _twin_run(scenario, *args, arch='squeezedet', C=3, ignore_density=None, masks=None, dtype=T.F64):
    cfg, sd, cases = _setup(arch, C, ignore_density)
    twin = T.Twin(sd, cfg.anchors, SIZE, arch, C, dtype).train()
    return scenario(twin, T.twin_batches(cases, dtype), T.TwinHelpers(masks), *args)


@functools.lru_cache(maxsize=None)
def _twin_cached(scenario, *args, dtype=T.F64):
    """(mask-free scenarios on the default operands: one float64 / float32 evaluation shared by the tests that need it)"""
    return _twin_run(scenario, *args, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _hip_alone(which, mean=False):
    """Gradients of micro-batch ``which`` run alone on a fresh model (dropout off): the operands of the bit-for-bit checks."""
    m, batches = _hip()
    if mean:
        loss, _ = m.forward_mean(batches[which])
        loss.backward()
        return T.snap(m)
    return T.sc_single(m, batches, HipHelpers(), which=which)['grads']


def _equal_bits(a, b, what):
    for n in a:
        assert (a[n] is None) == (b[n] is None), (what, n)
        if a[n] is not None:
            assert torch.equal(a[n], b[n]), f'{what}: {n} differs by {float((a[n] - b[n]).abs().max()):.3e}'


def _report(tag, got, ref, bars=T.DEFAULT_BARS, names=None):
    t, mx, l2 = T.measure({n: g for n, g in got.items() if g is not None}, ref, names)
    print(f'autograd surface {tag:46s} vs float64 twin: convdet {t:.2e} (bar {bars[0]:.1e})  max {mx:.2e} (bar {bars[1]:.1e})  '
          f'relL2 {l2:.2e} (bar {bars[2]:.1e})')


def test_training_step_is_deterministic_run_to_run():
    """DESIGN.md's claim the bit-for-bit checks below stand on: the same forward and backward twice, on one model and on two."""
    m, batches = _hip()
    for which in (0, 1):
        first = T.sc_single(m, batches, HipHelpers(), which=which)['grads']
        m.zero_grad()
        again = T.sc_single(m, batches, HipHelpers(), which=which)['grads']
        m.zero_grad()
        _equal_bits(first, again, f'micro-batch {which}, same model')
        _equal_bits(first, _hip_alone(which), f'micro-batch {which}, fresh model')


@pytest.mark.parametrize('mode', ['plain', 'zero_first', 'mean'])
def test_accumulation_over_micro_batches_of_different_size(mode):
    m, batches = _hip()
    out = T.sc_accumulate(m, batches, HipHelpers(), mode)
    ref = _twin_cached(T.sc_accumulate, mode)
    T.check_loss(out['loss_A'], ref['loss_A']); T.check_loss(out['loss_B'], ref['loss_B'])
    _report(f'accumulate A(2)+B(1) {mode}', out['grads'], ref['grads'])
    T.check_grads(out['grads'], ref['grads'])
    ga, gb = _hip_alone(0, mode == 'mean'), _hip_alone(1, mode == 'mean')
    _equal_bits(out['grads'], {n: ga[n] + gb[n] for n in ga}, 'accumulated p.grad against g_A + g_B')


@pytest.mark.parametrize('arch,C', [('squeezedetplus', 3), ('squeezedet', 20)])
def test_accumulation_other_model_and_padded_convdet_width(arch, C):
    """SqueezeDet+ and num_classes = 20 (ConvDet width 225, run zero-padded: ``convdet_unpack`` / ``wgrad_reduce_rows`` on two batch sizes)."""
    if C == 20:
        assert ops.convdet_pad_width(9 * 25) != 9 * 25
    m, batches = _hip(arch, C)
    out = T.sc_accumulate(m, batches, HipHelpers(arch), 'plain')
    ref = _twin_run(T.sc_accumulate, 'plain', arch=arch, C=C)
    T.check_loss(out['loss_A'], ref['loss_A']); T.check_loss(out['loss_B'], ref['loss_B'])
    _report(f'accumulate {arch} C={C}', out['grads'], ref['grads'])
    T.check_grads(out['grads'], ref['grads'])
    alone = []
    for which in (0, 1):
        m2, b2 = _hip(arch, C)
        alone.append(T.sc_single(m2, b2, HipHelpers(arch), which=which)['grads'])
    _equal_bits(out['grads'], {n: alone[0][n] + alone[1][n] for n in alone[0]}, 'accumulated p.grad against g_A + g_B')


@pytest.mark.parametrize('fused', [True, False])
def test_forwards_first_backwards_in_reverse_order_with_dropout(fused):
    """Forward A, forward B, backward B, backward A at dropout 0.5: the stream advances once per forward and every backward uses the
    mask of its own forward (fused form: the sign of the saved dropped activation; tensor form: the saved mask)."""
    torch.manual_seed(SEED)
    m, batches = _hip(dropout=0.5)
    m.base.fused_dropout = fused
    H = HipHelpers()
    d = m.base.drop_state(batches[0]['image'].device)
    seed, step0 = d.get()
    out = T.sc_forwards_first(m, batches, H)
    assert d.get() == (seed, step0 + 2) and len(H.masks) == 2 and not torch.equal(H.masks[0][:1], H.masks[1])
    ref = _twin_run(T.sc_forwards_first, masks=H.masks)
    T.check_loss(out['loss_A'], ref['loss_A']); T.check_loss(out['loss_B'], ref['loss_B'])
    for key in ('grads_A', 'grads_B'):
        _report(f'forwards first {key} fused_dropout={fused}', out[key], ref[key])
        T.check_grads(out[key], ref[key])
    for which, key in ((0, 'grads_A'), (1, 'grads_B')):
        m2, b2 = _hip(dropout=0.5)
        m2.base.fused_dropout = fused
        m2.base.set_dropout_rng(seed, step0 + which, b2[0]['image'].device)
        alone = T.sc_single(m2, b2, HipHelpers(), which=which)['grads']
        _equal_bits(out[key], alone, f'{key} against the micro-batch run alone at dropout step {step0 + which}')


@pytest.mark.parametrize('frozen', [T.frozen_but_convdet, T.frozen_middle_fire, T.frozen_all])
def test_partially_frozen_models(frozen):
    m, batches = _hip()
    out = T.sc_frozen(m, batches, HipHelpers(), frozen)
    T.check_frozen(out['grads'], frozen)
    if frozen is T.frozen_all:
        assert out['pred_requires_grad'] is False and out['pred_grad_fn'] is None
        assert m.base.last_grad_flat is None
        return
    ref = _twin_cached(T.sc_single)
    names = {n for n, g in out['grads'].items() if g is not None}
    T.check_loss(out['loss'], ref['loss'])
    _report(f'{frozen.__name__}', out['grads'], ref['grads'], names=names)
    T.check_grads(out['grads'], ref['grads'], names=names)
    full = _hip_alone(0)
    _equal_bits({n: out['grads'][n] for n in names}, {n: full[n] for n in names}, 'a trainable gradient against the unfrozen run')


@pytest.mark.parametrize('kind', T.FOREIGN_KINDS)
def test_foreign_upstream_gradients_on_pred(kind):
    """Upstream gradients no loss kernel produced (expanded, zero on whole columns / images, non-contiguous, scaled by 2**10 and 2**-10).
    The bars: the project's own unless the float32 twin alone exceeds one (then 4x its measured error); both figures are printed."""
    ref = _twin_cached(T.sc_foreign, kind)['grads']
    meas32 = T.measure(_twin_cached(T.sc_foreign, kind, dtype=T.F32)['grads'], ref)
    bars = T.widened(meas32)
    print(f'autograd surface foreign {kind:10s} float32 twin vs float64 twin: convdet {meas32[0]:.2e}  max {meas32[1]:.2e}  '
          f'relL2 {meas32[2]:.2e}  -> bars used {bars}')
    m, batches = _hip()
    seen = []
    out = T.sc_foreign(m, batches, HipHelpers(), kind, hook=lambda g: seen.append((g.stride(), g.is_contiguous())))
    if kind == 'sum':
        assert seen and all(s == 0 for s in seen[0][0]), f'the scenario no longer hands an expanded gradient over: {seen}'
    if kind == 'transpose':
        assert seen and not seen[0][1], f'the scenario no longer hands a non-contiguous gradient over: {seen}'
    _report(f'foreign {kind}', out['grads'], ref, bars)
    T.check_grads(out['grads'], ref, bars)


def test_power_of_two_loss_scales_give_power_of_two_gradients():
    """``loss.mean() * 1024`` against ``loss.mean() * 2**-10``: every gradient element equal times 2**20, bit for bit, except where one
    of the two is subnormal or zero (the share of those was checked on the float32 twin: tests/test_autograd_twin_host.py)."""
    grads = {}
    for kind in ('x1024', 'x2^-10'):
        m, batches = _hip()
        grads[kind] = T.sc_foreign(m, batches, HipHelpers(), kind)['grads']
    excluded = total = 0
    for n, big in grads['x1024'].items():
        small = grads['x2^-10'][n]
        ok = T.scaled_pair_mask(big, small)
        excluded += int((~ok).sum()); total += ok.numel()
        assert torch.equal(big[ok], small[ok] * 2.0 ** 20), f'{n}: {int((big[ok] != small[ok] * 2.0 ** 20).sum())} elements differ'
    print(f'autograd surface scaled pair: {excluded} of {total} elements excluded ({100.0 * excluded / total:.4f} %)')
    assert excluded < 0.01 * total


def test_eval_mode_with_grad_enabled():
    """No dropout, no step advance; the gradients are the twin's without a mask."""
    torch.manual_seed(SEED)
    m, batches = _hip(dropout=0.5)
    d = m.base.drop_state(batches[0]['image'].device)
    state0 = d.get()
    H = HipHelpers()
    out = T.sc_eval_with_grad(m, batches, H)
    assert d.get() == state0 and not H.masks
    ref = _twin_cached(T.sc_single)
    T.check_loss(out['loss'], ref['loss'])
    _report('eval mode with grad', out['grads'], ref['grads'])
    T.check_grads(out['grads'], ref['grads'])


def test_train_mode_under_no_grad():
    """The mask is applied, the stream advances by one, nothing is saved."""
    torch.manual_seed(SEED)
    m, batches = _hip(dropout=0.5)
    d = m.base.drop_state(batches[0]['image'].device)
    seed, step0 = d.get()
    H = HipHelpers()
    out = T.sc_train_no_grad(m, batches, H)
    assert d.get() == (seed, step0 + 1) and len(H.masks) == 1
    assert out['requires_grad'] is False and out['grad_fn'] is None and m.base.last_grad_flat is None
    ref = _twin_run(T.sc_train_no_grad, masks=H.masks)
    T.check_loss(out['loss'], ref['loss'])
    plain = _twin_cached(T.sc_single)['loss']
    assert float((ref['loss'] - plain).abs().max()) > 1e-3 * float(plain.abs().max()), 'the mask does not move the loss: no teeth'


@pytest.mark.parametrize('which', ['class_loss', 'bbox_loss', 'mixture'])
@pytest.mark.parametrize('form', ['sparse', 'masked'])
def test_loss_components_of_the_sparse_and_masked_forms(form, which):
    """Backward through ``stats['class_loss']``, ``stats['bbox_loss']`` and a mixture with ``loss.mean()`` on ``LossSparseFn`` /
    ``LossMaskedFn`` (the dense form: test_training_gpu.py::test_loss_component_gradients)."""
    dens = 0.2 if form == 'masked' else None
    m, batches = _hip(form=form, ignore_density=dens)
    out = T.sc_loss_component(m, batches, HipHelpers(), which)
    ref = _twin_run(T.sc_loss_component, which, ignore_density=dens)
    T.check_loss(out['loss'], ref['loss'])
    _report(f'{form} {which}', out['grads'], ref['grads'])
    T.check_grads(out['grads'], ref['grads'])


def test_fused_clip_sgd_after_an_accumulation():
    """After A + B accumulated, ``base.last_grad_flat`` holds g_B alone and is NOT the buffer ``p.grad`` views: the optimizer must step
    on ``p.grad``.  (a) Against ``fp64_ref.clip_sgd`` on the snapshot of the accumulated ``p.grad`` at the bars of
    tests/test_fp64_optim_gpu.py (2^-18 M; norm 2^-18) -- those bars are relative to the operands handed to ``clip_sgd``.  (b) Against
    ``clip_sgd`` on the TWIN's accumulated gradients: there the gradient itself is only known to the flip-aware bars, so each
    parameter element is held to 2^-18 M plus what those bars let through the update, lr * coef * (bar * max|g| + 2e-2 |g|) (the
    second term: the clip coefficient moves with the norm, which the relative-L2 bar bounds)."""
    import test_fp64_optim_gpu as O
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    m, batches = _hip()
    opt = FusedClipSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=5.0, flat_grad=lambda: m.base.last_grad_flat)
    T.sc_accumulate(m, batches, HipHelpers(), 'plain')
    assert opt._flat_base([p.grad for p in opt.params]) is None, 'the flat-buffer path would read the last micro-batch alone'
    p0, g0, b0 = O._snap(opt)
    norm = opt.step()
    torch.cuda.synchronize()
    O._check_step(opt, p0, g0, b0, norm, 'after accumulation A(2)+B(1)')
    ref = _twin_cached(T.sc_accumulate, 'plain')['grads']
    names = [n for n, _ in m.named_parameters()]
    tn, coef, refp, _ = R.clip_sgd(p0, [ref[n] for n in names], b0, opt.lr, opt.momentum, opt.weight_decay, opt.max_norm)
    worst = 0.0
    for n, p, r in zip(names, opt.params, refp):
        g = ref[n].abs()
        bar_n = T.BAR_TIGHT if n in T.TIGHT_NAMES else T.BAR_MAX
        allow = R.BAR_L * r.M + opt.lr * coef * (bar_n * max(float(g.max()), 1e-3) + T.BAR_L2 * g)
        err = (p.detach().double().cpu() - r.ref64).abs()
        worst = max(worst, float((err / allow).max()))
        assert bool((err <= allow).all()), (n, float((err / allow).max()))
    print(f'autograd surface clip+SGD after accumulation vs twin gradients: norm {float(norm):.6e} (twin {tn:.6e}), worst err/allowance {worst:.2e}')
    assert abs(float(norm) - tn) <= T.BAR_L2 * tn


def frozen_convdet(name):
    return name.startswith('base.convdet.')


@pytest.mark.parametrize('frozen,flat_path', [(T.frozen_but_convdet, False), (T.frozen_middle_fire, False), (frozen_convdet, True)])
def test_fused_clip_sgd_on_a_partially_frozen_model(frozen, flat_path):
    """The optimizer holds the trainable parameters only.  With ConvDet frozen their gradients are still the leading consecutive views of
    the flat buffer, which is then longer than the optimizer's total (the one-reduction norm must stop at its own total); with other
    parameters frozen the views are not consecutive and the separate-gradient path runs.  fp64_ref.clip_sgd at the bars of
    tests/test_fp64_optim_gpu.py either way."""
    import test_fp64_optim_gpu as O
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    m, batches = _hip()
    T.sc_frozen(m, batches, HipHelpers(), frozen)
    opt = FusedClipSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=5.0, flat_grad=lambda: m.base.last_grad_flat)
    assert 0 < len(opt.params) < len(list(m.parameters()))
    flat = opt._flat_base([p.grad for p in opt.params])
    assert (flat is not None) == flat_path
    if flat is not None:
        assert flat.numel() > opt.total
    frozen_before = {n: p.detach().clone() for n, p in m.named_parameters() if not p.requires_grad}
    p0, g0, b0 = O._snap(opt)
    norm = opt.step()
    torch.cuda.synchronize()
    O._check_step(opt, p0, g0, b0, norm, f'frozen model, flat path {flat is not None}')
    for n, p in m.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p, frozen_before[n]), f'{n}: frozen, but changed by the step'


# ---- the three loud failures ---------------------------------------------------------------------------------------------------------------

def _no_launch_guard(monkeypatch):
    """The refusals are host side: no backward kernel may be launched by a refused call."""
    from squeezedet_pytorch_amd import backward as bw
    calls = []
    real = bw.run_backbone_backward
    monkeypatch.setattr(bw, 'run_backbone_backward', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize('name', [T.INPLACE_PARAM, 'base.features.3.squeeze.weight', 'base.convdet.weight'])
def test_inplace_parameter_update_between_forward_and_backward_raises(name, monkeypatch):
    m, batches = _hip()
    calls = _no_launch_guard(monkeypatch)
    out = {}
    rel = name.split('.', 1)[1]                       # (the node names the parameter relative to SqueezeDetBase)
    with pytest.raises(RuntimeError, match=f'modified by an inplace operation.* {rel} '):
        T.sc_inplace_update(m, batches, HipHelpers(), out, name=name)
    assert all(g is None for g in out['grads'].values()), 'a gradient was written'
    assert not calls
    # an optimizer step is such an update
    m, batches = _hip()
    loss, _ = m(batches[0])
    loss.mean().backward()
    loss2, _ = m(batches[0])
    torch.optim.SGD(m.parameters(), lr=1e-3).step()
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        loss2.mean().backward()


@pytest.mark.parametrize('via', ['loss', 'pred'])
@pytest.mark.parametrize('retain', [False, True])
def test_second_backward_through_the_same_forward_raises(retain, via, monkeypatch):
    """Through ``loss.mean()`` without ``retain_graph`` torch itself refuses at the loss node (its saved tensors are gone); in the other
    three cases the call reaches the backbone's node, which has freed its activations and says so."""
    m, batches = _hip()
    calls = _no_launch_guard(monkeypatch)
    out = {}
    with pytest.raises(RuntimeError, match='backward through the graph a second time') as e:
        T.sc_second_backward(m, batches, HipHelpers(), out, retain=retain, via=via)
    if retain or via == 'pred':
        assert 'frees its saved activations after the first backward' in str(e.value)
    assert len(calls) == 1
    assert all(g is not None for g in out['first'].values())
    _equal_bits(out['first'], out['second'], 'the first backward\'s gradients after the refused second one')
    if via == 'loss':
        _equal_bits(out['first'], _hip_alone(0), 'the first backward')


def test_image_that_requires_grad_raises():
    m, batches = _hip()
    out = {}
    with pytest.raises(RuntimeError, match='image requires grad'):
        T.sc_image_requires_grad(m, batches, HipHelpers(), out)
    assert not out and m.base.last_grad_flat is None
    # also with every parameter frozen (no autograd node at all), and not under no_grad
    T.sc_frozen(m, batches, HipHelpers(), T.frozen_all)
    img = batches[0]['image'].detach().clone().requires_grad_()
    with pytest.raises(RuntimeError, match='image requires grad'):
        m.base(img)
    with torch.no_grad():
        assert m.base(img).requires_grad is False
