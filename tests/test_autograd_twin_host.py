"""CPU tier of the autograd-surface tests: the float64 twin (tests/autograd_twin.py) is what tests/test_autograd_surface_gpu.py holds the
HIP model to, so it is checked here first -- against ``oracle.train_step_reference``, in every scenario on its own, for the torch
conventions the GPU tests rely on, and for teeth: the bars reject the three silent failures an autograd surface written by hand can
have (an accumulation that keeps the last micro-batch only, a backward that uses another forward's dropout mask, a frozen parameter
that gets zeros instead of no gradient)."""
import functools

import numpy as np
import pytest
import torch

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import synthetic

import autograd_twin as T

SIZE = T.SIZE


@functools.lru_cache(maxsize=None)
def _setup(arch='squeezedet', num_classes=3, ignore_density=None):
    cfg = sqd.make_cfg(arch=arch, input_size=SIZE, num_classes=num_classes)
    sd = synthetic.make_state_dict(arch, seed=1234, num_classes=num_classes)
    return cfg, sd, T.make_cases(cfg, num_classes, ignore_density)


def _twin(arch='squeezedet', num_classes=3, ignore_density=None, dtype=T.F64):
    cfg, sd, cases = _setup(arch, num_classes, ignore_density)
    return T.Twin(sd, cfg.anchors, SIZE, arch, num_classes, dtype).train(), T.twin_batches(cases, dtype), cfg, sd


def _mask_shapes(order, arch='squeezedet'):
    c = synthetic.convdet_in_channels(arch)
    return [(n, c, 4, 6) for n in order]


@pytest.mark.parametrize('arch', ['squeezedet', 'squeezedetplus'])
def test_twin_equals_the_oracle_train_step(arch):
    twin, batches, cfg, sd = _twin(arch)
    assert [n for n, _ in twin.named_parameters()] == list(sd.keys())
    out = T.sc_single(twin, batches, T.TwinHelpers())
    sd64 = {k: v.double() for k, v in sd.items()}
    x, gt = batches[0]['image'], batches[0]['gt']
    _, _, grads, _, loss_vec, _ = oracle.train_step_reference(sd64, None, x, gt, cfg.anchors.astype(np.float64), SIZE, arch=arch)
    np.testing.assert_allclose(out['loss'].numpy(), loss_vec.numpy(), rtol=1e-12)
    for n, g in out['grads'].items():
        np.testing.assert_allclose(g.numpy(), grads[n].numpy(), rtol=1e-12, atol=1e-300, err_msg=n)


def test_twin_takes_a_dropout_mask_and_returns_pred():
    twin, batches, cfg, sd = _twin()
    mask, = T.random_masks(_mask_shapes([2]), seed=9)
    loss, stats, pred = twin(batches[0], drop_mask=mask, want_pred=True)
    ref = oracle.backbone_forward(batches[0]['image'], {k: v.double() for k, v in sd.items()}, drop_mask=mask)
    assert torch.equal(pred.detach(), ref) and set(stats) == {'loss', 'class_loss', 'score_loss', 'bbox_loss'} and loss.shape == (2,)
    twin.eval()
    assert torch.equal(twin.predict(batches[0], mask).detach(), oracle.backbone_forward(batches[0]['image'], {k: v.double() for k, v in sd.items()}))


def test_masked_twin_is_the_reference_of_the_masked_launches():
    """The twin's loss with an ignore bitmap against tests/ignore_ref.py (the float64 reference the masked kernels are held to)."""
    import ignore_ref as IR
    twin, batches, cfg, sd = _twin(ignore_density=0.2)
    b = batches[0]
    assert b['ign'].any()
    loss, stats, pred = twin(b, want_pred=True)
    weights = (cfg.class_loss_weight, cfg.positive_score_loss_weight, cfg.negative_score_loss_weight, cfg.bbox_loss_weight)
    ref = IR.masked_loss(pred.detach().float(), b['gt'].float(), b['ign'], torch.from_numpy(cfg.anchors).float(), SIZE, 3, weights)
    p32 = pred.detach().float().double().requires_grad_(True)               # (the reference reads pred rounded to float32)
    l32, st32 = twin.loss_of(p32, b)
    got = torch.stack([st32['class_loss'], st32['score_loss'], st32['bbox_loss'], l32]).detach()
    np.testing.assert_allclose(got.numpy(), ref['losses'].ref64.numpy(), rtol=1e-9)
    assert float((loss - l32).detach().abs().max()) <= 1e-5 * float(loss.detach().abs().max())


# ---- every scenario on the twin alone ------------------------------------------------------------------------------------------------------

def _sum_of_singles(which=(0, 1)):
    total = None
    for w in which:
        twin, batches, _, _ = _twin()
        g = T.sc_single(twin, batches, T.TwinHelpers(), which=w)['grads']
        total = g if total is None else {n: total[n] + g[n] for n in g}
    return total


@pytest.mark.parametrize('mode', ['plain', 'zero_first', 'mean'])
def test_scenario_accumulate(mode):
    twin, batches, _, _ = _twin()
    out = T.sc_accumulate(twin, batches, T.TwinHelpers(), mode)
    want = _sum_of_singles()
    for n, g in out['grads'].items():
        np.testing.assert_allclose(g.numpy(), want[n].numpy(), rtol=1e-12, atol=1e-300, err_msg=n)
    assert out['loss_A'].shape == (2,) and out['loss_B'].shape == (1,)


def _forwards_first(masks):
    twin, batches, _, _ = _twin()
    return T.sc_forwards_first(twin, batches, T.TwinHelpers(masks))


def test_scenario_forwards_first_and_its_teeth():
    mA, mB = T.random_masks(_mask_shapes([2, 1]), seed=21)
    out = _forwards_first([mA, mB])
    for which, mask, key in ((0, mA, 'grads_A'), (1, mB, 'grads_B')):
        twin, batches, _, _ = _twin()
        alone = T.sc_single(twin, batches, T.TwinHelpers([mask]), which=which)['grads']
        for n, g in out[key].items():
            assert torch.equal(g, alone[n]), n
    # teeth: each backward with the mask of the OTHER step of the stream (the shapes differ, so the step's draw at the own shape)
    sA, sB = T.random_masks(_mask_shapes([1, 2]), seed=21)          # the same stream read in the other order
    wrong = _forwards_first([sB, sA])
    for key in ('grads_A', 'grads_B'):
        with pytest.raises(AssertionError):
            T.check_grads(wrong[key], out[key])
        T.check_grads(out[key], out[key])


def test_teeth_accumulation_that_keeps_the_last_micro_batch():
    want = _sum_of_singles()
    last_only = _sum_of_singles(which=(1,))
    with pytest.raises(AssertionError):
        T.check_grads(last_only, want)
    T.check_grads(want, want)


@pytest.mark.parametrize('frozen', [T.frozen_but_convdet, T.frozen_middle_fire, T.frozen_all])
def test_scenario_frozen_and_its_teeth(frozen):
    twin, batches, _, _ = _twin()
    out = T.sc_frozen(twin, batches, T.TwinHelpers(), frozen)
    T.check_frozen(out['grads'], frozen)
    if frozen is T.frozen_all:
        assert out['pred_requires_grad'] is False and out['pred_grad_fn'] is None
        return
    full = _sum_of_singles(which=(0,))
    for n, g in out['grads'].items():
        if g is not None:
            assert torch.equal(g, full[n]), n                        # a trainable parameter's gradient does not depend on who else trains
    # teeth: zeros instead of no gradient
    zeroed = {n: (torch.zeros_like(full[n]) if g is None else g) for n, g in out['grads'].items()}
    with pytest.raises(AssertionError):
        T.check_frozen(zeroed, frozen)


@functools.lru_cache(maxsize=None)
def _foreign(kind, dtype):
    twin, batches, _, _ = _twin(dtype=dtype)
    strides = []
    out = T.sc_foreign(twin, batches, T.TwinHelpers(), kind, hook=lambda g: strides.append(g.stride()))
    return out['grads'], strides


@pytest.mark.parametrize('kind', T.FOREIGN_KINDS)
def test_scenario_foreign_gradients_float32_twin_against_float64(kind):
    """The float32 chain's own error in each foreign-gradient scenario: what the GPU tier's bars are widened from when it exceeds them
    (autograd_twin.widened).  Printed, so the figure is in the test log."""
    g64, strides = _foreign(kind, T.F64)
    g32, _ = _foreign(kind, T.F32)
    meas = T.measure(g32, g64)
    print(f'foreign {kind:10s} float32 twin vs float64 twin: convdet {meas[0]:.2e}  max {meas[1]:.2e}  relL2 {meas[2]:.2e}  -> bars {T.widened(meas)}')
    assert all(np.isfinite(m) for m in meas) and all(float(g.abs().max()) > 0 for g in g64.values())
    if kind == 'sum':
        assert strides and all(s == 0 for s in strides[0]), f'pred.sum() no longer hands an expanded gradient over: {strides}'
    if kind == 'image0':
        twin, batches, _, _ = _twin()
        only0 = [{k: (v[:1] if isinstance(v, torch.Tensor) else v) for k, v in batches[0].items()}]
        g0 = T.sc_foreign(twin, only0, T.TwinHelpers(), kind)['grads']
        for n in g0:
            np.testing.assert_allclose(g0[n].numpy(), g64[n].numpy(), rtol=1e-12, atol=1e-12 * float(g64[n].abs().max()))   # image 1 contributes nothing


def test_scaled_upstream_gradients_are_exact_powers_of_two_apart():
    """``loss.mean() * 1024`` against ``loss.mean() * 2**-10`` in float32: equal times 2**20 wherever neither is zero or subnormal, and
    those excluded elements are below 1 % of all (the GPU tier asserts the same equality bit for bit on the kernels)."""
    big, _ = _foreign('x1024', T.F32)
    small, _ = _foreign('x2^-10', T.F32)
    excluded = both_zero = total = 0
    for n in big:
        ok = T.scaled_pair_mask(big[n], small[n])
        excluded += int((~ok).sum()); total += ok.numel()
        both_zero += int(((big[n] == 0) & (small[n] == 0)).sum())
        assert torch.equal(big[n][ok], small[n][ok] * 2.0 ** 20), n
    print(f'scaled pair: {both_zero} of {total} elements are zero in both runs ({100.0 * both_zero / total:.2f} %: dead ReLU channels), '
          f'{excluded} excluded as subnormal or zero in one run only ({100.0 * excluded / total:.4f} %)')
    assert excluded < 0.01 * total


def test_scenario_eval_with_grad_and_train_no_grad():
    mask, = T.random_masks(_mask_shapes([2]), seed=5)
    twin, batches, _, _ = _twin()
    H = T.TwinHelpers([mask])
    out = T.sc_eval_with_grad(twin, batches, H)
    assert len(H.masks) == 1, 'eval mode consumed a mask'
    plain = _sum_of_singles(which=(0,))
    for n, g in out['grads'].items():
        assert torch.equal(g, plain[n]), n
    twin, batches, _, _ = _twin()
    H = T.TwinHelpers([mask])
    ng = T.sc_train_no_grad(twin, batches, H)
    assert not H.masks and ng['requires_grad'] is False and ng['grad_fn'] is None
    assert not torch.equal(ng['loss'], out['loss']), 'the mask was not applied'


@pytest.mark.parametrize('which', ['class_loss', 'bbox_loss', 'mixture'])
def test_scenario_loss_components_masked_form(which):
    twin, batches, _, _ = _twin(ignore_density=0.2)
    out = T.sc_loss_component(twin, batches, T.TwinHelpers(), which)
    assert all(g is not None and torch.isfinite(g).all() for g in out['grads'].values())
    assert float(out['grads']['base.convdet.weight'].abs().max()) > 0


# ---- the torch conventions the GPU tier relies on ------------------------------------------------------------------------------------------

def test_torch_raises_on_an_inplace_parameter_update_before_backward():
    twin, batches, _, _ = _twin()
    out = {}
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        T.sc_inplace_update(twin, batches, T.TwinHelpers(), out)
    # (torch has written the gradients of the layers behind the modified one by then; the HIP model's backbone is ONE node, which
    # refuses before its first launch, so there no gradient at all is written -- asserted on the GPU tier)
    assert out['grads'][T.INPLACE_PARAM] is None


@pytest.mark.parametrize('via', ['loss', 'pred'])
def test_torch_second_backward_conventions(via):
    twin, batches, _, _ = _twin()
    out = {}
    with pytest.raises(RuntimeError, match='backward through the graph a second time'):
        T.sc_second_backward(twin, batches, T.TwinHelpers(), out, retain=False, via=via)
    assert all(g is not None for g in out['first'].values())
    twin, batches, _, _ = _twin()
    out = {}
    T.sc_second_backward(twin, batches, T.TwinHelpers(), out, retain=True, via=via)
    for n in out['first']:
        assert torch.equal(out['second'][n], 2.0 * out['first'][n]), n


def test_torch_gives_the_image_a_gradient():
    """What the HIP model cannot do (its backward ends at the stem's weight gradient) and therefore refuses loudly."""
    twin, batches, _, _ = _twin()
    out = {}
    T.sc_image_requires_grad(twin, batches, T.TwinHelpers(), out)
    assert out['image_grad'] is not None and float(out['image_grad'].abs().max()) > 0


def test_backbone_node_refusals_are_host_side():
    """The three refusals of ``BackboneFn`` / ``backbone_apply`` sit in front of every launch: they need no device.  (The GPU tier runs
    them through the whole module.)"""
    from squeezedet_pytorch_amd import backward as bw
    from squeezedet_pytorch_amd.autograd import backbone_apply
    from squeezedet_pytorch_amd.model import SqueezeDetBase
    base = SqueezeDetBase(sqd.make_cfg(input_size=SIZE))
    with pytest.raises(RuntimeError, match='image requires grad'):
        backbone_apply(base, torch.zeros(1, 3, 64, 96, requires_grad=True))
    params = [p for _, p in base.named_parameters()]
    names = [n for n, _ in base.named_parameters()]

    class Ctx:
        pass
    ctx = Ctx()
    ctx.base, ctx.saved, ctx.names, ctx.params, ctx.param_state = base, {}, names, params, bw._param_state(params)
    with torch.no_grad():
        params[5].add_(1.0)
    with pytest.raises(RuntimeError, match=f'modified by an inplace operation: parameter {names[5]} '):
        bw.BackboneFn.backward(ctx, torch.zeros(1, 4, 6, 72))
    ctx.saved = None
    with pytest.raises(RuntimeError, match='backward through the graph a second time.*freed|backward through the graph a second time.*frees'):
        bw.BackboneFn.backward(ctx, torch.zeros(1, 4, 6, 72))
