"""CPU tier: the surface of the loss stack that its shared bodies must not move -- the parameter lists of the public ``ops.loss_*``
wrappers, what ``ops.loss_fns`` returns, the ``forward`` / ``backward`` parameter lists of the six ``backward.Loss*Fn`` classes (the
module code calls them positionally), and the upstream-operand checks of the backward wrappers: a bad ``coef``, ``gmean``, ``nobj`` or
``counts`` raises ``ValueError`` before the library is touched, a good one goes on to the library."""
import inspect

import pytest
import torch

from squeezedet_pytorch_amd import _native as nat
from squeezedet_pytorch_amd import backward, ops
import test_fp64_loss_gpu as L

TAIL = ['input_size', 'num_classes', 'weights']
DENSE, SPARSE, MASKED = ['pred', 'gt', 'anchors'], ['pred', 'sgt', 'anchors'], ['pred', 'sgt', 'ignore', 'anchors']
SIGNATURES = {
    'loss_fwd': DENSE + TAIL, 'loss_mean_fwd': DENSE + TAIL,
    'loss_bwd': DENSE + ['nobj', 'coef'] + TAIL, 'loss_mean_bwd': DENSE + ['nobj', 'gmean'] + TAIL,
    'loss_fwd_many': DENSE + TAIL, 'loss_mean_fwd_many': DENSE + TAIL,
    'loss_bwd_many': DENSE + ['nobj', 'coef'] + TAIL, 'loss_mean_bwd_many': DENSE + ['nobj', 'gmean'] + TAIL,
    'loss_sparse_fwd': SPARSE + TAIL, 'loss_sparse_mean_fwd': SPARSE + TAIL,
    'loss_sparse_bwd': SPARSE + ['nobj', 'coef'] + TAIL, 'loss_sparse_mean_bwd': SPARSE + ['nobj', 'gmean'] + TAIL,
    'loss_masked_fwd': MASKED + TAIL, 'loss_masked_mean_fwd': MASKED + TAIL,
    'loss_masked_bwd': MASKED + ['counts', 'coef'] + TAIL + ['out'], 'loss_masked_mean_bwd': MASKED + ['counts', 'gmean'] + TAIL + ['out'],
}


@pytest.mark.parametrize('name', sorted(SIGNATURES))
def test_wrapper_signature(name):
    params = inspect.signature(getattr(ops, name)).parameters
    assert list(params) == SIGNATURES[name]
    for p in params.values():
        assert p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
        if p.name == 'out':
            assert p.default is None
        else:
            assert p.default is inspect.Parameter.empty


def test_loss_fns_order():
    assert ops.loss_fns(3) == (ops.loss_fwd, ops.loss_mean_fwd, ops.loss_bwd, ops.loss_mean_bwd)
    assert ops.loss_fns(80) == (ops.loss_fwd_many, ops.loss_mean_fwd_many, ops.loss_bwd_many, ops.loss_mean_bwd_many)


FUNCTIONS = {
    'LossFn': (['ctx', 'pred', 'gt', 'anchors', 'loss_mod'], None, ['ctx', 'g']),
    'LossMeanFn': (['ctx', 'pred', 'gt', 'anchors', 'loss_mod'], None, ['ctx', 'g', '_gl']),
    'LossSparseFn': (['ctx', 'pred', 'anchors', 'loss_mod'], 'sgt', ['ctx', 'g']),
    'LossSparseMeanFn': (['ctx', 'pred', 'anchors', 'loss_mod'], 'sgt', ['ctx', 'g', '_gl']),
    'LossMaskedFn': (['ctx', 'pred', 'anchors', 'loss_mod', 'ignore'], 'sgt', ['ctx', 'g']),
    'LossMaskedMeanFn': (['ctx', 'pred', 'anchors', 'loss_mod', 'ignore'], 'sgt', ['ctx', 'g', '_gl']),
}


@pytest.mark.parametrize('name', sorted(FUNCTIONS))
def test_autograd_function_signature(name):
    fn = getattr(backward, name)
    assert isinstance(fn, type) and issubclass(fn, torch.autograd.Function)
    positional, var, bwd = FUNCTIONS[name]
    params = list(inspect.signature(fn.forward).parameters.values())
    assert [p.name for p in params if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD] == positional
    assert [p.name for p in params if p.kind is inspect.Parameter.VAR_POSITIONAL] == ([var] if var else [])
    assert len(params) == len(positional) + (1 if var else 0)
    assert list(inspect.signature(fn.backward).parameters) == bwd


B, A, C = 2, 30, 3


def _bad_upstream():
    """(wrapper, which operand, its bad value): what each backward wrapper refuses.  The dense wrappers look at shapes only (and the
    dense mean backward does not look at nobj); the sparse ones also at nobj's dtype; the masked ones also refuse what is no tensor
    and a coef on another device."""
    coef_shape, nobj_shape = torch.ones(2, B), torch.ones(B + 1)
    gmean_two, gmean_f64 = torch.ones(2), torch.ones(1, dtype=torch.float64)
    for name in ('loss_bwd', 'loss_bwd_many'):
        yield name, 'coef', coef_shape
        yield name, 'nobj', nobj_shape
    for name in ('loss_mean_bwd', 'loss_mean_bwd_many'):
        yield name, 'gmean', gmean_two
        yield name, 'gmean', gmean_f64
    yield 'loss_sparse_bwd', 'coef', coef_shape
    yield 'loss_sparse_bwd', 'nobj', nobj_shape
    yield 'loss_sparse_bwd', 'nobj', torch.ones(B, dtype=torch.float64)
    yield 'loss_sparse_mean_bwd', 'gmean', gmean_two
    yield 'loss_sparse_mean_bwd', 'gmean', gmean_f64
    yield 'loss_sparse_mean_bwd', 'nobj', nobj_shape
    yield 'loss_sparse_mean_bwd', 'nobj', torch.ones(B, dtype=torch.float64)
    for name in ('loss_masked_bwd', 'loss_masked_mean_bwd'):
        yield name, 'counts', torch.ones(B)
        yield name, 'counts', torch.ones(2, B, dtype=torch.float64)
        yield name, 'counts', torch.ones(2, B, device='meta')
        yield name, 'counts', [[1.0] * B] * 2
    yield 'loss_masked_bwd', 'coef', coef_shape
    yield 'loss_masked_bwd', 'coef', torch.ones(3, B, device='meta')
    yield 'loss_masked_bwd', 'coef', None
    yield 'loss_masked_mean_bwd', 'gmean', gmean_two
    yield 'loss_masked_mean_bwd', 'gmean', gmean_f64
    yield 'loss_masked_mean_bwd', 'gmean', torch.ones(1, device='meta')
    yield 'loss_masked_mean_bwd', 'gmean', 1.0


def test_upstream_operands_are_checked_before_the_library(monkeypatch):
    class Reached(Exception):
        pass

    def no_library():
        raise Reached()
    monkeypatch.setattr(nat, 'lib', no_library)
    pred, gt, anchors = L.random_case(B, A, C, seed=5)
    sgt = ops.sparse_gt_from_dense(gt)
    total = sgt.anchor_idx.shape[0]
    ignore = torch.zeros(B, ops.ignore_words(A), dtype=torch.int32)
    # the operands live on the CPU, where the geometry checks would stop every call at "pred must be on the GPU": stand in for
    # them, so that a call gets as far as its upstream operands
    monkeypatch.setattr(ops, '_check_loss_args', lambda *a: (B, A))
    monkeypatch.setattr(ops, '_check_sparse_loss_args', lambda *a: (B, A, total, sgt))
    monkeypatch.setattr(ops, '_check_masked_loss_args', lambda *a: (B, A, total, sgt, ignore))
    good = {'nobj': torch.ones(B), 'counts': torch.ones(2, B), 'coef': torch.ones(3, B), 'gmean': torch.ones(1)}

    def call(name, **bad):
        operands = [pred, gt, anchors] if SIGNATURES[name][:3] == DENSE else [pred, sgt, ignore, anchors] if 'ignore' in SIGNATURES[name] \
            else [pred, sgt, anchors]
        upstream = [bad.get(k, good[k]) for k in SIGNATURES[name][len(operands):len(operands) + 2]]
        return getattr(ops, name)(*operands, *upstream, L.SIZE, C, L.WEIGHTS)

    backward_wrappers = [n for n in SIGNATURES if n.endswith('bwd') or n.endswith('bwd_many')]
    assert len(backward_wrappers) == 8
    for name in backward_wrappers:                 # good operands get past the checks
        with pytest.raises(Reached):
            call(name)
    seen = set()
    for name, which, value in _bad_upstream():
        with pytest.raises(ValueError, match=which):
            call(name, **{which: value})
        seen.add(name)
    assert seen == set(backward_wrappers)
