"""CPU tier: the host side of the sparse ground truth (``ops.SparseGT``): the torch-only converters, the argument checks of the four
``ops.loss_sparse_*`` wrappers (every one raises before the library is touched), the launch plan's ``sparse_gt`` switch, the four
C-ABI entries in the header and the ctypes table, and the collate helper's pass-through of dense batches."""
import os
import re

import pytest
import torch

import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import _native as nat
from squeezedet_pytorch_amd import ops, plan
from squeezedet_pytorch_amd.trainer import encode_sparse_batch
import test_fp64_loss_gpu as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('sqd_loss_sparse_fwd', 'sqd_loss_sparse_mean_fwd', 'sqd_loss_sparse_bwd', 'sqd_loss_sparse_mean_bwd')


def test_converters_round_trip():
    B, A, C = 3, 1000, 20
    _, gt, _ = L.random_case(B, A, C, seed=777, nobj=[1, 999, 160])
    sgt = ops.sparse_gt_from_dense(gt)
    assert isinstance(sgt, ops.SparseGT) and sgt._fields == ('anchor_idx', 'boxes', 'deltas', 'class_ids', 'offsets')
    assert sgt.offsets.tolist() == [0, 1, 1000, 1160]
    assert sgt.anchor_idx.dtype == sgt.class_ids.dtype == sgt.offsets.dtype == torch.int32
    assert sgt.boxes.dtype == sgt.deltas.dtype == torch.float32 and tuple(sgt.boxes.shape) == tuple(sgt.deltas.shape) == (1160, 4)
    for b in range(B):
        idx = sgt.anchor_idx[sgt.offsets[b]:sgt.offsets[b + 1]]
        assert bool((idx[1:] > idx[:-1]).all())                      # ascending anchor order
        assert torch.equal(idx.long(), torch.nonzero(gt[b, :, 0] > 0).flatten())
    assert torch.equal(sgt.class_ids.long(), gt[gt[..., 0] > 0][:, 9:].argmax(1))
    back = ops.sparse_gt_to_dense(sgt, A, C)
    assert back.dtype == torch.float32 and torch.equal(back, gt)
    # an out-of-range anchor index (the encoder's "unassigned" value A, or a negative one) is dropped; a class id outside [0, C)
    # leaves the one-hot empty
    free = int(torch.nonzero(gt[0, :, 0] == 0)[0])
    extra = ops.SparseGT(torch.cat([torch.tensor([A, -1, free], dtype=torch.int32), sgt.anchor_idx]),
                         torch.cat([torch.tensor([[1., 2., 3., 4.]] * 3), sgt.boxes]), torch.cat([torch.full((3, 4), .5), sgt.deltas]),
                         torch.cat([torch.tensor([0, 1, C], dtype=torch.int32), sgt.class_ids]),
                         sgt.offsets + torch.tensor([0, 3, 3, 3], dtype=torch.int32))
    want = gt.clone()
    want[0, free, :9] = torch.tensor([1., 1., 2., 3., 4., .5, .5, .5, .5])
    assert torch.equal(ops.sparse_gt_to_dense(extra, A, C), want)
    # no positives at all
    empty = ops.sparse_gt_from_dense(torch.zeros(2, 5, 12))
    assert empty.offsets.tolist() == [0, 0, 0] and empty.anchor_idx.numel() == 0 and tuple(empty.boxes.shape) == (0, 4)
    assert torch.equal(ops.sparse_gt_to_dense(empty, 5, 3), torch.zeros(2, 5, 12))


def _good(B=2, A=30, C=3):
    pred, gt, anchors = L.random_case(B, A, C, seed=5)
    return pred, ops.sparse_gt_from_dense(gt), anchors


def _bad_operands():
    """(what is wrong, pred, sgt, anchors, C): one broken operand each; everything lives on the CPU, so a call that got past the
    checks would stop at the device check -- still a ValueError, still before the library."""
    pred, sgt, anchors = _good()
    n = sgt.anchor_idx.shape[0]
    yield 'all on the CPU', pred, sgt, anchors, 3
    yield 'pred dtype', pred.double(), sgt, anchors, 3
    yield 'pred width', pred[..., :7], sgt, anchors, 3
    yield 'pred rank', pred[0], sgt, anchors, 3
    yield 'class count', pred, sgt, anchors, 0
    yield 'not a SparseGT', pred, tuple(sgt), anchors, 3
    yield 'dense gt given', pred, torch.zeros(2, 30, 12), anchors, 3
    yield 'anchor_idx dtype', pred, sgt._replace(anchor_idx=sgt.anchor_idx.long()), anchors, 3
    yield 'boxes dtype', pred, sgt._replace(boxes=sgt.boxes.double()), anchors, 3
    yield 'deltas dtype', pred, sgt._replace(deltas=sgt.deltas.half()), anchors, 3
    yield 'class_ids dtype', pred, sgt._replace(class_ids=sgt.class_ids.long()), anchors, 3
    yield 'offsets dtype', pred, sgt._replace(offsets=sgt.offsets.long()), anchors, 3
    yield 'offsets shape', pred, sgt._replace(offsets=sgt.offsets[:-1]), anchors, 3
    yield 'offsets shape (B+2)', pred, sgt._replace(offsets=torch.cat([sgt.offsets, sgt.offsets[-1:]])), anchors, 3
    yield 'boxes total', pred, sgt._replace(boxes=sgt.boxes[:-1]), anchors, 3
    yield 'deltas total', pred, sgt._replace(deltas=torch.zeros(n + 1, 4)), anchors, 3
    yield 'class_ids total', pred, sgt._replace(class_ids=sgt.class_ids[1:]), anchors, 3
    yield 'boxes width', pred, sgt._replace(boxes=torch.zeros(n, 5)), anchors, 3
    yield 'anchor_idx rank', pred, sgt._replace(anchor_idx=sgt.anchor_idx.view(-1, 1)), anchors, 3
    yield 'anchors shape', pred, sgt, anchors[:-1], 3
    yield 'anchors dtype', pred, sgt, anchors.double(), 3


def test_argument_checks_raise_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError('an argument check let a bad operand through to the library')
    monkeypatch.setattr(nat, 'lib', no_library)
    nobj, coef, gmean = torch.ones(2), torch.ones(3, 2), torch.ones(1)
    seen = 0
    for what, pred, sgt, anchors, C in _bad_operands():
        for call in (lambda: ops.loss_sparse_fwd(pred, sgt, anchors, L.SIZE, C, L.WEIGHTS),
                     lambda: ops.loss_sparse_mean_fwd(pred, sgt, anchors, L.SIZE, C, L.WEIGHTS),
                     lambda: ops.loss_sparse_bwd(pred, sgt, anchors, nobj, coef, L.SIZE, C, L.WEIGHTS),
                     lambda: ops.loss_sparse_mean_bwd(pred, sgt, anchors, nobj, gmean, L.SIZE, C, L.WEIGHTS)):
            with pytest.raises(ValueError):
                call()
            seen += 1
    assert seen == 4 * 21
    with pytest.raises(ValueError, match='256'):
        ops.loss_sparse_fwd(torch.zeros(1, 4, 262), _good()[1], torch.zeros(4, 4), L.SIZE, 257, L.WEIGHTS)


@pytest.mark.parametrize('C', [3, 80])
def test_launch_plan_switch(C):
    base = plan.training_launch_plan(num_classes=C)
    assert base == plan.training_launch_plan(num_classes=C, sparse_gt=False)
    sparse = plan.training_launch_plan(num_classes=C, sparse_gt=True)
    assert len(sparse) == len(base)
    diff = [(a, b) for a, b in zip(base, sparse) if a != b]
    A = 24 * 78 * 9
    assert diff == [(('loss_fwd', f'loss A{A}'), ('loss_sparse_fwd', f'loss A{A}')),
                    (('loss_bwd', f'lossbwd A{A}'), ('loss_sparse_bwd', f'lossbwd A{A}'))]
    if C == 3:
        assert plan.training_launch_plan() == base


def test_header_and_ctypes_table_carry_the_entries():
    txt = open(os.path.join(ROOT, 'include', 'sqd_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name in ENTRIES:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, f'{name} is not declared in include/sqd_hip.h'
        args = [a.strip() for a in m.group(1).split(',')]
        assert name in nat._SIGNATURES and len(nat._SIGNATURES[name]) == len(args)
        for want in ('anchor_idx', 'boxes', 'deltas', 'class_ids', 'offsets', 'int total'):
            assert any(a.endswith(want) for a in args), (name, want)
        assert not any(a.endswith(' gt') or a.endswith('*gt') for a in args)


@pytest.mark.parametrize('flag', [False, True])
def test_collate_passes_dense_batches_through(flag):
    cfg = sqd.make_cfg(input_size=(64, 96), device='cpu')
    assert cfg.sparse_gt is False
    cfg.sparse_gt = flag
    batch = {'image': torch.zeros(1, 3, 64, 96), 'gt': torch.zeros(1, cfg.num_anchors, 12), 'image_meta': {}}
    assert encode_sparse_batch(batch, cfg) is batch
    both = dict(batch, gt_boxes=[[[1., 2., 30., 40.]]], gt_class_ids=[[0]])
    assert encode_sparse_batch(both, cfg) is both
    plain = {'image': torch.zeros(1, 3, 64, 96)}
    assert encode_sparse_batch(plain, cfg) is plain
