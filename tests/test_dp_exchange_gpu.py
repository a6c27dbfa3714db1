"""GPU tier: the device ("native") branch of ``GradientExchange`` held, element by element, to the count-weighted mean of the ranks'
local gradients (tests/dp_exchange_ref.py): ``|got - expected| <= 2^-18 M`` on EVERY element of the flat buffer, exactly 0 where
``M == 0``.  ``expected = (sum_r b_r g_r) / sum_r b_r`` in float64, ``g_r`` = rank r's own gradient of its local mean with no exchange
attached -- so no model reference and none of its ReLU-flip noise enters, and a forgotten ``scale`` (the staged slab reduction, the
padded ConvDet's row reduction, ``scale_slice`` for the stem), a wrong bucket boundary or a wrong divisor is five orders of magnitude
outside (tests/test_dp_exchange_host.py has the mutants).

One process: ``StubDist`` stands in for ``torch.distributed`` and adds the peers' prepared buffer in ``all_reduce`` on whatever stream
the exchange issues it.  64x96 input (grid 4x6), synthetic weights, dropout off.  Preconditions asserted, not assumed: ``g_r`` is
bit-identical run to run, and the staged reduce at ``scale = 1`` is bitwise the one-launch reduce.

Kernel level: ``WgradBatch.reduce`` over every split of a four-layer table (bitwise at scale 1, exactly ``fl32(sum * scale)`` at 3 and
5, inside NaN guard bands), ``ops.wgrad_reduce_rows`` with a scale, and ``sqd_grad_scale`` on both sides of the size where its
grid-stride loop starts."""
import functools

import numpy as np
import pytest
import torch

import dp_exchange_ref as X

pytestmark = pytest.mark.gpu
SIZE = (64, 96)
GUARD = 7

MATCH = dict(sparse_gt=True, ignore_overlap=0.5, match_iou=0.5, match_ignore_iou=0.4, bbox_loss='giou')
CASES = {
    'squeezedet_3_2': dict(shards=(3, 2)),
    'squeezedet_1_4': dict(shards=(1, 4)),
    'squeezedet_2_1_1': dict(shards=(2, 1, 1)),
    'squeezedetplus_2_1': dict(arch='squeezedetplus', shards=(2, 1)),
    'classes20_sparse_1_3': dict(C=20, shards=(1, 3), cfg=dict(sparse_gt=True)),
    'masked_match_giou_3_2': dict(shards=(3, 2), cfg=MATCH),
    'unfused_squeeze_bwd_3_2': dict(shards=(3, 2), base=dict(fuse_squeeze_bwd=False)),
    'ungrouped_wgrad_3_2': dict(shards=(3, 2), base=dict(group_wgrad=False)),
    'no_overlap_3_2': dict(shards=(3, 2), overlap=False),
}


def _batches(cfg, C, shards, seed_img=3, seed_gt=2):
    """One batch per shard of the same global batch (images seed 3, boxes seed 2: the operands of tests/test_data_parallel_gpu.py)."""
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.annotations import encode_annotations
    B = sum(shards)
    x = synthetic.make_images(B, SIZE, seed=seed_img)
    sparse = bool(getattr(cfg, 'sparse_gt', False))
    if not sparse:
        gt = synthetic.make_gt(B, cfg.anchors, SIZE, C, seed=seed_gt, min_boxes=2, max_boxes=3)
    else:
        cls_list, box_list = synthetic.make_gt_boxes(B, SIZE, C, seed=seed_gt, min_boxes=2, max_boxes=3)
    out, lo = [], 0
    for b in shards:
        batch = {'image': x[lo:lo + b].cuda()}
        if not sparse:
            batch['gt'] = gt[lo:lo + b].cuda()
        elif cfg.match_iou is None:
            batch['gt_sparse'] = encode_annotations(cls_list[lo:lo + b], box_list[lo:lo + b], cfg.anchors, C, dense=False)
        else:
            ign = [np.array([[0., 0., 95., 20.]], np.float32)] * b              # the anchors lying to one half on the upper rows
            sgt, bitmap = encode_annotations(cls_list[lo:lo + b], box_list[lo:lo + b], cfg.anchors, C, dense=False, ignore_boxes_list=ign,
                                             ignore_overlap=cfg.ignore_overlap, match=(cfg.match_iou, cfg.match_ignore_iou, cfg.match_max_extra))
            batch['gt_sparse'], batch['gt_ignore'] = sgt, bitmap
        out.append(batch)
        lo += b
    return out


def _model(arch='squeezedet', C=3, cfg_kw=None, base_kw=None):
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    cfg = sqd.make_cfg(arch=arch, input_size=SIZE, num_classes=C, dropout_prob=0.0, device='cuda', **(cfg_kw or {}))
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict(arch, seed=1234, num_classes=C))
    m = m.cuda().train()
    for k, v in (base_kw or {}).items():
        assert hasattr(m.base, k), k
        setattr(m.base, k, v)
    return cfg, m


def _backward(m, batch):
    """zero_grad -> forward -> loss.mean().backward() -> the flat gradient buffer (not a copy)."""
    m.zero_grad()
    loss, _ = m(batch)
    loss.mean().backward()
    torch.cuda.synchronize()
    return m.base.last_grad_flat


def _local_gradients(m, batches):
    """Every shard's gradient of its local mean with no exchange attached, run twice: bit-identical, or the expectation has no footing."""
    assert getattr(m.base, 'grad_sync', None) is None
    out = []
    for r, batch in enumerate(batches):
        first = _backward(m, batch).clone()
        again = _backward(m, batch)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32)), \
            f'shard {r}: the local gradient differs run to run in {int((first != again).sum())} elements'
        assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
        out.append(first)
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (model, batches, local gradients, slots, total): shared by the two ranks a case is seen from."""
    c = CASES[name]
    C = c.get('C', 3)
    cfg, m = _model(c.get('arch', 'squeezedet'), C, c.get('cfg'), c.get('base'))
    batches = _batches(cfg, C, c['shards'])
    g = _local_gradients(m, batches)
    slots, total = X.make_slots([(n, p.shape) for n, p in m.base.named_parameters()])
    assert total == g[0].numel()
    return m, batches, g, slots, total


def _exchanged(m, batch, shards, rank, g, monkeypatch, overlap=True, optimizer=None):
    """One backward of ``batch`` as rank ``rank`` with the stub's peers -> (flat gradient, stub, exchange); the model stays attached."""
    from squeezedet_pytorch_amd.exchange import attach_data_parallel
    stub = X.install(monkeypatch, X.StubDist(len(shards), rank))
    stub.prepare([g[r] for r in range(len(shards)) if r != rank], [shards[r] for r in range(len(shards)) if r != rank])
    ex = attach_data_parallel(m, optimizer, overlap=overlap, broadcast=False, seed_offset=False)
    assert ex is not None and m.base.grad_sync is ex and ex.world() == len(shards)
    got = _backward(m, batch)
    assert ex._native, 'the device branch did not run'
    return got, stub, ex


def _check_against_expectation(tag, m, got, g, shards, slots, total):
    want, M = X.expected_and_M(g, shards)
    ok, ratio, nbad = X.hold_bar(got, want, M)
    zeros = int((M == 0).sum())
    print(f'dp exchange {tag:44s} max |d|/M {ratio:.3e} (bar {X.BAR_L:.3e})  outside {nbad} of {total}  elements with M == 0: {zeros}')
    assert ok, f'{tag}: {nbad} elements outside 2^-18 M, worst ratio {ratio:.3e}'
    assert total - zeros > total // 4, 'most of the buffer is exactly zero: the case checks little'
    # every p.grad is the matching view of that buffer
    for n, p in m.base.named_parameters():
        off, cnt = slots[n]
        assert p.grad is not None and p.grad.data_ptr() == got.data_ptr() + 4 * off and p.grad.numel() == cnt, n
        assert torch.equal(p.grad.reshape(-1), got[off:off + cnt]), n
    return ratio


def _check_collectives(stub, ex, slots, total, overlap, nbuckets):
    X.assert_buckets_tile(stub.calls, total, nbuckets)
    assert [c[:2] for c in stub.calls] == ex.buckets_last_step
    assert [c[0] for c in stub.calls] == X.stage_cuts(slots), 'the buckets are not the backward\'s stages'
    if overlap:
        assert not any(c[2] for c in stub.calls), f'overlap=True, but a collective was issued on the default stream: {stub.calls}'
    else:
        assert all(c[2] for c in stub.calls), f'overlap=False, but a collective was issued off the default stream: {stub.calls}'
    assert ex._pending == [] and ex._flat is None


@pytest.mark.parametrize('rank', [0, 1])
@pytest.mark.parametrize('name', list(CASES))
def test_exchange_is_the_weighted_mean_of_the_local_gradients(name, rank, monkeypatch):
    from squeezedet_pytorch_amd import ops
    c = CASES[name]
    shards, overlap = c['shards'], c.get('overlap', True)
    m, batches, g, slots, total = _case(name)
    if c.get('C', 3) == 20:
        assert ops.convdet_padded(9, 20) and m.base.convdet_exec() is not m.base.convdet
    try:
        got, stub, ex = _exchanged(m, batches[rank], shards, rank, g, monkeypatch, overlap)
        _check_against_expectation(f'{name} rank {rank}', m, got, g, shards, slots, total)
        _check_collectives(stub, ex, slots, total, overlap, nbuckets=4)
        slot = torch.as_strided(got, (1,), (1,), total)
        assert float(slot) == float(sum(shards)), 'the count slot does not hold the global image count'
    finally:
        m.base.grad_sync = None


def test_a_forgotten_scale_slice_on_the_device_fails_the_bar(monkeypatch):
    """Teeth, on the device path itself: with ``scale_slice`` stubbed out exactly the stem's 1792 elements (less the exactly-zero ones)
    leave the bar -- the fault the criteria of tests/test_data_parallel_gpu.py let through at rel2 8.6e-3."""
    from squeezedet_pytorch_amd.exchange import GradientExchange
    shards = CASES['squeezedet_3_2']['shards']
    m, batches, g, slots, total = _case('squeezedet_3_2')
    monkeypatch.setattr(GradientExchange, 'scale_slice', lambda self, lo, hi: None)
    try:
        got, _stub, _ex = _exchanged(m, batches[0], shards, 0, g, monkeypatch)
        want, M = X.expected_and_M(g, shards)
        ok, ratio, nbad = X.hold_bar(got, want, M)
        stem = slots['features.0.weight'][1] + slots['features.0.bias'][1]
        err = (got.double() - want).abs()
        outside = (~(err <= X.BAR_L * M)).nonzero().flatten()
        print(f'dp exchange scale_slice stubbed out: max |d|/M {ratio:.3e}  outside {nbad} (the stem holds {stem} elements)')
        assert not ok and ratio > 0.1
        assert stem == 1792 and int(outside.max()) < stem, 'an element outside the stem left the bar'
        assert 0 < nbad <= int((g[0][:stem] != 0).sum())    # (an element this rank contributes 0 to cannot show the fault)
    finally:
        m.base.grad_sync = None


def test_two_backwards_in_a_row_on_one_attached_model(monkeypatch):
    """Second step: another batch, other shard sizes.  It holds the bar against its OWN expectation, so nothing of the first step's
    buffer, pending list or count slot survives."""
    shards_a, shards_b = (3, 2), (1, 3)
    cfg, m = _model()
    batches_a = _batches(cfg, 3, shards_a)
    batches_b = _batches(cfg, 3, shards_b, seed_img=13, seed_gt=12)
    g_a, g_b = _local_gradients(m, batches_a), _local_gradients(m, batches_b)
    slots, total = X.make_slots([(n, p.shape) for n, p in m.base.named_parameters()])
    try:
        got_a, stub, ex = _exchanged(m, batches_a[0], shards_a, 0, g_a, monkeypatch)
        first = got_a.clone()
        _check_against_expectation('two steps: first (3, 2) rank 0', m, got_a, g_a, shards_a, slots, total)
        _check_collectives(stub, ex, slots, total, True, 4)
        stub.prepare([g_b[1]], [shards_b[1]])
        got_b = _backward(m, batches_b[0])                  # (zero_grad inside)
        assert got_b.data_ptr() != got_a.data_ptr()
        _check_against_expectation('two steps: second (1, 3) rank 0', m, got_b, g_b, shards_b, slots, total)
        _check_collectives(stub, ex, slots, total, True, 4)
        assert float(torch.as_strided(got_b, (1,), (1,), total)) == 4.0
        assert torch.equal(got_a, first), 'the second backward wrote into the first step\'s buffer'
    finally:
        m.base.grad_sync = None


def test_fused_clip_sgd_behind_the_exchange(monkeypatch):
    """One ``FusedClipSGD`` step on the exchanged flat buffer: parameters and momentum against ``fp64_ref.clip_sgd`` applied to the
    MEASURED exchanged gradient at the bars of tests/test_fp64_optim_gpu.py, and the norm it clips by is the global one: within
    2^-18 (||got|| + ||M||) of ||expected|| (the norm kernel's bar plus ||got - expected|| <= 2^-18 ||M||)."""
    import test_fp64_optim_gpu as O
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    shards = (3, 2)
    cfg, m = _model()
    batches = _batches(cfg, 3, shards)
    g = _local_gradients(m, batches)
    slots, total = X.make_slots([(n, p.shape) for n, p in m.base.named_parameters()])
    want, M = X.expected_and_M(g, shards)
    global_norm = float(want.norm())
    m.zero_grad()
    opt = FusedClipSGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=0.5 * global_norm,
                       flat_grad=lambda: m.base.last_grad_flat)
    try:
        got, stub, ex = _exchanged(m, batches[0], shards, 0, g, monkeypatch, optimizer=opt)
        _check_against_expectation('clip + SGD: the exchanged gradient', m, got, g, shards, slots, total)
        assert opt._flat_base([p.grad for p in opt.params]) is not None, 'the gradients are not views of the flat buffer'
        p0, g0, b0 = O._snap(opt)
        norm = opt.step()
        torch.cuda.synchronize()
        tn64 = O._check_step(opt, p0, g0, b0, norm, 'behind the exchange, shards (3, 2) rank 0')
        local_norm = float(g[0].double().norm())
        print(f'dp exchange clip + SGD: norm {float(norm):.6e}  global {global_norm:.6e}  this rank\'s local {local_norm:.6e}')
        assert abs(float(norm) - global_norm) <= X.BAR_L * (tn64 + float(M.norm()))
        assert float(norm) > opt.max_norm                   # the clip was on
    finally:
        m.base.grad_sync = None


# ---- kernel level ----------------------------------------------------------------------------------------------------------------------

def _rand(*shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32))


def _guarded(n):
    """-> (view of n floats at the odd float offset GUARD inside a NaN buffer, the buffer)."""
    buf = torch.full((n + 2 * GUARD,), float('nan'), device='cuda')
    return buf[GUARD:GUARD + n], buf


def _guards_nan(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


@functools.lru_cache(maxsize=None)
def _wgrad_table():
    """The four-layer table of test_kernels_gpu.py::test_wgrad_batched_reduce_is_bitwise_the_per_layer_reduce with its slabs written,
    and the single-launch reduction at scale 1 -> (WgradBatch, row starts [5], reference flat buffer)."""
    from squeezedet_pytorch_amd import ops
    B, H, W = 2, 9, 21
    layers = [('a', 32, 16, 9), ('b', 16, 64, 1), ('c', 72, 24, 9), ('d', 48, 48, 1)]       # (key, N, C, taps)
    off, entries, starts = 0, [], []
    for key, N, C, taps in layers:
        starts.append(off)
        entries.append((key, N, C, taps, B, H, W, off, off + N * C * taps))
        off += N * C * taps + N
    starts.append(off)
    wb = ops.WgradBatch(entries, torch.device('cuda'))
    for i, (key, N, C, taps) in enumerate(layers):
        dy = _rand(B, H, W, N + 8, seed=40 + i).cuda()
        x = _rand(B, H, W, C + 4, seed=50 + i).cuda()
        assert ops.conv_wgrad(dy, 4, N, x, 4, C, taps, slab=wb.slab(key)) is None
    ref = torch.full((off,), float('nan'), device='cuda')
    wb.reduce(ref)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ref).all()) and any(wb.splits[k] > 1 for k in wb.splits), wb.splits
    return wb, starts, ref


@pytest.mark.parametrize('scale', [1.0, 3.0, 5.0])
@pytest.mark.parametrize('row_hi', [1, 2, 3])
def test_wgrad_batch_staged_reduce(row_hi, scale):
    """``reduce(0, row_hi)`` then ``reduce(row_hi, 4)`` (``sqd_wgrad_reduce_batched_range``): the first call leaves the other rows
    alone, both stay inside the buffer, and together they are the single launch times ``scale`` -- one rounding of an exact product
    (``t *= scale`` in the kernel's epilogue), so bit for bit ``fl32(sum * scale)``; at scale 1 bitwise the single launch."""
    wb, starts, ref = _wgrad_table()
    n = ref.numel()
    flat, buf = _guarded(n)
    wb.reduce(flat, 0, row_hi, scale=scale)
    torch.cuda.synchronize()
    cut = starts[row_hi]
    assert bool(torch.isnan(flat[cut:]).all()), 'the first range wrote into the rows of the second'
    assert not bool(torch.isnan(flat[:cut]).any()) and _guards_nan(buf, n)
    wb.reduce(flat, row_hi, 4, scale=scale)
    torch.cuda.synchronize()
    assert _guards_nan(buf, n)
    want = ref * scale                                       # float32 multiply: fl32(sum * scale)
    assert torch.equal(flat.view(torch.int32), want.view(torch.int32)), \
        f'{int((flat != want).sum())} elements differ from fl32(sum * {scale})'


def test_wgrad_reduce_rows_with_a_scale():
    """The padded ConvDet's own reduction (N 54 of 64, C 768, 9 taps, S 3) at scale 3: exactly ``fl32(3 * the scale-1 result)``."""
    from squeezedet_pytorch_amd import ops
    S, N, Npad, C, taps = 3, 54, 64, 768, 9
    stride = Npad * taps * C + Npad
    slab = torch.randn(S * stride, generator=torch.Generator().manual_seed(5)).cuda()
    out = {}
    for scale in (1.0, 3.0):
        dw, bw = _guarded(N * C * taps)
        db, bb = _guarded(N)
        ops.wgrad_reduce_rows(slab, S, N, Npad, C, taps, dw.view(N, C, 3, 3), db, scale=scale)
        torch.cuda.synchronize()
        assert _guards_nan(bw, N * C * taps) and _guards_nan(bb, N)
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        out[scale] = (dw, db)
    for one, three in zip(out[1.0], out[3.0]):
        assert torch.equal(three.view(torch.int32), (one * 3.0).view(torch.int32))
    assert float(out[1.0][0].abs().max()) > 0


LOOP_AT = 2048 * 1024                    # sqd_grad_scale: one block of 256 threads per 1024 elements, at most 2048 blocks -- past this size the
                                         # grid no longer grows and the grid-stride loop takes a fifth trip


def _grad_scale(g, n, mul, div_by, fill, fill_value):
    from squeezedet_pytorch_amd import _native as nat
    return nat.lib().sqd_grad_scale(nat.c_p(g) if g else None, n, mul, nat.c_p(div_by) if div_by else None,
                                    nat.c_p(fill) if fill else None, fill_value, nat.stream_handle(torch.device('cuda')))


@pytest.mark.parametrize('n', [1, 255, 1024, LOOP_AT - 1, LOOP_AT + 5])
def test_grad_scale_kernel(n):
    """``sqd_grad_scale`` as the exchange calls it -- fill only (n = 0: the count slot), multiply only (``scale_slice``), divide by the
    device scalar in the slot (``finish``) -- and both at once, on a view at an odd float offset: exactly ``fl32(fl32(g * mul) / d)``
    computed on the host, nothing outside the view touched, the slot written by the fill alone."""
    from squeezedet_pytorch_amd import _native as nat
    g0 = _rand(n, seed=n % 1000)
    buf = torch.full((n + 1 + 2 * GUARD,), float('nan'), device='cuda')      # [guard][n values][count slot][guard]
    g = buf[GUARD:GUARD + n]
    g.copy_(g0)
    assert (g.data_ptr() // 4) % 2 == 1
    slot = g.data_ptr() + 4 * n

    def outside_intact(slot_value):
        got_slot = float(buf[GUARD + n])
        return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n + 1:]).all()) and \
            (got_slot != got_slot if slot_value is None else got_slot == slot_value)
    # fill only
    assert _grad_scale(0, 0, 1.0, 0, slot, 5.0) == 0
    torch.cuda.synchronize()
    assert outside_intact(5.0) and torch.equal(g.cpu(), g0)
    # multiply only
    assert _grad_scale(g.data_ptr(), n, 3.0, 0, 0, 0.0) == 0
    torch.cuda.synchronize()
    want = g0 * 3.0
    assert outside_intact(5.0) and torch.equal(g.cpu().view(torch.int32), want.view(torch.int32))
    # divide by the device scalar
    assert _grad_scale(g.data_ptr(), n, 1.0, slot, 0, 0.0) == 0
    torch.cuda.synchronize()
    want = want / torch.tensor(5.0)
    assert outside_intact(5.0) and torch.equal(g.cpu().view(torch.int32), want.view(torch.int32))
    # multiply, divide and fill in one launch (the slot is outside the scaled range; another scalar divides)
    d = torch.tensor([3.0], device='cuda')
    g.copy_(g0)
    assert _grad_scale(g.data_ptr(), n, 2.5, d.data_ptr(), slot, 9.0) == 0
    torch.cuda.synchronize()
    want = (g0 * 2.5) / torch.tensor(3.0)
    assert outside_intact(9.0) and torch.equal(g.cpu().view(torch.int32), want.view(torch.int32))
    # a fill slot inside the scaled range: the argument error, before any launch
    before = buf.clone()
    for k in sorted({0, n // 2, n - 1}):
        assert _grad_scale(g.data_ptr(), n, 2.0, 0, g.data_ptr() + 4 * k, 1.0) == nat.ERR_BAD_ARG
    assert _grad_scale(0, 0, 1.0, 0, 0, 1.0) == nat.ERR_BAD_ARG                 # nothing to do at all
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), 'a refused call wrote'
