"""CPU tier: the property the data-parallel gradient exchange is held to (tests/dp_exchange_ref.py) has teeth, and the criteria it
replaces did not.

Operands: the oracle's float64 gradients of the case tests/test_data_parallel_gpu.py runs (64x96, seeds 1234 / 3 / 2, five images), per
shard, rounded to float32 -- what a rank hands to the exchange.  For shards (3, 2) and (1, 4), seen from either rank:

* ``restated`` without a fault holds ``|got - expected| <= 2^-18 M`` on every element (the ratio is a few 2^-24);
* every mutant fails it;
* measured by the old criteria (relative L2 <= 1e-2 and ConvDet max-abs <= 2e-4 against the single-process gradient of all five images)
  a never-scaled stem, a never-scaled bias and a bucket that starts one element late all PASS: the figures are printed per mutant.

Then ``StubDist`` drives the CPU branch of ``GradientExchange`` itself through the three-cut sequence of tests/test_data_parallel_cpu.py:
bit for bit ``restated``, buckets that tile ``[0, total + 1)`` once each tail first, the count slot in the first."""
import functools

import pytest
import torch

import dp_exchange_ref as X

SIZE = (64, 96)
SHARDS = ((3, 2), (1, 4))
OLD_PASSES = ('stem_unscaled', 'one_bias_unscaled', 'bucket_drops_first_element')


@functools.lru_cache(maxsize=None)
def _operands():
    """-> (slots, total, {(lo, hi): flat float32 gradient of the local mean of images [lo, hi)}, float64 gradient of all five, ConvDet
    size).  One float64 oracle run per shard, shared by every test of the module."""
    import oracle
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    cfg = sqd.make_cfg(input_size=SIZE, device='cpu')
    sd = {k: v.double() for k, v in synthetic.make_state_dict('squeezedet', seed=1234).items()}
    x = synthetic.make_images(5, SIZE, seed=3).double()
    gt = synthetic.make_gt(5, cfg.anchors, SIZE, seed=2, min_boxes=2, max_boxes=3).double()
    slots, total = X.make_slots([(k, v.shape) for k, v in sd.items()])
    assert total == 2082120

    def grad(lo, hi):
        _, _, grads, _, _, _ = oracle.train_step_reference(sd, None, x[lo:hi], gt[lo:hi], cfg.anchors, SIZE)
        return torch.cat([grads[k].reshape(-1) for k in sd])
    ranges = {(0, 3), (3, 5), (0, 1), (1, 5)}
    local = {r: grad(*r).float() for r in ranges}
    ncd = slots['base.convdet.weight'][1] + slots['base.convdet.bias'][1]
    assert slots['base.convdet.bias'][0] + slots['base.convdet.bias'][1] == total
    return slots, total, local, grad(0, 5), ncd


def _shard_grads(shards):
    _, _, local, _, _ = _operands()
    lo, out = 0, []
    for b in shards:
        out.append(local[lo, lo + b])
        lo += b
    return out


def test_stage_cuts_are_the_backward_walks_buckets():
    slots, total, _, _, _ = _operands()
    cuts = X.stage_cuts(slots)
    assert cuts == [slots[f'base.features.{i}.squeeze.weight'][0] for i in (9, 6, 3)] + [0]


@pytest.mark.parametrize('shards', SHARDS)
@pytest.mark.parametrize('rank', [0, 1])
def test_restated_exchange_holds_the_bar_and_every_mutant_fails_it(shards, rank):
    slots, total, _, ref64, ncd = _operands()
    gs = _shard_grads(shards)
    want, M = X.expected_and_M(gs, shards)
    cuts = X.stage_cuts(slots)
    got = X.restated(gs, shards, slots, None, cuts, rank)
    ok, ratio, nbad = X.hold_bar(got, want, M)
    rel2, cd = X.old_criteria(got, ref64, ncd)
    print(f'dp exchange host shards {shards} rank {rank} {"none":28s} max |d|/M {ratio:.3e} (bar {X.BAR_L:.3e})  outside {nbad:8d}  '
          f'old: rel2 {rel2:.2e} convdet {cd:.2e}')
    assert ok and ratio <= 8 * 2.0 ** -24, ratio
    assert rel2 <= 1e-5 and cd <= 1e-5, 'the weighted mean of the shard gradients is not the gradient of the global mean'
    for mutant in X.MUTANTS:
        bad = X.restated(gs, shards, slots, mutant, cuts, rank)
        ok, ratio, nbad = X.hold_bar(bad, want, M)
        rel2, cd = X.old_criteria(bad, ref64, ncd)
        old_pass = rel2 <= X.OLD_REL2 and cd <= X.OLD_CONVDET
        print(f'dp exchange host shards {shards} rank {rank} {mutant:28s} max |d|/M {ratio:.3e} (bar {X.BAR_L:.3e})  outside {nbad:8d}  '
              f'old: rel2 {rel2:.2e} convdet {cd:.2e} -> {"PASSES" if old_pass else "caught"}')
        assert not ok and nbad >= 1, f'{mutant} holds the bar: the property has no teeth against it'
        assert ratio >= 1e3 * X.BAR_L, (mutant, ratio)           # not a near miss: orders of magnitude outside
        if mutant in OLD_PASSES:
            assert old_pass, f'{mutant}: rel2 {rel2:.2e}, convdet {cd:.2e}'


def test_restated_single_bucket_equals_staged_buckets_for_two_ranks():
    """a + b is order-free: with one peer the bucketing cannot change a bit."""
    slots, total, _, _, _ = _operands()
    gs = _shard_grads((3, 2))
    assert torch.equal(X.restated(gs, (3, 2), slots, None, X.stage_cuts(slots)), X.restated(gs, (3, 2), slots, None, (0,)))


def test_hold_bar_requires_exact_zero_where_the_magnitude_is_zero():
    g = [torch.tensor([0.0, 1.0]), torch.tensor([0.0, 3.0])]
    want, M = X.expected_and_M(g, (3, 2))
    assert want.tolist() == [0.0, 9.0 / 5.0] and M.tolist() == [0.0, 9.0 / 5.0]
    assert X.hold_bar(torch.tensor([0.0, 1.8]), want, M)[0]
    ok, ratio, nbad = X.hold_bar(torch.tensor([1e-30, 1.8]), want, M)
    assert not ok and nbad == 1 and ratio == float('inf')
    assert not X.hold_bar(torch.tensor([0.0, float('nan')]), want, M)[0]


@pytest.mark.parametrize('shards,rank', [((3, 2), 0), ((3, 2), 1), ((1, 4), 0), ((2, 1, 1), 1)])
def test_stub_drives_the_cpu_branch_of_the_exchange(shards, rank, monkeypatch):
    """begin -> (scale_slice, ready) per cut, tail first -> finish, as tests/test_data_parallel_cpu.py drives it over gloo."""
    from squeezedet_pytorch_amd import exchange
    slots, total, local, _, _ = _operands()
    if len(shards) == 3:
        gs = [local[0, 3], local[3, 5], local[0, 1]]               # (any three gradients serve: the map is linear)
    else:
        gs = _shard_grads(shards)
    cuts = [slots['base.features.9.squeeze.weight'][0], slots['base.features.6.squeeze.weight'][0], 0]
    stub = X.install(monkeypatch, X.StubDist(len(shards), rank))
    stub.prepare([g for r, g in enumerate(gs) if r != rank], [b for r, b in enumerate(shards) if r != rank])
    flat = torch.empty(total + 1)
    flat[:total] = gs[rank]
    ex = exchange.GradientExchange()
    assert ex.world() == len(shards)
    ex.begin(flat, total, shards[rank])
    top = total
    for c in cuts:
        ex.scale_slice(c, top)
        ex.ready(c, top)
        top = c
    ex.finish()
    X.assert_buckets_tile(stub.calls, total, nbuckets=3)
    assert [c[:2] for c in stub.calls] == ex.buckets_last_step and all(c[2] for c in stub.calls)
    want = X.restated(gs, shards, slots, None, cuts, rank)
    assert torch.equal(flat[:total], want)
    assert float(flat[total]) == float(sum(shards))
    e64, M = X.expected_and_M(gs, shards)
    ok, ratio, _ = X.hold_bar(flat[:total], e64, M)
    assert ok, ratio
    assert ex._pending == [] and ex._flat is None


def test_stub_refuses_a_tensor_that_is_not_a_slice_of_the_flat_buffer():
    stub = X.StubDist(2, 0).prepare([torch.zeros(8)], [2])
    with pytest.raises(AssertionError):
        stub.all_reduce(torch.zeros(4), op=stub.ReduceOp.SUM)
    flat = torch.ones(9)
    stub.all_reduce(flat[3:9], op=stub.ReduceOp.SUM)
    assert stub.calls == [(3, 9, True)] and flat.tolist() == [1.0] * 8 + [3.0]
