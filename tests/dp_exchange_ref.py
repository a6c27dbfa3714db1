"""What the data-parallel gradient exchange (``exchange.GradientExchange``) must compute, and a stand-in for ``torch.distributed``.

For fixed shards the exchange is a linear map of the ranks' local gradients, so its expected value needs no model reference:

    expected = (sum_r b_r g_r) / sum_r b_r        (float64; g_r: rank r's gradient of its LOCAL mean, b_r: its image count)

An element goes through one multiply by a small integer, one add per peer and one division: 3 to 4 fp32 roundings of magnitude
``M = (sum_r b_r |g_r|) / sum_r b_r``.  The bar is ``fp64_ref.BAR_L`` (2^-18) times ``M`` on EVERY element, about 20x the rounding bound;
where ``M == 0`` the result must be exactly 0.

* ``expected_and_M`` / ``hold_bar``: the property.
* ``restated``: the exchange restated in float32 torch as ``backward.py`` drives it (scale by ``b_r`` where the gradient is produced, a
  count slot behind the gradients, buckets summed tail first, ONE division by the summed slot), with the faults of ``MUTANTS``.
* ``StubDist``: what ``exchange._dist()`` returns, for two or three "ranks" in one process -- no spawn, no sockets.
* ``old_criteria``: the figures the two-process test held the exchange to before (relative L2, ConvDet max-abs).

Imports nothing that needs a GPU."""
import torch

from fp64_ref import BAR_L

F32, F64 = torch.float32, torch.float64

MUTANTS = ('stem_unscaled', 'one_bias_unscaled', 'convdet_unscaled', 'one_stage_unscaled', 'divide_by_world', 'divide_by_local_count',
           'bucket_drops_first_element', 'count_slot_in_wrong_bucket')
OLD_REL2, OLD_CONVDET = 1e-2, 2e-4                   # tests/test_data_parallel_gpu.py against a single-process run


def expected_and_M(g_list, b_list):
    """-> (expected, M) float64 on the device of ``g_list``: the count-weighted mean of the ranks' flat gradients and its magnitude."""
    assert len(g_list) == len(b_list) and len(g_list) > 0
    tot = float(sum(int(b) for b in b_list))
    e = torch.zeros_like(g_list[0], dtype=F64)
    m = torch.zeros_like(e)
    for g, b in zip(g_list, b_list):
        assert g.dtype == F32 and g.shape == e.shape
        e += float(int(b)) * g.double()
        m += float(int(b)) * g.double().abs()
    return e / tot, m / tot


def hold_bar(got, expected, M):
    """-> (every element within BAR_L * M [exactly 0 where M == 0], the largest |d| / M over M > 0, the number of elements outside)."""
    assert got.dtype == F32 and got.shape == expected.shape == M.shape
    err = (got.double() - expected).abs()
    bad = ~(err <= BAR_L * M)                        # (NaN counts as outside)
    pos = M > 0
    ratio = float((err[pos] / M[pos]).max()) if bool(pos.any()) else 0.0
    if bool((err[~pos] != 0).any()):
        ratio = float('inf')
    return not bool(bad.any()), ratio, int(bad.sum())


def old_criteria(got, ref64, convdet_numel):
    """(relative L2 over the buffer, ConvDet max-abs over max|ref|) against a single-process gradient ``ref64``: what
    tests/test_data_parallel_gpu.py asserts (<= OLD_REL2, <= OLD_CONVDET)."""
    d = got.double() - ref64
    cd = ref64[-convdet_numel:]
    return float(d.norm() / ref64.norm()), float(d[-convdet_numel:].abs().max() / cd.abs().max())


def make_slots(named_shapes):
    """[(name, shape)] in ``named_parameters`` order -> {name: (offset, numel)} and the total."""
    slots, off = {}, 0
    for name, shape in named_shapes:
        n = 1
        for d in shape:
            n *= int(d)
        slots[name] = (off, n)
        off += n
    return slots, off


def stage_cuts(slots):
    """The bucket boundaries of the backward walk (descending, ending at 0): a stage ends in front of the first Fire module behind a
    pool, i.e. where the feature index jumps by more than one between two ``squeeze.weight`` entries, and the stem is the last
    bucket.  (squeezedet: features.9 / .6 / .3 / 0.)"""
    pre = next(iter(slots)).split('features.')[0]
    idx = sorted({int(n[len(pre):].split('.')[1]) for n in slots if n.startswith(pre + 'features.') and '.squeeze.' in n})
    firsts = [i for k, i in enumerate(idx) if k == 0 or i - idx[k - 1] > 1]
    return [slots[f'{pre}features.{i}.squeeze.weight'][0] for i in reversed(firsts)] + [0]


def _unscaled_names(slots, cuts, mutant):
    names = list(slots)
    if mutant == 'stem_unscaled':
        return [n for n in names if '.features.0.' in '.' + n]
    if mutant == 'one_bias_unscaled':
        biases = [n for n in names if n.endswith('.bias')]
        return [biases[len(biases) // 2]]
    if mutant == 'convdet_unscaled':
        return [n for n in names if '.convdet.' in '.' + n]
    if mutant == 'one_stage_unscaled':
        lo, hi = (cuts[1], cuts[0]) if len(cuts) > 1 else (0, slots[names[-1]][0])
        return [n for n in names if lo <= slots[n][0] < hi]
    return []


def restated(g_list, b_list, slots, mutant=None, cuts=(0,), rank=0):
    """The exchange as rank ``rank`` sees it, float32: every rank's tensors times ``b_r`` (where they are produced), the count slot
    appended, the buckets ``[cut, previous cut)`` summed tail first (own + the sum of the peers in rank order: ``StubDist``), one
    division by the summed slot.  ``mutant``: one of ``MUTANTS`` put into the otherwise correct sequence.  -> flat float32 [total]."""
    assert mutant is None or mutant in MUTANTS, mutant
    total = g_list[0].numel()
    cuts = list(cuts)
    assert cuts[-1] == 0 and all(a > b for a, b in zip(cuts, cuts[1:])) and cuts[0] < total
    skip = _unscaled_names(slots, cuts, mutant)
    bufs = []
    for g, b in zip(g_list, b_list):
        buf = torch.empty(total + 1, dtype=F32)
        buf[:total] = g * float(int(b))
        for n in skip:                               # the fault is in the code, so every rank has it
            off, cnt = slots[n]
            buf[off:off + cnt] = g[off:off + cnt]
        buf[total] = float(int(b))
        bufs.append(buf)
    own = bufs[rank]
    peers = [bufs[r] for r in range(len(bufs)) if r != rank]
    peer = peers[0].clone()
    for p in peers[1:]:
        peer += p
    late = None
    if mutant == 'bucket_drops_first_element':
        # the boundary that is off by one: the first (tail first) whose element receives something from the peers -- many gradient
        # elements are exactly 0 (dead ReLUs), and an element the peers add 0 to cannot show the fault
        late = next((k for k, c in enumerate(cuts) if float(peer[c]) != 0.0), None)
        assert late is not None, 'every bucket starts on an element the peers contribute 0 to'
    top = total
    for k, c in enumerate(cuts):
        lo, hi = c, (total + 1 if top == total else top)
        if k == late:
            lo += 1                                  # the collective starts one element late: that element keeps the local b * g
        if mutant == 'count_slot_in_wrong_bucket' and hi == total + 1:
            hi = total                               # the slot is never summed: it holds the local count when the division reads it
        own[lo:hi] += peer[lo:hi]
        top = c
    if mutant == 'divide_by_world':
        div = torch.tensor(float(len(bufs)), dtype=F32)
    elif mutant == 'divide_by_local_count':
        div = torch.tensor(float(int(b_list[rank])), dtype=F32)
    else:
        div = own[total].clone()
    return own[:total] / div


class _Work:
    def __init__(self, event):
        self._event = event

    def wait(self):
        if self._event is not None:                  # (as a process group's Work: the current stream waits for the collective)
            torch.cuda.current_stream().wait_event(self._event)
        return True


class StubDist:
    """Stands in for the ``torch.distributed`` module that ``exchange._dist()`` returns: this process is rank ``rank`` of ``world``,
    and ``all_reduce`` adds the matching slice of the peers' prepared buffer (``prepare``) to its argument on the current stream.
    ``calls``: every collective as (lo, hi, issued on the default stream)."""

    class ReduceOp:
        SUM = 'sum'

    def __init__(self, world, rank=0):
        self.world, self.rank = int(world), int(rank)
        self.calls = []
        self.peer = None

    def prepare(self, peer_g, peer_b, device=None):
        """``peer_g`` / ``peer_b``: the flat local gradients and image counts of the OTHER ranks, in rank order."""
        assert len(peer_g) == len(peer_b) == self.world - 1
        buf = None
        for g, b in zip(peer_g, peer_b):
            one = torch.cat([g.detach().to(F32) * float(int(b)), torch.full((1,), float(int(b)), dtype=F32, device=g.device)])
            buf = one if buf is None else buf + one
        self.peer = buf if device is None else buf.to(device)
        self.calls = []
        return self

    def get_world_size(self, group=None):
        return self.world

    def get_rank(self, group=None):
        return self.rank

    def broadcast(self, tensor, src=0, group=None, async_op=False):
        return None

    def all_reduce(self, t, op=None, group=None, async_op=False):
        assert op == self.ReduceOp.SUM and self.peer is not None
        n = self.peer.numel()
        assert t.dtype == F32 and t.is_contiguous() and t.device == self.peer.device
        assert t.untyped_storage().nbytes() == 4 * n, 'not a slice of the flat gradient buffer (total + 1 floats)'
        lo = t.storage_offset()
        hi = lo + t.numel()
        assert 0 <= lo < hi <= n
        on_default = True
        event = None
        if t.is_cuda:
            on_default = torch.cuda.current_stream(t.device) == torch.cuda.default_stream(t.device)
        t.add_(self.peer[lo:hi])
        if t.is_cuda:
            event = torch.cuda.Event()
            event.record()
        self.calls.append((lo, hi, on_default))
        return _Work(event) if async_op else None


def install(monkeypatch, stub):
    """``exchange._dist()`` -> ``stub`` until the test ends."""
    from squeezedet_pytorch_amd import exchange
    monkeypatch.setattr(exchange, '_dist', lambda group=None: stub)
    return stub


def assert_buckets_tile(calls, total, nbuckets=None):
    """The recorded collectives cover [0, total + 1) once each, tail first, the count slot in the first of them."""
    assert calls, 'no collective was issued'
    assert calls[0][1] == total + 1, f'the first bucket {calls[0][:2]} does not carry the count slot at {total}'
    for (lo, _hi, _s), (_lo2, hi2, _s2) in zip(calls, calls[1:]):
        assert hi2 == lo, f'buckets {[c[:2] for c in calls]} do not tile the buffer tail first'
    assert calls[-1][0] == 0, f'buckets {[c[:2] for c in calls]} stop short of the head of the buffer'
    assert all(lo < hi for lo, hi, _s in calls)
    if nbuckets is not None:
        assert len(calls) == nbuckets, [c[:2] for c in calls]
