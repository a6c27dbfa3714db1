"""CPU tier: ``plans.PlanCache`` -- when a packed-weight copy counts as stale and how it is brought up to date -- with CPU parameter
holders and recording stand-ins for the plan constructors and the three batched refreshers (no kernel runs)."""
import copy

import pytest
import torch
import torch.nn as nn

from squeezedet_pytorch_amd import plans
from squeezedet_pytorch_amd.plans import PlanCache, version

IN_PLACE = ('wino', 'bridge', 'conv')             # in the order ``refresh`` launches them
REBUILD = ('fused_expand', 'fire_wino')
NMODS = {'conv': 1, 'wino': 1, 'fused_expand': 2, 'fire_wino': 2, 'bridge': 3}


class _Holder(nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.weight = nn.Parameter(torch.randn(4, 4, 1, 1, generator=g))
        self.bias = nn.Parameter(torch.randn(4, generator=g))


class _Plan:
    """Stand-in for a plan: forward conv / wino plans read the bias through the plan, data-gradient ones have none."""

    def __init__(self, mods, direction):
        self.bias = mods[0].bias.detach() if direction == 'fwd' else None


class _Model(nn.Module):
    def __init__(self, n=6):
        super().__init__()
        self.mods = nn.ModuleList(_Holder(i) for i in range(n))
        self.plan_cache = PlanCache()
        self.built = []                            # (kind, key, direction) of every build() call

    def get(self, kind, key, idx, direction='fwd'):
        mods = tuple(self.mods[i] for i in idx)
        assert len(mods) == NMODS[kind]

        def build():
            self.built.append((kind, key, direction))
            return _Plan(mods, direction)
        return self.plan_cache.get(kind, key, mods, build, direction)

    def entry(self, kind, key, direction='fwd'):
        hit = [e for e in self.plan_cache.entries() if (e.kind, e.key, e.direction) == (kind, key, direction)]
        assert len(hit) == 1
        return hit[0]

    def stale(self):
        return {(e.kind, e.key, e.direction) for e in self.plan_cache.entries() if e.version != version(e.mods)}


# what the tests below cache: (kind, key, indices of the modules, direction)
LAYOUT = [
    ('conv', '0.squeeze', (0,), 'fwd'), ('conv', '0.squeeze', (0,), 'dgrad'), ('conv', '1.expand1x1', (1,), 'fwd'),
    ('conv', '2.expand1x1', (2,), 'dgrad'), ('conv', '3.squeeze', (3,), 'fwd'), ('conv', '3.squeeze@pool', (3,), 'fwd'),
    ('wino', '1.expand3x3', (1,), 'fwd'), ('wino', '1.expand3x3', (1,), 'dgrad'), ('wino', '4.expand3x3', (4,), 'fwd'),
    ('wino', 'convdet', (5,), 'dgrad'),
    ('bridge', (0, 12, False), (0, 1, 2), 'fwd'), ('bridge', (2, 12, True), (2, 3, 4), 'fwd'), ('bridge', (4, 10, False), (4, 5, 0), 'fwd'),
    ('fused_expand', (0, 7), (0, 1), 'fwd'), ('fused_expand', (1, 7), (1, 2), 'fwd'), ('fused_expand', (3, 7), (3, 4), 'fwd'),
    ('fused_expand', (4, 7), (4, 5), 'fwd'),
    ('fire_wino', (1, 10), (1, 2), 'fwd'), ('fire_wino', (3, 10), (3, 4), 'fwd'), ('fire_wino', (5, 10), (5, 0), 'fwd'),
]


def _filled():
    m = _Model()
    for kind, key, idx, direction in LAYOUT:
        m.get(kind, key, idx, direction)
    assert len(m.built) == len(LAYOUT) and not m.stale()
    return m


def _holding(i):
    return {(kind, key, direction) for kind, key, idx, direction in LAYOUT if i in idx}


@pytest.fixture
def calls(monkeypatch):
    """The three refreshers replaced by recorders: [(kind, [plans], [dgrad flags] | [parameter tensors per item])]."""
    log = []

    def packer(kind):
        def fake(plans_and_weights, is_dgrad):
            log.append((kind, [p for p, _w in plans_and_weights], list(is_dgrad), [w for _p, w in plans_and_weights]))
            return f'{kind} table {len(log)}'
        return fake

    def bridges(items):
        log.append(('bridge', [it[0] for it in items], None, [it[1:] for it in items]))
        return f'bridge tables {len(log)}'
    monkeypatch.setattr(plans, 'repack_batched', packer('conv'))
    monkeypatch.setattr(plans, 'repack_wino_batched', packer('wino'))
    monkeypatch.setattr(plans, 'refresh_bridge_plans', bridges)
    return log


def test_staleness_rule():
    m = _filled()
    with torch.no_grad():
        m.mods[1].weight.mul_(1.5)                           # in-place op on a weight: exactly the entries that hold module 1
        assert m.stale() == _holding(1)
        m.mods[4].bias.mul_(1.5)                             # ... and on a bias
        assert m.stale() == _holding(1) | _holding(4)
    m = _filled()
    m.mods[2].weight.data.mul_(2.0)                          # through .data: neither the counter nor the pointer moves
    m.mods[2].bias.data.mul_(2.0)
    assert m.stale() == set()
    m.mods[2].weight.data = m.mods[2].weight.data.clone()    # a new storage is seen
    assert m.stale() == _holding(2)
    m.mods[5].bias.data = m.mods[5].bias.data.clone()
    assert m.stale() == _holding(2) | _holding(5)
    m.plan_cache.clear()
    assert list(m.plan_cache.entries()) == [] and m.stale() == set()
    m.get('conv', '0.squeeze', (0,))                          # (and everything is built again afterwards)
    assert m.built[-1] == ('conv', '0.squeeze', 'fwd') and len(m.built) == len(LAYOUT) + 1


def test_refresh_groups_the_stale_entries_by_kind(calls):
    m = _filled()
    plans_before = {(e.kind, e.key, e.direction): e.plan for e in m.plan_cache.entries()}
    m.plan_cache.refresh()
    assert calls == []                                       # nothing stale: nothing at all
    with torch.no_grad():
        m.mods[0].weight.mul_(1.01)
        m.mods[1].bias.mul_(1.01)
    stale = _holding(0) | _holding(1)
    assert m.stale() == stale
    for kind in IN_PLACE + REBUILD:                          # several stale and several fresh entries of every kind
        n = sum(1 for k in stale if k[0] == kind)
        assert 2 <= n < sum(1 for e in LAYOUT if e[0] == kind), kind
    m.plan_cache.refresh()
    assert [c[0] for c in calls] == list(IN_PLACE)           # each refresher once, in this order
    for kind, got_plans, flags, params in calls:
        want = [k for k in plans_before if k in stale and k[0] == kind]
        assert [id(p) for p in got_plans] == [id(plans_before[k]) for k in want], kind
        if kind == 'bridge':
            for k, item in zip(want, params):
                mods = m.entry(*k).mods
                assert [t.data_ptr() for t in item] == [t.data_ptr() for mod in mods for t in (mod.weight, mod.bias)]
                assert not any(t.requires_grad for t in item)
        else:
            assert flags == [k[2] != 'fwd' for k in want], kind
            assert [w.data_ptr() for w in params] == [m.entry(*k).mods[0].weight.data_ptr() for k in want]
    assert m.stale() == {k for k in stale if k[0] in REBUILD}     # the rebuild kinds are not touched
    assert len(m.built) == len(LAYOUT)
    assert m.plan_cache._tables == {'wino': 'wino table 1', 'bridge': 'bridge tables 2', 'conv': 'conv table 3'}
    m.plan_cache.refresh()
    assert len(calls) == 3                                   # a second refresh calls nothing


def test_plan_identity_in_place_kinds_keep_their_plan_rebuild_kinds_get_a_new_one(calls):
    m = _filled()
    before = {(e.kind, e.key, e.direction): e.plan for e in m.plan_cache.entries()}
    with torch.no_grad():
        for mod in m.mods:
            mod.weight.mul_(1.01)
    m.plan_cache.refresh()
    for kind, key, idx, direction in LAYOUT:
        p = m.get(kind, key, idx, direction)
        assert (p is before[kind, key, direction]) == (kind in IN_PLACE), (kind, key)
        assert m.get(kind, key, idx, direction) is p
    assert m.built[len(LAYOUT):] == [(k, key, d) for k, key, _i, d in LAYOUT if k in REBUILD]      # each built exactly once
    assert len(calls) == 3 and not m.stale()
    # a stale entry met by get(): refreshed in place through its kind's refresher, with that one entry
    after = {(e.kind, e.key, e.direction): e.plan for e in m.plan_cache.entries()}
    nbuilt, batched = len(m.built), dict(m.plan_cache._tables)
    with torch.no_grad():
        for mod in m.mods:
            mod.bias.mul_(1.01)
    for kind, key, idx, direction in LAYOUT:
        n = len(calls)
        p = m.get(kind, key, idx, direction)
        if kind in IN_PLACE:
            assert p is after[kind, key, direction] and len(calls) == n + 1
            assert calls[-1][0] == kind and [id(q) for q in calls[-1][1]] == [id(p)]
            assert calls[-1][2] == (None if kind == 'bridge' else [direction != 'fwd'])
        else:
            assert p is not after[kind, key, direction] and len(calls) == n
        assert m.get(kind, key, idx, direction) is p and len(calls) == n + (kind in IN_PLACE)
    assert len(m.built) == nbuilt + sum(1 for e in LAYOUT if e[0] in REBUILD) and not m.stale()
    # the one-entry launches keep their tables apart: the tables of the batched launches (which a captured step replays) stay alive
    assert all(m.plan_cache._tables[kind] is batched[kind] for kind in IN_PLACE) and len(m.plan_cache._tables) == 2 * len(IN_PLACE)


def test_bias_is_repointed_for_forward_entries_only(calls):
    m = _filled()
    for mod in m.mods:
        mod.bias.data = mod.bias.data.clone()                # (what .to() or load_state_dict(assign=True) does)
    m.plan_cache.refresh()
    seen = 0
    for e in m.plan_cache.entries():
        if e.kind in ('conv', 'wino'):
            if e.direction == 'fwd':
                assert e.plan.bias.data_ptr() == e.mods[0].bias.data_ptr() and not e.plan.bias.requires_grad
                seen += 1
            else:
                assert e.plan.bias is None
    assert seen == 6
    m.mods[3].bias.data = m.mods[3].bias.data.clone()        # ... and by the refresh a stale get() does
    p = m.get('conv', '3.squeeze', (3,))
    assert p.bias.data_ptr() == m.mods[3].bias.data_ptr()
    m.mods[0].weight.data = m.mods[0].weight.data.clone()
    assert m.get('conv', '0.squeeze', (0,), 'dgrad').bias is None


def test_one_module_under_two_keys_is_refreshed_from_the_stored_module(calls):
    """'3.squeeze' and '3.squeeze@pool' hold the same module: both are refreshed from it.  The holders sit in a list whose indices
    do not match the names, so reading the key as a path would pick another module (or none)."""
    cache = PlanCache()
    mods = [_Holder(10 + i) for i in range(3)]
    sq = mods[0]                                             # ('3.squeeze' parsed as a path would ask for index 3)
    pa = cache.get('conv', ('3.squeeze', 5), (sq,), lambda: _Plan((sq,), 'fwd'))
    pb = cache.get('conv', ('3.squeeze@pool', 5), (sq,), lambda: _Plan((sq,), 'fwd'))
    pc = cache.get('conv', (object(), 5), (mods[1],), lambda: _Plan((mods[1],), 'fwd'))      # any hashable is a key
    assert pa is not pb
    with torch.no_grad():
        sq.weight.mul_(2.0)
    cache.refresh()
    assert len(calls) == 1 and calls[0][0] == 'conv'
    assert [id(p) for p in calls[0][1]] == [id(pa), id(pb)] and pc not in calls[0][1]
    assert [w.data_ptr() for w in calls[0][3]] == [sq.weight.data_ptr()] * 2
    assert all(e.version == version(e.mods) for e in cache.entries())


def test_deepcopy_entries_reference_the_copied_modules(calls):
    m = _filled()
    c = copy.deepcopy(m)
    old = {id(mod) for mod in m.mods}
    new = {id(mod): i for i, mod in enumerate(c.mods)}
    assert len(list(c.plan_cache.entries())) == len(LAYOUT)
    for e, (kind, key, idx, direction) in zip(c.plan_cache.entries(), LAYOUT):
        assert (e.kind, e.key, e.direction) == (kind, key, direction)
        assert tuple(new[id(mod)] for mod in e.mods) == idx and not any(id(mod) in old for mod in e.mods)
        assert e.plan is not m.entry(kind, key, direction).plan
    # the copies were packed from the ORIGINAL parameters' storage: every entry of the copy is stale, none of the original
    assert c.stale() == {(k, key, d) for k, key, _i, d in LAYOUT} and not m.stale()
    c.plan_cache.refresh()
    assert [x[0] for x in calls] == list(IN_PLACE)
    for _kind, _plans, _flags, params in calls[:1] + calls[2:]:
        assert {w.data_ptr() for w in params} <= {mod.weight.data_ptr() for mod in c.mods}


def test_model_keeps_read_only_views_in_the_former_dictionary_shapes():
    """``SqueezeDetBase._plans`` / ``_wino_plans`` / ``_fused_plans`` read the cache in the shapes of the dictionaries it replaced:
    (name, cfg, direction) -> (version, plan); ('fused' | 'firewino', idx, cfg) -> (version, plan); ('firebridge', idx, cfg, pooled)
    -> (version, plan, mods)."""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd.model import SqueezeDetBase
    base = SqueezeDetBase(sqd.make_cfg(device='cpu'))
    i, f, nxt = next((i, f, n) for i, (f, n) in enumerate(zip(base.features, base.features[1:]))
                     if hasattr(f, 'expand3x3') and hasattr(n, 'squeeze'))
    pair, three = (f.expand1x1, f.expand3x3), (f.expand1x1, f.expand3x3, nxt.squeeze)

    def get(kind, key, mods, direction='fwd'):
        return base.plan_cache.get(kind, key, mods, lambda: _Plan(mods, direction), direction)
    sq_f, sq_d = get('conv', (f'{i}.squeeze', 5), (f.squeeze,)), get('conv', (f'{i}.squeeze', 5), (f.squeeze,), 'dgrad')
    det = get('conv', ('convdet', 3), (base.convdet,))
    wino = get('wino', (f'{i}.expand3x3', 2), (f.expand3x3,), 'dgrad')
    fused, fwino, bridge = get('fused_expand', (i, 7), pair), get('fire_wino', (i, 10), pair), get('bridge', (i, 12, True), three)
    assert base._plans == {(f'{i}.squeeze', 5, 'fwd'): (version((f.squeeze,)), sq_f), (f'{i}.squeeze', 5, 'dgrad'): (version((f.squeeze,)), sq_d),
                           ('convdet', 3, 'fwd'): (version((base.convdet,)), det)}
    assert base._wino_plans == {(f'{i}.expand3x3', 2, 'dgrad'): (version((f.expand3x3,)), wino)}
    assert base._fused_plans == {('fused', i, 7): (version(pair), fused), ('firewino', i, 10): (version(pair), fwino),
                                 ('firebridge', i, 12, True): (version(three), bridge, three)}
    base.invalidate_plans()
    assert base._plans == {} and base._wino_plans == {} and base._fused_plans == {}
