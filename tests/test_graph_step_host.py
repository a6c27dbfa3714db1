"""CPU tier of the captured training step (trainer.GraphedStep): what decides whether a captured graph is still valid (the signature),
how large the fixed sparse-gt buffers are (the capacity), when the optimizer's device hyper-parameter table is written, and the status
codes of the three new entry points.  No GPU call is made."""
import ctypes

import pytest


def _sig(**kw):
    from squeezedet_pytorch_amd.trainer import step_signature
    args = dict(image_shape=(2, 64, 96), form='dense', cap=0, training=True, trainable=('a.weight', 'a.bias'), clip_on=True,
                loss_weights=(1.0, 3.75, 100.0, 6.0))
    args.update(kw)
    return step_signature(**args)


def test_signature_changes_with_what_a_captured_step_depends_on():
    base = _sig()
    assert base == _sig() and hash(base) == hash(_sig())
    assert _sig(trainable=['a.weight', 'a.bias']) == base            # (a list or a tuple of the same names)
    changed = {
        'B': _sig(image_shape=(3, 64, 96)),
        'H': _sig(image_shape=(2, 128, 96)),
        'W': _sig(image_shape=(2, 64, 192)),
        'form sparse': _sig(form='sparse', cap=64),
        'form masked': _sig(form='masked', cap=64),
        'capacity': _sig(form='sparse', cap=128),
        'eval mode': _sig(training=False),
        'frozen parameter': _sig(trainable=('a.weight',)),
        'clip off': _sig(clip_on=False),
        'loss weight': _sig(loss_weights=(1.0, 3.75, 100.0, 5.0)),
    }
    sigs = [base] + list(changed.values())
    assert len(set(sigs)) == len(sigs), 'two different steps share a signature'
    assert changed['form sparse'] != changed['form masked']


def test_gt_form_of_a_batch():
    from squeezedet_pytorch_amd.trainer import gt_form
    assert gt_form({'image': 0, 'gt': 1}) == 'dense'
    assert gt_form({'image': 0, 'gt_sparse': 1}) == 'sparse'
    assert gt_form({'image': 0, 'gt_sparse': 1, 'gt_ignore': None}) == 'sparse'
    assert gt_form({'image': 0, 'gt_sparse': 1, 'gt_ignore': 2}) == 'masked'
    with pytest.raises(ValueError, match='neither gt nor gt_sparse'):
        gt_form({'image': 0})


def test_sparse_capacity_rounding():
    from squeezedet_pytorch_amd.trainer import SPARSE_CAP_MIN, sparse_capacity
    assert SPARSE_CAP_MIN == 64
    for total, want in ((0, 64), (1, 64), (63, 64), (64, 64), (65, 128), (128, 128), (129, 256), (1000, 1024), (1024, 1024), (1025, 2048)):
        assert sparse_capacity(total) == want, total
    # never shrinks, doubles from where it is
    assert sparse_capacity(3, current=256) == 256
    assert sparse_capacity(257, current=256) == 512
    assert sparse_capacity(2000, current=128) == 2048
    for total in range(0, 5000, 37):
        cap = sparse_capacity(total)
        assert cap >= max(total, 64) and cap & (cap - 1) == 0 and (cap == 64 or cap // 2 < total)


def test_hyper_table_is_written_only_when_a_value_changed():
    """The rule behind FusedClipSGD.refresh_hyper, against a recording fake of the native call."""
    from squeezedet_pytorch_amd.trainer import HyperTable
    calls = []
    t = HyperTable(calls.append)
    v = (0.01, 0.9, 1e-4, 5.0)
    assert t.refresh(v) is True and calls == [v]
    for _ in range(3):
        assert t.refresh(v) is False
    assert calls == [v]
    assert t.refresh([0.01, 0.9, 1e-4, 5.0]) is False            # the same values in another container
    v2 = (0.005, 0.9, 1e-4, 5.0)                                  # an LR schedule
    assert t.refresh(v2) is True and calls == [v, v2]
    assert t.refresh(v2) is False
    for i, other in enumerate(((0.005, 0.8, 1e-4, 5.0), (0.005, 0.8, 0.0, 5.0), (0.005, 0.8, 0.0, 0.0))):      # every field counts
        assert t.refresh(other) is True and len(calls) == 3 + i
    assert t.refresh(calls[-1], force=True) is True and len(calls) == 6      # (a new table buffer)
    # under capture: nothing is written; a stale table is the caller's bug
    n = len(calls)
    assert t.refresh(calls[-1], capturing=True) is False and len(calls) == n
    with pytest.raises(RuntimeError, match='stale under stream capture'):
        t.refresh(v, capturing=True)
    assert len(calls) == n and t.written == calls[-1]


def test_new_entry_points_refuse_null_pointers_without_gpu():
    from squeezedet_pytorch_amd import _native as nat
    lib = nat.lib()
    null = ctypes.c_void_p(0)
    some = ctypes.c_void_p(4096)                  # never dereferenced: validation happens before any launch
    for name in ('sqd_sgd_clip_step_chunked_dev', 'sqd_fill_f32x4', 'sqd_train_log_push'):
        assert name in nat._SIGNATURES
    dev = lib.sqd_sgd_clip_step_chunked_dev
    assert dev(null, some, 1, some, some, some, some, null) == nat.ERR_BAD_ARG          # descs
    assert dev(some, null, 1, some, some, some, some, null) == nat.ERR_BAD_ARG          # chunks
    assert dev(some, some, 0, some, some, some, some, null) == nat.ERR_BAD_ARG          # no chunk
    assert dev(some, some, -3, some, some, some, some, null) == nat.ERR_BAD_ARG
    assert dev(some, some, 1, some, some, some, null, null) == nat.ERR_BAD_ARG          # hyper table
    assert lib.sqd_fill_f32x4(null, 1.0, 2.0, 3.0, 4.0, null) == nat.ERR_BAD_ARG
    push = lib.sqd_train_log_push
    assert push(null, 2, some, some, some, 64, null) == nat.ERR_BAD_ARG
    assert push(some, 2, null, some, some, 64, null) == nat.ERR_BAD_ARG
    assert push(some, 2, some, null, some, 64, null) == nat.ERR_BAD_ARG
    assert push(some, 2, some, some, null, 64, null) == nat.ERR_BAD_ARG
    assert push(some, 0, some, some, some, 64, null) == nat.ERR_BAD_ARG
    assert push(some, 2, some, some, some, 0, null) == nat.ERR_BAD_ARG


def test_cfg_field_and_refusals_that_need_no_gpu():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd.trainer import GraphedStep
    assert sqd.make_cfg(device='cpu').graph_step is False
    assert sqd.make_cfg(device='cpu', graph_step=True).graph_step is True
    import torch
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match='FusedClipSGD.*SGD'):
        GraphedStep(lin, torch.optim.SGD(lin.parameters(), lr=0.1))


def test_pack_table_cache_evicts_least_recently_used(monkeypatch):
    """plans._pack_tables (descriptor tables of the batched re-pack launches, cached by content): a hit returns the same tensors and
    counts as a use; beyond 16 entries the least recently used one goes, never one of the latest few -- the tables of a refresh that
    ran a moment ago (one per kind) are all still there when the same refresh is captured into a graph."""
    from squeezedet_pytorch_amd import plans
    monkeypatch.setattr(plans, '_PACK_TABLES', {})
    get = lambda i, what='conv': plans._pack_tables(what, 'cpu', [[i, i + 1, i + 2]])      # noqa: E731
    first = {i: get(i) for i in range(17)}
    assert len(plans._PACK_TABLES) == 17 and all(get(i)[0] is first[i][0] for i in range(17))
    assert first[3][0].tolist() == [[3, 4, 5]] and first[3][0].dtype.is_floating_point is False
    # 0 is used again, then 18 distinct keys arrive in total: 1 (the least recently used) goes, 0 stays
    assert get(0)[0] is first[0][0]
    get(17)
    assert len(plans._PACK_TABLES) == 17
    assert get(0)[0] is first[0][0], 'a recently used table was evicted'
    assert get(1)[0] is not first[1][0], 'the least recently used table was kept'
    # a full cache, then the three tables of one refresh (conv, wino, bridge): all three are hits right afterwards
    for i in range(100, 120):
        get(i)
    trio = [get(1000, what) for what in ('wino', 'bridge', 'conv')]
    assert len(plans._PACK_TABLES) <= 18
    for what, t in zip(('wino', 'bridge', 'conv'), trio):
        assert get(1000, what)[0] is t[0], f'{what}: the table of a refresh that just ran is a miss'
