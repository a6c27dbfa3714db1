"""``trainer`` stays the one import point of the training path: every name it exposed before its split into ``exchange``, ``optim`` and
``graph_step`` is still there and IS the object of its home module, and the rank-stream state is one dict, whichever module it is
reached through."""
import types

import pytest
import torch

from squeezedet_pytorch_amd import exchange, graph_step, optim
from squeezedet_pytorch_amd import trainer as tr

HOMES = {
    exchange: ['_dist', 'shard_sizes', 'GradientExchange', 'broadcast_parameters', 'find_base', '_RANK_STREAMS', 'mark_rank_streams_set',
               'attach_data_parallel', 'detach_data_parallel', 'allreduce_gradients'],
    optim: ['HyperTable', 'FusedClipBase', 'FusedClipSGD', 'FusedClipAdamW'],
    graph_step: ['SPARSE_CAP_MIN', 'LOG_RING', 'LOG_ROWS', 'sparse_capacity', 'gt_form', 'step_signature', 'GraphedStep'],
    tr: ['encode_sparse_batch', 'LOSS_KEYS', 'Trainer', 'make_train_step'],
}


@pytest.mark.parametrize('home,name', [(h, n) for h, names in HOMES.items() for n in names], ids=lambda v: v if isinstance(v, str) else v.__name__)
def test_trainer_exports_the_home_modules_object(home, name):
    assert getattr(tr, name) is getattr(home, name)
    obj = getattr(home, name)
    if isinstance(obj, (type, types.FunctionType)):
        assert obj.__module__ == home.__name__, f'{name} is defined in {obj.__module__}, not in {home.__name__}'


def test_rank_stream_state_is_one_dict(monkeypatch):
    """``mark_rank_streams_set`` through ``trainer`` acts on the state ``attach_data_parallel`` reads: a rank whose streams are marked as
    set keeps its seed at the next attach, one whose mark was cleared gets the rank offset again."""
    assert exchange.attach_data_parallel.__globals__['_RANK_STREAMS'] is tr._RANK_STREAMS
    assert tr.mark_rank_streams_set.__globals__['_RANK_STREAMS'] is tr._RANK_STREAMS
    dist = types.SimpleNamespace(get_rank=lambda group=None: 3, get_world_size=lambda group=None: 4)     # a process group's rank 3
    base = types.SimpleNamespace(grad_sync=None)
    monkeypatch.setattr(exchange, '_dist', lambda group=None: dist)
    monkeypatch.setattr(exchange, 'find_base', lambda model: base)
    was, seed_was = dict(tr._RANK_STREAMS), torch.initial_seed()
    try:
        torch.manual_seed(5)
        tr.mark_rank_streams_set(True)
        assert exchange._RANK_STREAMS == {'set': True, 'seed': 5}
        assert tr.attach_data_parallel(None, broadcast=False) is base.grad_sync and torch.initial_seed() == 5
        tr.mark_rank_streams_set(False)
        assert exchange._RANK_STREAMS == {'set': False, 'seed': None}
        tr.attach_data_parallel(None, broadcast=False)
        assert torch.initial_seed() == 5 + 3 and exchange._RANK_STREAMS == {'set': True, 'seed': 8}
    finally:
        tr._RANK_STREAMS.update(was)
        torch.manual_seed(seed_was)
