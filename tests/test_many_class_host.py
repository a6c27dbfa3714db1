"""CPU tier: the host side of the many-class head (``sqd_decode_many_fwd`` / ``sqd_resolve_many_fwd`` / ``sqd_detect_many_fwd`` /
``sqd_filter_many_fwd`` / ``sqd_loss_many_*``), of the padded ConvDet (``sqd_channel_pack_fwd`` / ``sqd_channel_unpack_fwd`` /
``sqd_wgrad_reduce_rows``) and the routing above them (``ops.head_path``, ``ops.convdet_width``, ``make_cfg``, the launch plans).
Every refusal is decided before any launch, so the status codes are exercised without a GPU: the pointers handed in are host
buffers that a refused call never touches."""
import ctypes
import os
import re

import pytest
import torch

import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import _native as nat, ops, plan
from test_detect_wide_host import _buf, _detect_args, _filter_args

A_MAX = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('sqd_decode_many_fwd', 'sqd_resolve_many_fwd', 'sqd_detect_many_fwd', 'sqd_filter_many_fwd', 'sqd_loss_many_fwd',
       'sqd_loss_many_mean_fwd', 'sqd_loss_many_bwd', 'sqd_loss_many_mean_bwd', 'sqd_channel_pack_fwd', 'sqd_channel_unpack_fwd',
       'sqd_wgrad_reduce_rows')
NULL = ctypes.c_void_p(0)


def test_new_symbols_exported_declared_and_documented():
    lib = nat.lib()
    header = open(os.path.join(ROOT, 'include', 'sqd_hip.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW:
        assert hasattr(lib, name) and name in nat._SIGNATURES, name
        assert re.search(r'\bint\s+%s\s*\(' % name, header), f'{name} not declared in include/sqd_hip.h'
        assert name in integration, f'{name} not in INTEGRATION.md'
    for name in ('decode_many', 'resolve_many', 'detect_many', 'filter_dense_many', 'loss_fwd_many', 'loss_mean_fwd_many', 'loss_bwd_many',
                 'loss_mean_bwd_many', 'head_path', 'convdet_width', 'convdet_padded', 'detect_fn', 'filter_fn', 'loss_fns'):
        assert callable(getattr(ops, name)), name


def test_detect_many_and_filter_many_status_codes():
    for f, args, ki, names in ((nat.lib().sqd_detect_many_fwd, _detect_args, 4, ('pred', 'anchors', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx')),
                               (nat.lib().sqd_filter_many_fwd, _filter_args, 3, ('ids', 'scores', 'boxes', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx'))):
        for n in names:
            assert f(*args(null=(n,))) == 1, f'null {n}'
        assert f(*args(C=0)) == 1
        assert f(*args(K=0)) == 1
        assert f(*args(A=0)) == 1 and f(*args(B=0)) == 1
        assert f(*args(C=257)) == 2
        assert f(*args(K=1025)) == 2
        assert f(*args(A=A_MAX + 1)) == 2
        assert f(*args(C=80, A=101, ws_words=103)) == 1                   # a short workspace: ceil4(101) = 104 words needed
        assert f(*args(C=256, ws_words=0)) == 1
        a = args(C=20)
        a[ki] = ctypes.c_void_p(a[ki].value + 4)                          # misaligned workspace
        assert f(*a) == 1


def test_decode_and_resolve_many_status_codes():
    lib = nat.lib()
    p = [_buf() for _ in range(7)]
    dec = lambda ptrs, B=1, A=10, C=20: lib.sqd_decode_many_fwd(*ptrs, B, A, C, 64, 96, NULL)
    res = lambda ptrs, B=1, A=10, C=20: lib.sqd_resolve_many_fwd(*ptrs, B, A, C, 64, 96, NULL)
    for i in range(5):
        assert dec([NULL if j == i else p[j] for j in range(5)]) == 1, i
    for i in (0, 1, 2, 4, 5, 6):                                          # (logp, index 3, may be null)
        assert res([NULL if j == i else p[j] for j in range(7)]) == 1, i
    for f, ptrs in ((dec, p[:5]), (res, p)):
        assert f(ptrs, C=0) == 1 and f(ptrs, C=-1) == 1
        assert f(ptrs, C=257) == 2
        assert f(ptrs, A=0) == 1 and f(ptrs, B=0) == 1


def test_loss_many_status_codes():
    lib = nat.lib()
    tail = lambda C, B=1, A=10: [B, A, C, 64, 96, 1.0, 3.75, 100.0, 6.0, NULL]
    six, seven = [_buf() for _ in range(6)], [_buf() for _ in range(7)]
    for f, ptrs in ((lib.sqd_loss_many_fwd, six), (lib.sqd_loss_many_bwd, six), (lib.sqd_loss_many_mean_fwd, seven),
                    (lib.sqd_loss_many_mean_bwd, six)):
        for i in range(len(ptrs)):
            assert f(*[NULL if j == i else q for j, q in enumerate(ptrs)], *tail(20)) == 1, i
        assert f(*ptrs, *tail(0)) == 1
        assert f(*ptrs, *tail(257)) == 2
        assert f(*ptrs, *tail(20, A=0)) == 1 and f(*ptrs, *tail(20, B=0)) == 1
    # the <= 16-class entry points keep their own answer
    assert lib.sqd_loss_fwd(*six, *tail(17)) == 1


def test_pad_kernels_status_codes():
    lib = nat.lib()
    a, b, c = _buf(), _buf(), _buf()
    for f in (lib.sqd_channel_pack_fwd, lib.sqd_channel_unpack_fwd):
        assert f(NULL, b, 4, 225, 256, NULL) == 1 and f(a, NULL, 4, 225, 256, NULL) == 1
        assert f(a, b, 0, 225, 256, NULL) == 1
        assert f(a, b, 4, 0, 256, NULL) == 1
        assert f(a, b, 4, 257, 256, NULL) == 1                            # Npad < N
    r = lib.sqd_wgrad_reduce_rows
    assert r(NULL, b, c, 2, 225, 256, 768, 9, 1.0, NULL) == 1 and r(a, NULL, c, 2, 225, 256, 768, 9, 1.0, NULL) == 1
    assert r(a, b, NULL, 2, 225, 256, 768, 9, 1.0, NULL) == 1
    assert r(a, b, c, 0, 225, 256, 768, 9, 1.0, NULL) == 1
    assert r(a, b, c, 2, 257, 256, 768, 9, 1.0, NULL) == 1
    assert r(a, b, c, 2, 225, 256, 768, 4, 1.0, NULL) == 1


def test_head_path_table():
    assert ops.head_path(1) == 'narrow' and ops.head_path(16) == 'narrow'
    assert ops.head_path(17) == 'many' and ops.head_path(256) == 'many'
    for C in (0, 257):
        with pytest.raises(ValueError, match='256'):
            ops.head_path(C)
    assert ops.detect_fn(3, 64, 16848) is ops.detect and ops.detect_fn(16, 65, 16848) is ops.detect_wide
    assert ops.detect_fn(17, 64, 16848) is ops.detect_many and ops.detect_fn(80, 1024, A_MAX) is ops.detect_many
    assert ops.filter_fn(3, 64, 100) is ops.filter_dense and ops.filter_fn(20, 64, 100) is ops.filter_dense_many
    with pytest.raises(ValueError, match='1024'):
        ops.detect_fn(20, 1025, 100)
    assert ops.loss_fns(16)[0] is ops.loss_fwd and ops.loss_fns(17) == (ops.loss_fwd_many, ops.loss_mean_fwd_many, ops.loss_bwd_many,
                                                                       ops.loss_mean_bwd_many)


def test_many_class_buffers():
    """Past 16 classes the detect is always the two-launch form: its buffers carry the wide workspace whatever K and A are."""
    dev = torch.device('cpu')
    B, A = 2, 216
    assert ops._det_buffers(B, 64, dev, A, 3)[5].numel() == ops.det_workspace_words(B, A)
    assert ops._det_buffers(B, 64, dev, A, 16)[5].numel() == ops.det_workspace_words(B, A)
    assert ops._det_buffers(B, 64, dev, A, 17)[5].numel() == ops.det_workspace_words_wide(B, A, 64)
    assert ops.det_buffers_packed(B, 100, dev, A, 80)[0][5].numel() == ops.det_workspace_words_wide(B, A, 100)
    assert ops.det_buffers_packed(B, 64, dev, A)[0][5].numel() == ops.det_workspace_words(B, A)


def test_convdet_width_helper():
    for C in (3, 7, 11, 15):
        N, Npad = ops.convdet_width(9, C)
        assert N == Npad == 9 * (C + 5) and not ops.convdet_padded(9, C)
    for C, want in ((5, 128), (20, 256), (80, 768), (1, 64), (256, 2368)):
        N, Npad = ops.convdet_width(9, C)
        assert N == 9 * (C + 5) and Npad == want and ops.convdet_padded(9, C)
        assert Npad % 64 == 0 and 0 < Npad - N < 64
    for C in range(1, 257):
        assert not ops.convdet_padded(4, C) and not ops.convdet_padded(8, C)


def test_make_cfg_refusals():
    for C in (0, -1, 257):
        with pytest.raises(ValueError, match='256'):
            sqd.make_cfg(input_size=(64, 96), num_classes=C)
    with pytest.raises(ValueError, match='256'):
        sqd.make_cfg(input_size=(64, 96), num_classes=5, class_names=('a', 'b', 'c'))
    with pytest.raises(ValueError, match='256'):
        sqd.make_cfg(input_size=(64, 96), class_names=('a', 'b'))
    cfg = sqd.make_cfg(input_size=(64, 96))
    assert cfg.num_classes == 3 and cfg.class_names == ('Car', 'Pedestrian', 'Cyclist')
    cfg = sqd.make_cfg(input_size=(64, 96), num_classes=80)
    assert len(cfg.class_names) == 80 and len(set(cfg.class_names)) == 80
    assert sqd.make_cfg(input_size=(64, 96), num_classes=256).num_classes == 256


@pytest.mark.parametrize('C', [3, 7])
def test_aligned_widths_plan_exactly_as_without_padding(C, monkeypatch):
    kw = dict(batch=2, input_size=(64, 96), num_classes=C)
    inf, trn = plan.inference_launch_plan(**kw), plan.training_launch_plan(**kw)
    kitti = (plan.inference_launch_plan(num_classes=C), plan.training_launch_plan(num_classes=C))
    monkeypatch.setattr(ops, 'convdet_pad_width', lambda N: int(N))       # the padding helper forced off
    assert plan.inference_launch_plan(**kw) == inf and plan.training_launch_plan(**kw) == trn
    assert (plan.inference_launch_plan(num_classes=C), plan.training_launch_plan(num_classes=C)) == kitti
    assert not any('pack' in name or 'reduce_rows' in name for name, _ in inf + trn)
    assert any(tag.startswith(f'9tap C768 N{9 * (C + 5)} ') for _, tag in inf)


def test_twenty_classes_plan_lists_padded_convdet_and_pack_unpack():
    kw = dict(batch=2, input_size=(64, 96), num_classes=20)
    inf, trn = plan.inference_launch_plan(**kw), plan.training_launch_plan(**kw)
    assert ('convdet_pack', 'pack N225 <- 256 4x6') in inf and inf[-1] == ('detect', 'detect_many A216 K64')
    assert inf[-3][1] == '9tap C768 N256 4x6'
    names = [n for n, _ in trn]
    i_pack, i_unpack, i_rows = names.index('convdet_pack'), names.index('convdet_unpack'), names.index('wgrad_reduce_rows')
    assert trn[i_pack - 1][1] == '9tap C768 N256 4x6' and names[i_pack + 1:i_pack + 3] == ['loss_fwd', 'loss_bwd']
    assert i_unpack == i_pack + 3 and trn[i_unpack] == ('convdet_unpack', 'unpack N225 -> 256 4x6')
    assert trn[i_unpack + 1][1] == 'wgrad 9tap C768 N256 4x6' and i_rows == i_unpack + 2
    assert trn[i_rows] == ('wgrad_reduce_rows', 'N225 of 256 C768')
    assert trn[i_rows + 1][1] == '9tap C256 N768 4x6'                     # the data gradient reads the padded width as its C
    assert trn[-1] == ('wgrad_reduce_batched', '30 layers')               # ConvDet's slabs are not in the batched reduction
    assert not any('N225 ' in tag.split('<-')[0] and tag.startswith('9tap') for _, tag in trn)
