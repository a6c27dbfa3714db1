"""CPU tier: the wide fused detect's host side (csrc/detect_wide.hip ``sqd_detect_wide_fwd`` / ``sqd_filter_wide_fwd`` /
``sqd_detect_wide_workspace_words``, ``ops.detect_path``).  Every refusal is decided before any launch, so the status codes can be
exercised without a GPU: the pointers handed in are host buffers that a refused call never touches."""
import ctypes

import pytest
import torch

from squeezedet_pytorch_amd import _native as nat, ops

A_MAX = 1 << 20


def _buf(nbytes=4096):
    """A 16-byte aligned host address inside a buffer that stays alive with the returned pointer."""
    raw = ctypes.create_string_buffer(nbytes + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    p = ctypes.c_void_p(addr)
    p._keep = raw
    return p


def _detect_args(B=1, A=100, C=3, K=64, ws_words=None, null=()):
    ptrs = {n: _buf() for n in ('pred', 'anchors', 'scales', 'shifts', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx')}
    for n in null:
        ptrs[n] = ctypes.c_void_p(0)
    if ws_words is None:
        ws_words = B * (-(-A // 4) * 4)
    return ([ptrs[n] for n in ('pred', 'anchors', 'scales', 'shifts', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx')]
            + [B, A, C, 384, 1248, K, 0.4, 0.3, ws_words, ctypes.c_void_p(0)])


def _filter_args(B=1, A=100, C=3, K=64, ws_words=None, null=()):
    ptrs = {n: _buf() for n in ('ids', 'scores', 'boxes', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx')}
    for n in null:
        ptrs[n] = ctypes.c_void_p(0)
    if ws_words is None:
        ws_words = B * (-(-A // 4) * 4)
    return ([ptrs[n] for n in ('ids', 'scores', 'boxes', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx')]
            + [B, A, C, K, 0.4, 0.3, ws_words, ctypes.c_void_p(0)])


def test_wide_symbols_are_exported_and_declared():
    lib = nat.lib()
    for name in ('sqd_detect_wide_fwd', 'sqd_filter_wide_fwd', 'sqd_detect_wide_workspace_words'):
        assert hasattr(lib, name) and name in nat._SIGNATURES
    for name in ('detect_wide', 'filter_dense_wide', 'det_workspace_words_wide', 'detect_path'):
        assert callable(getattr(ops, name))


def test_detect_wide_status_codes():
    f = nat.lib().sqd_detect_wide_fwd
    for n in ('pred', 'anchors', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx'):
        assert f(*_detect_args(null=(n,))) == 1, f'null {n}'
    assert f(*_detect_args(K=0)) == 1
    assert f(*_detect_args(K=-3)) == 1
    assert f(*_detect_args(A=0)) == 1
    assert f(*_detect_args(B=0)) == 1
    assert f(*_detect_args(C=0)) == 1
    assert f(*_detect_args(K=1025)) == 2
    assert f(*_detect_args(A=A_MAX + 1)) == 2
    assert f(*_detect_args(C=17)) == 2
    assert f(*_detect_args(A=101, ws_words=103)) == 1                     # ceil4(101) = 104 words needed
    assert f(*_detect_args(B=3, A=A_MAX, K=1024, ws_words=3 * A_MAX - 1)) == 1
    assert f(*_detect_args(ws_words=0)) == 1
    a = _detect_args()
    a[4] = ctypes.c_void_p(a[4].value + 4)                                # misaligned workspace
    assert f(*a) == 1


def test_filter_wide_status_codes():
    f = nat.lib().sqd_filter_wide_fwd
    for n in ('ids', 'scores', 'boxes', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx'):
        assert f(*_filter_args(null=(n,))) == 1, f'null {n}'
    assert f(*_filter_args(K=0)) == 1
    assert f(*_filter_args(K=1025)) == 2
    assert f(*_filter_args(A=A_MAX + 1)) == 2
    assert f(*_filter_args(C=17)) == 2
    assert f(*_filter_args(A=101, ws_words=103)) == 1


WIDE_ENTRIES = ('sqd_detect_wide_fwd', 'sqd_filter_wide_fwd', 'sqd_detect_many_fwd', 'sqd_filter_many_fwd', 'sqd_detect_nms_fwd',
                'sqd_filter_nms_fwd', 'sqd_detect_views_fwd')

# two faults in one call: which of them the entry point reports.  `mode` exists for the rule-taking entry points only, `ready`
# (keys_ready) for the two nms ones, V for the views one; a fault an entry point cannot express is not in its row below.
DOUBLE_FAULTS = {
    'K limit + short workspace': dict(K=1025, ws_words=0),
    'A limit + short workspace': dict(A=A_MAX + 1, ws_words=0),
    'class limit + short workspace': dict(C=257, ws_words=0),
    'K limit + bad mode': dict(K=1025, mode=3),
    'K limit + negative score_thresh': dict(K=1025, thr=-0.1),
    'null pointer + K limit': dict(null=True, K=1025),
    'null pointer + short workspace': dict(null=True, ws_words=0),
    'keys_ready + 17 classes': dict(ready=1, C=17),
    'keys_ready + class limit': dict(ready=1, C=257),
    'keys_ready + short workspace': dict(ready=1, ws_words=0),
    'V = 0 + K = 1025': dict(V=0, K=1025),
    'pooled row limit + short workspace': dict(V=1 << 18, A=5, ws_words=0),
}


def _double_fault_call(lib, entry, B=1, A=100, C=3, K=64, V=2, ws_words=None, null=False, mode=None, thr=None, ready=None):
    """The status of one call, or None where the entry point has no such argument."""
    stream = ctypes.c_void_p(0)
    views, rule, nms = entry == 'sqd_detect_views_fwd', entry in WIDE_ENTRIES[4:], entry.endswith('_nms_fwd')
    if ((mode is not None or thr is not None) and not rule) or (ready is not None and not nms) or (V != 2 and not views):
        return None
    mode, thr, ready = mode or 0, 0.3 if thr is None else thr, ready or 0
    first = ctypes.c_void_p(0) if null else _buf()
    if views:
        if ws_words is None:
            ws_words = B * max(V, 1) * (-(-A // 4) * 4)
        return lib.sqd_detect_views_fwd(first, *[_buf() for _ in range(8)], B, V, A, C, 384, 1248, K, 0.4, thr, ws_words, mode, 0.5, 0, stream)
    args = (_filter_args if 'filter' in entry else _detect_args)(B, A, C, K, ws_words)
    args[0] = first
    args[-3] = thr
    if nms:
        args = args[:-1] + [mode, 0.5, 0, ready, stream]
    return getattr(lib, entry)(*args)


def _double_fault_statuses(lib):
    return {e: {name: s for name, kw in DOUBLE_FAULTS.items() if (s := _double_fault_call(lib, e, **kw)) is not None} for e in WIDE_ENTRIES}


# recorded from the library before the family moved behind one launcher (csrc/detect_wide.hip: launch_wide), by this very table
_BIT_MATRIX_ROW = {'K limit + short workspace': 2, 'A limit + short workspace': 2, 'class limit + short workspace': 2,
                   'null pointer + K limit': 1, 'null pointer + short workspace': 1}
_RULE_ROW = dict(_BIT_MATRIX_ROW, **{'K limit + bad mode': 1, 'K limit + negative score_thresh': 1})
DOUBLE_FAULT_STATUS = {
    'sqd_detect_wide_fwd': _BIT_MATRIX_ROW, 'sqd_filter_wide_fwd': _BIT_MATRIX_ROW,
    'sqd_detect_many_fwd': _BIT_MATRIX_ROW, 'sqd_filter_many_fwd': _BIT_MATRIX_ROW,
    'sqd_detect_nms_fwd': dict(_RULE_ROW, **{'keys_ready + 17 classes': 1, 'keys_ready + class limit': 2, 'keys_ready + short workspace': 1}),
    'sqd_filter_nms_fwd': dict(_RULE_ROW, **{'keys_ready + 17 classes': 1, 'keys_ready + class limit': 1, 'keys_ready + short workspace': 1}),
    'sqd_detect_views_fwd': dict(_RULE_ROW, **{'V = 0 + K = 1025': 1, 'pooled row limit + short workspace': 2}),
}


def test_refusal_precedence_of_two_faults_at_once():
    """Every wide-family entry point refuses a call with two faults with the status it always gave: a null pointer or a size below 1
    (status 1) before a bad rule (1), before a limit (2), before the workspace (1), before keys_ready misuse (1).  Nothing is launched."""
    got = _double_fault_statuses(nat.lib())
    assert set(DOUBLE_FAULT_STATUS) == set(WIDE_ENTRIES) and all(len(v) >= 5 for v in DOUBLE_FAULT_STATUS.values())
    for e in WIDE_ENTRIES:
        assert got[e] == DOUBLE_FAULT_STATUS[e], e


def test_wide_workspace_words():
    w = nat.lib().sqd_detect_wide_workspace_words
    Bs, As, Ks = (1, 2, 20, 64), (1, 3, 4, 5, 64, 16848, 25597, 32400, 65535, 65536, 73440, A_MAX), (1, 64, 65, 256, 1024)
    for B in Bs:
        for A in As:
            for K in Ks:
                n = w(B, A, K)
                assert n >= B * (-(-A // 4) * 4), (B, A, K, n)
                assert ops.det_workspace_words_wide(B, A, K) == n
    for K in Ks:                                                          # non-decreasing in each argument
        for A in As:
            assert all(w(b0, A, K) <= w(b1, A, K) for b0, b1 in zip(Bs, Bs[1:]))
        for B in Bs:
            assert all(w(B, a0, K) <= w(B, a1, K) for a0, a1 in zip(As, As[1:]))
    for B in Bs:
        for A in As:
            assert all(w(B, A, k0) <= w(B, A, k1) for k0, k1 in zip(Ks, Ks[1:]))
    for B, A, K in ((1, 1, 1025), (1, A_MAX + 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1 << 12, A_MAX, 64)):
        assert w(B, A, K) == -1, (B, A, K)
    with pytest.raises(ValueError, match='1024'):
        ops.det_workspace_words_wide(1, 1, 1025)
    with pytest.raises(ValueError, match='2\\^20'):
        ops.det_workspace_words_wide(1, A_MAX + 1, 1)


def test_detect_path_table():
    assert ops.detect_path(64, 25596) == 'narrow'
    assert ops.detect_path(1, 1) == 'narrow'
    assert ops.detect_path(65, 1) == 'wide'
    assert ops.detect_path(1, 25597) == 'wide'
    assert ops.detect_path(1024, A_MAX) == 'wide'
    with pytest.raises(ValueError, match='1024'):
        ops.detect_path(1025, 1)
    with pytest.raises(ValueError, match='2\\^20'):
        ops.detect_path(1, A_MAX + 1)
    with pytest.raises(ValueError):
        ops.detect_path(0, 1)


def test_buffer_sizes():
    """Narrow parameters get exactly the narrow workspace (keys + one arrival counter per image); wide parameters the wide one."""
    dev = torch.device('cpu')
    B, A = 20, 16848
    assert ops._det_buffers(B, 64, dev, A)[5].numel() == ops.det_workspace_words(B, A) == B * A + B
    assert ops.det_buffers_packed(B, 64, dev, A)[0][5].numel() == B * A + B
    assert len(ops._det_buffers(B, 64, dev)) == 5 and len(ops._det_buffers(B, 256, dev)) == 5
    for K, A2 in ((65, A), (256, A), (64, 32400), (1024, 73440)):
        want = ops.det_workspace_words_wide(B, A2, K)
        assert ops._det_buffers(B, K, dev, A2)[5].numel() == want
        bufs, flat = ops.det_buffers_packed(B, K, dev, A2)
        assert bufs[5].numel() == want and tuple(bufs[1].shape) == (B, K) and tuple(bufs[3].shape) == (B, K, 4)
