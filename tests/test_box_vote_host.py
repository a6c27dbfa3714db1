"""CPU tier: box voting's host side (DESIGN.md section 3 "Box voting"; csrc/detect_wide.hip ``sqd_detect_vote_fwd`` /
``sqd_filter_vote_fwd`` / ``sqd_detect_views_vote_fwd``; ``ops`` ``vote_iou`` / ``return_votes``; ``cfg.box_vote_iou``) and the numpy
reference tests/box_vote_ref.py.  Every refusal is decided before any launch, so the status codes can be exercised without a GPU: the
pointers handed in are host buffers that a refused call never touches."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import box_vote_ref as vref
import nms_ref
from squeezedet_pytorch_amd import _native as nat, ops

ENTRIES = ('sqd_detect_vote_fwd', 'sqd_filter_vote_fwd', 'sqd_detect_views_vote_fwd')
A_MAX = 1 << 20
F = np.float32


def _buf(nbytes=4096):
    raw = ctypes.create_string_buffer(nbytes + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    p._keep = raw
    return p


NULL = ctypes.c_void_p(0)
# the pointer arguments of each entry in order; the ones in brackets may be null
POINTERS = {
    'sqd_detect_vote_fwd': ('pred', 'anchors', '[scales]', '[shifts]', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx'),
    'sqd_filter_vote_fwd': ('ids', 'scores', 'boxes', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx'),
    'sqd_detect_views_vote_fwd': ('pred', 'anchors', 'xf', 'keys', 'cnt', 'cls', 'sc', 'bx', 'idx'),
}


def _call(entry, null=(), B=1, A=100, C=3, K=64, V=2, ws_words=None, mode=0, thr=0.3, ready=0, vote=0.5, votes=True):
    ptrs = [NULL if n in null else _buf() for n in POINTERS[entry]]
    views = entry == 'sqd_detect_views_vote_fwd'
    if ws_words is None:
        ws_words = B * (max(V, 1) if views else 1) * (-(-A // 4) * 4)
    tail = [ws_words, mode, 0.5, 0] + ([] if views else [ready]) + [vote, _buf() if votes else NULL, NULL]
    if views:
        args = ptrs + [B, V, A, C, 384, 1248, K, 0.4, thr] + tail
    elif entry == 'sqd_filter_vote_fwd':
        args = ptrs + [B, A, C, K, 0.4, thr] + tail
    else:
        args = ptrs + [B, A, C, 384, 1248, K, 0.4, thr] + tail
    return getattr(nat.lib(), entry)(*args)


def test_symbols_are_exported_declared_and_bound():
    lib = nat.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sqd_hip.h')).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in nat._SIGNATURES
        assert f'int {name}(' in header
        sibling = name.replace('_views_vote_', '_views_').replace('_vote_', '_nms_')
        sig, sib = nat._SIGNATURES[name], nat._SIGNATURES[sibling]
        assert sig == sib[:-1] + [ctypes.c_float, ctypes.c_void_p] + sib[-1:], name      # vote_iou, det_votes before the stream


@pytest.mark.parametrize('entry', ENTRIES)
def test_status_codes(entry):
    for n in POINTERS[entry]:
        if not n.startswith('['):
            assert _call(entry, null=(n,)) == 1, f'null {n}'
    for bad in (0.0, -0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        assert _call(entry, vote=bad) == 1, bad
    assert _call(entry, K=1025) == 2
    assert _call(entry, C=257) == 2
    assert _call(entry, A=A_MAX + 1) == 2
    assert _call(entry, K=0) == 1 and _call(entry, mode=3) == 1 and _call(entry, thr=-0.1) == 1
    assert _call(entry, A=101, ws_words=103) == 1
    # two faults at once: the family's precedence -- a null pointer (1), then the rule and vote_iou (1), then a limit (2), then the workspace (1)
    assert _call(entry, K=1025, vote=1.5) == 1
    assert _call(entry, C=257, vote=float('nan')) == 1
    assert _call(entry, K=1025, ws_words=0) == 2
    assert _call(entry, null=(POINTERS[entry][0],), K=1025) == 1
    # a null det_votes is legal: with it the limit is still what is reported, and 1.0 is inside the range
    assert _call(entry, K=1025, votes=False) == 2
    assert _call(entry, K=1025, vote=1.0, votes=False) == 2
    if entry != 'sqd_detect_views_vote_fwd':
        assert _call(entry, ready=1, C=17) == 1                           # keys_ready passes through as in the sibling
    else:
        assert _call(entry, V=0) == 1 and _call(entry, V=1 << 18, A=5, ws_words=0) == 2


def test_ops_refuse_a_bad_vote_iou_by_name():
    z = torch.zeros(1, 4, 8)
    anchors = torch.zeros(4, 4)
    ids, sc, bx = torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4), torch.zeros(1, 4, 4)
    for bad in (True, False, 0, 0.0, -0.1, 1.5, float('nan'), float('inf'), 'x', np.bool_(True)):
        with pytest.raises(ValueError, match='detect_nms: vote_iou'):
            ops.detect_nms(z, anchors, (64, 64), 3, vote_iou=bad)
        with pytest.raises(ValueError, match='filter_nms: vote_iou'):
            ops.filter_dense_nms(ids, sc, bx, 3, vote_iou=bad)
        with pytest.raises(ValueError, match='detect_views: vote_iou'):
            ops.detect_views(z, anchors, (64, 64), 3, 1, torch.zeros(1, 6), vote_iou=bad)
        with pytest.raises(ValueError, match='detect_fn: vote_iou'):
            ops.detect_fn(3, 64, 100, vote_iou=bad)
        with pytest.raises(ValueError, match='filter_fn: vote_iou'):
            ops.filter_fn(3, 64, 100, vote_iou=bad)
    assert ops.check_vote_iou('t', None) is None and ops.check_vote_iou('t', 1) == 1.0 and ops.check_vote_iou('t', np.float32(0.5)) == 0.5


def test_detect_fn_and_filter_fn_bind_vote_iou():
    # off: exactly the objects of before
    assert ops.detect_fn(3, 64, 16848, vote_iou=None) is ops.detect and ops.detect_fn(3, 256, 16848, vote_iou=None) is ops.detect_wide
    assert ops.detect_fn(20, 64, 16848, vote_iou=None) is ops.detect_many and ops.filter_fn(3, 64, 16848, vote_iou=None) is ops.filter_dense
    f = ops.detect_fn(3, 64, 16848, 'linear', False, 0.7, vote_iou=None)
    assert f.func is ops.detect_nms and f.keywords == {'nms_mode': 'linear', 'nms_sigma': 0.7, 'nms_agnostic': False}
    # on: the rule and vote_iou bound to the scan launch, hard class-wise included
    for C, K, A in ((3, 64, 16848), (3, 1024, 1 << 20), (80, 1, 1)):
        for mode, agn in (('hard', False), ('linear', False), ('gaussian', True), ('hard', True)):
            f = ops.detect_fn(C, K, A, mode, agn, 0.7, vote_iou=0.5)
            assert f.func is ops.detect_nms
            assert f.keywords == {'nms_mode': mode, 'nms_sigma': 0.7, 'nms_agnostic': agn, 'vote_iou': 0.5}
            g = ops.filter_fn(C, K, A, mode, agn, 0.7, vote_iou=0.5)
            assert g.func is ops.filter_dense_nms and g.keywords == f.keywords
    with pytest.raises(ValueError):
        ops.detect_fn(3, 1025, 100, vote_iou=0.5)
    with pytest.raises(ValueError):
        ops.filter_fn(257, 64, 100, vote_iou=0.5)


def test_make_cfg_box_vote_iou():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import config
    assert sqd.make_cfg(device='cpu').box_vote_iou is None
    assert config.check_box_vote(types.SimpleNamespace(), 't') is None               # a cfg without the field: off
    for ok in (0.5, 1.0, 1, np.float32(0.75)):
        assert config.check_box_vote(sqd.make_cfg(device='cpu', box_vote_iou=ok), 't') == float(ok)
    for bad in (0, 0.0, 1.5, -0.5, True, False, 'x', float('nan'), float('inf'), (0.5,)):
        with pytest.raises(ValueError, match='box_vote_iou'):
            sqd.make_cfg(device='cpu', box_vote_iou=bad)


def test_the_lane_signature_follows_box_vote_iou():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import lanes
    cfg = sqd.make_cfg(device='cpu')
    fake = types.SimpleNamespace(cfg=cfg, det=types.SimpleNamespace(model=types.SimpleNamespace(base=types.SimpleNamespace(fuse_detect_keys=True))))
    sig = lanes.DetectStream._params_signature
    off = sig(fake)
    cfg.box_vote_iou = 0.5
    half = sig(fake)
    cfg.box_vote_iou = 0.75
    assert len({off, half, sig(fake)}) == 3
    cfg.box_vote_iou = None
    assert sig(fake) == off
    del cfg.box_vote_iou
    assert sig(fake) == off


# ---- the reference itself ------------------------------------------------------------------------------------------------------------
THR, NMS = 0.3, 0.4


def _hull_ok(box, voter_boxes):
    lo, hi = voter_boxes.min(0), voter_boxes.max(0)
    return bool(np.all(box >= lo) and np.all(box <= hi))


def test_reference_singletons_hull_and_row_order():
    cls, sc, bx = nms_ref.make_case(7, 2, 216, 3)
    K, C = 64, 3
    moved = singles = 0
    for b in range(2):
        emitted = nms_ref.soft_filter(cls[b], sc[b], bx[b], K, NMS, THR, C, 'hard')['anchor_idx']
        assert len(emitted) >= 10
        for iou in (0.5, 0.75, 1.0):
            boxes, votes, voters = vref.vote(cls[b], sc[b], bx[b], K, THR, C, emitted, iou, return_voters=True)
            assert boxes.dtype == F and votes.dtype == np.int32 and votes.min() >= 1
            for row, a in enumerate(emitted):
                assert int(a) in voters[row].tolist() and len(voters[row]) == votes[row]
                assert np.all(cls[b][voters[row]] == cls[b][a])
                if votes[row] == 1:                                         # nobody agreed: the pivot's own bits
                    assert boxes[row].tobytes() == bx[b, a].tobytes()
                    singles += 1
                else:
                    moved += int(boxes[row].tobytes() != bx[b, a].tobytes())
                assert _hull_ok(boxes[row], bx[b][voters[row]]), (b, iou, row)
            # every row is computed on its own: any order (and any subset) of the rows gives the same rows
            perm = np.random.RandomState(b).permutation(len(emitted))
            pb, pv = vref.vote(cls[b], sc[b], bx[b], K, THR, C, emitted[perm], iou)
            assert pb.tobytes() == boxes[perm].tobytes() and np.array_equal(pv, votes[perm])
            if iou == 1.0:
                assert np.all(votes == 1)                                   # (the generator has no two identical boxes)
    assert moved >= 10 and singles >= 10


def test_singleton_identity_in_float64():
    """(s * b) / s returns b for fp32 s > 0 and fp32 b: the product is exact in fp64 and the quotient rounds back to the fp32 value."""
    rs = np.random.RandomState(0)
    s = rs.uniform(1e-6, 1, 200000).astype(F)
    b = np.concatenate([rs.uniform(-2000, 2000, 150000), rs.standard_normal(50000) * 1e-3]).astype(F)
    back = ((s.astype(np.float64) * b.astype(np.float64)) / s.astype(np.float64)).astype(F)
    assert back.tobytes() == b.tobytes()


def test_reference_agnostic_keeps_the_classes_apart_and_nan_never_votes():
    cls, sc, bx = nms_ref.make_case(7, 1, 216, 3)
    emitted = nms_ref.soft_filter(cls[0], sc[0], bx[0], 64, NMS, THR, 3, 'hard', 0.5, True)['anchor_idx']
    boxes, votes, voters = vref.vote(cls[0], sc[0], bx[0], 64, THR, 3, emitted, 0.5, return_voters=True)
    assert all(np.all(cls[0][v] == cls[0][a]) for v, a in zip(voters, emitted))
    # a zero-area pivot has u = 0 / 0 with itself and with its twin: it votes for itself by index, the twin does not
    c = np.zeros(3, np.int64)
    s = np.array([0.9, 0.8, 0.7], F)
    b = np.array([[5, 5, 5, 5], [5, 5, 5, 5], [0, 0, 10, 10]], F)
    out, n = vref.vote(c, s, b, 64, THR, 1, np.array([0, 1, 2]), 0.5)
    assert n.tolist() == [1, 1, 1] and out.tobytes() == b.tobytes()
    # an ineligible candidate (class outside 0 .. C-1) never votes
    c2 = np.array([0, 5, 0], np.int64)
    b2 = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 11]], F)
    out2, n2 = vref.vote(c2, s, b2, 64, THR, 3, np.array([0]), 0.5)
    assert n2.tolist() == [2] and out2[0, 3] > 10 and out2[0, 3] < 11
