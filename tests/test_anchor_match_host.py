"""CPU tier of the IoU-threshold matcher: the host twin ``boxes.anchor_match`` against the independent restatement of
tests/anchor_match_ref.py bit for bit on the shared case list; the case list's own coverage (extras, a band, overflow where it is
meant) and its teeth (every mutant of the restatement changes some output); ``config.check_match``; the argument checks of
``ops.anchor_match`` and of the raw entry, which come before any launch; and the feature switched off."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import anchor_match_ref as M
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import annotations, boxes, ops
from squeezedet_pytorch_amd.config import check_match

CASES = M.cases()
ALL = CASES + [M.kitti_case()]
OUTPUTS = ('anchor_idx', 'box_idx', 'deltas', 'offsets', 'ignore', 'overflow')


def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    if x.dtype == np.float32:
        return y.dtype == np.float32 and x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32))
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize('case', ALL, ids=lambda c: c['name'])
def test_host_twin_equals_the_restatement(case):
    ref = M.reference(case)
    idx, _ = M.primaries(case)
    got = boxes.anchor_match(case['anchors'], case['boxes'], idx, case['pos_iou'], case['ign_iou'], case['max_extra'], ignore=case['ignore_in'])
    for name, g in zip(OUTPUTS, got):
        assert _same(g, ref[name]), (case['name'], name)
    A, B, total = case['anchors'].shape[0], len(case['boxes']), sum(b.shape[0] for b in case['boxes'])
    assert got[0].shape == (total + B * case['max_extra'],)
    offs = np.cumsum([0] + [b.shape[0] for b in case['boxes']])
    assert got[3].tolist() == [int(offs[b]) + b * case['max_extra'] for b in range(B + 1)]
    for b in range(B):                                  # the SparseGT contract: the anchors of an image are distinct
        seg = got[0][got[3][b]:got[3][b + 1]]
        seg = seg[seg < A]
        assert len(set(seg.tolist())) == seg.shape[0]


@pytest.mark.parametrize('case', ALL, ids=lambda c: c['name'])
def test_case_covers_what_it_is_for(case):
    """Every case has an extra positive and a band anchor somewhere, overflows exactly where it is meant to, and every box keeps its
    primary.  (A = 1 cannot have an extra: the one anchor is the primary of every image that has a box.)"""
    ref = M.reference(case)
    A = case['anchors'].shape[0]
    print(case['name'], 'extras', ref['extras'].tolist(), 'band', ref['band'].tolist(), 'overflow', ref['overflow'].tolist())
    if A == 1:
        assert ref['extras'].sum() == 0 and ref['band'].sum() == 0
    else:
        assert ref['extras'].sum() >= 1 and ref['band'].sum() >= 1
    assert bool(ref['overflow'].any()) == case['overflows']
    assert np.array_equal(ref['overflow'], np.maximum(ref['extras'] - case['max_extra'], 0))
    idx, _ = M.primaries(case)
    for b, bx in enumerate(case['boxes']):
        assert ref['extras'][b] == 0 and ref['band'][b] == 0 if bx.shape[0] == 0 else True
        seg = ref['anchor_idx'][ref['offsets'][b]:ref['offsets'][b + 1]]
        assert np.array_equal(seg[:bx.shape[0]], idx[b])
        assert (seg[bx.shape[0] + min(int(ref['extras'][b]), case['max_extra']):] == A).all()


def test_case_list_is_the_one_the_rule_needs():
    names = [c['name'] for c in CASES]
    assert len(set(names)) == len(names)
    for g in ('64x96', '48x80', 'seed20_80x112'):
        assert f'grid-{g}' in names
    assert {c['anchors'].shape[0] for c in CASES if c['name'].startswith('cloud-')} == {1, 31, 32, 33, 1023, 1025}
    assert any(any(b.shape[0] == 0 for b in c['boxes']) for c in CASES)
    assert any(max(b.shape[0] for b in c['boxes']) > 256 for c in CASES)
    caps = {c['name']: c['max_extra'] for c in CASES if c['name'].startswith('capacity-')}
    most = int(M.reference(next(c for c in CASES if c['name'] == 'capacity-exact'))['extras'].max())
    assert caps == {'capacity-0': 0, 'capacity-exact': most, 'capacity-one-fewer': most - 1}
    k = M.kitti_case()
    assert k['anchors'].shape == (16848, 4) and len(k['boxes']) == 3
    assert np.array_equal(k['anchors'], np.asarray(sqd.make_cfg().anchors, np.float64))


def test_tie_goes_to_the_lowest_box():
    case = next(c for c in CASES if c['name'] == 'identical-boxes')
    ref = M.reference(case)
    assert np.array_equal(case['boxes'][0][0], case['boxes'][0][1]) and np.array_equal(case['boxes'][1][1], case['boxes'][1][2])
    n0 = case['boxes'][0].shape[0]
    seg = slice(ref['offsets'][0] + n0, ref['offsets'][0] + n0 + int(ref['extras'][0]))
    assert 0 in ref['box_idx'][seg] and 1 not in ref['box_idx'][seg]


def test_threshold_is_inclusive():
    """``boundary-pos``: pos_iou and ign_iou are the computed overlaps of two (box, anchor) pairs; both anchors are on the upper side."""
    case = next(c for c in CASES if c['name'] == 'boundary-pos')
    ref, strict = M.reference(case), M.reference(case, 'strict_thresholds')
    j_pos, j_ign = case['edge']
    ov = M.overlaps(case['boxes'][0], case['anchors'])
    assert ov[:, j_pos].max() == case['pos_iou'] and ov[:, j_ign].max() == case['ign_iou']
    n = case['boxes'][0].shape[0]
    assert j_pos in ref['anchor_idx'][n:].tolist() and j_pos not in strict['anchor_idx'][n:].tolist()
    assert ref['ignore'][0, j_ign] and not strict['ignore'][0, j_ign] and not ref['ignore'][0, j_pos] and strict['ignore'][0, j_pos]


@pytest.mark.parametrize('mutant', M.MUTANTS)
def test_every_mutant_changes_some_output(mutant):
    moved = [c['name'] for c in CASES if any(not _same(M.reference(c)[k], M.reference(c, mutant)[k]) for k in OUTPUTS)]
    print(mutant, moved)
    assert moved, f'{mutant}: no case tells it from the rule'


# ---- configuration -----------------------------------------------------------------------------------------------------------------------

def _cfg(**kw):
    return SimpleNamespace(**kw)


def test_check_match():
    assert check_match(_cfg(), 'x') is None                                      # a cfg without the fields: off
    cfg = sqd.make_cfg()
    assert (cfg.match_iou, cfg.match_ignore_iou, cfg.match_max_extra) == (None, None, 512) and check_match(cfg, 'x') is None
    assert check_match(_cfg(sparse_gt=True, match_iou=0.5), 'x') == (0.5, 0.5, 512)              # no band
    assert check_match(_cfg(sparse_gt=True, match_iou=0.5, match_ignore_iou=0.4, match_max_extra=0), 'x') == (0.5, 0.4, 0)
    assert check_match(_cfg(sparse_gt=True, match_iou=1, match_ignore_iou=1.0, match_max_extra=np.int64(7)), 'x') == (1.0, 1.0, 7)
    assert sqd.make_cfg(sparse_gt=True, match_iou=0.6, match_ignore_iou=0.5).match_iou == 0.6
    with pytest.raises(ValueError, match='sparse_gt'):
        check_match(_cfg(match_iou=0.5), 'x')
    with pytest.raises(ValueError, match='sparse_gt'):
        sqd.make_cfg(match_iou=0.5)
    for bad in (0.0, -0.5, 1.5, float('nan'), float('inf'), 'half', True):
        with pytest.raises(ValueError, match='match'):
            check_match(_cfg(sparse_gt=True, match_iou=bad), 'x')
        with pytest.raises(ValueError, match='match'):
            check_match(_cfg(sparse_gt=True, match_iou=0.9, match_ignore_iou=bad), 'x')
    with pytest.raises(ValueError, match='match_ignore_iou <= match_iou'):
        check_match(_cfg(sparse_gt=True, match_iou=0.4, match_ignore_iou=0.5), 'x')
    with pytest.raises(ValueError, match='needs match_iou'):
        check_match(_cfg(sparse_gt=True, match_ignore_iou=0.5), 'x')
    for bad in (-1, 1.5, '8', None, True):
        with pytest.raises(ValueError, match='match_max_extra'):
            check_match(_cfg(sparse_gt=True, match_iou=0.5, match_max_extra=bad), 'x')
    # the loader and the collate helper ask the same question
    from squeezedet_pytorch_amd.train_data import TrainLoader
    from squeezedet_pytorch_amd.trainer import encode_sparse_batch
    import ignore_ref as IR
    cfg = sqd.make_cfg(input_size=(70, 100))
    cfg.match_iou = 0.5
    with pytest.raises(ValueError, match='sparse_gt'):
        TrainLoader(IR.FlaggedDataset('deleted'), cfg)
    with pytest.raises(ValueError, match='sparse_gt'):
        encode_sparse_batch({'image': torch.zeros(1, 3, 70, 100)}, cfg)
    cfg.sparse_gt = True
    assert TrainLoader(IR.FlaggedDataset('deleted'), cfg).match == (0.5, 0.5, 512)
    assert TrainLoader(IR.FlaggedDataset('deleted'), sqd.make_cfg(input_size=(70, 100))).match is None


def test_host_twin_refuses_bad_arguments():
    a, b, i = np.array([[20., 20., 11., 11.]]), [np.array([[10, 10, 30, 30]], np.float32)], [np.array([0])]
    for pos, ign, cap in ((0.0, 0.0, 1), (0.5, 0.6, 1), (1.5, 0.5, 1), (float('nan'), 0.5, 1), (0.5, float('nan'), 1), (0.5, 0.4, -1), (0.5, 0.4, 1.5)):
        with pytest.raises(ValueError):
            boxes.anchor_match(a, b, i, pos, ign, cap)
    with pytest.raises(ValueError):
        boxes.anchor_match(a, b, [], 0.5, 0.4, 1)
    with pytest.raises(ValueError):
        boxes.anchor_match(a, b, [np.array([0, 0])], 0.5, 0.4, 1)
    got = boxes.anchor_match(a, b, i, 0.5, None, 2)                               # ign_iou None: no band
    assert got[0].tolist() == [0, 1, 1] and not got[4].any()


def test_wrapper_checks_come_before_the_library(monkeypatch):
    from squeezedet_pytorch_amd import _native as nat
    monkeypatch.setattr(nat, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was touched')))
    sgt = ops.sparse_gt_from_dense(torch.zeros(2, 40, 12))
    a64 = torch.zeros(40, 4, dtype=torch.float64)
    for pos, ign, cap in ((0.0, None, 1), (0.5, 0.6, 1), (float('nan'), None, 1), (0.5, 0.4, -1), (0.5, 0.4, 2.0)):
        with pytest.raises(ValueError, match='match|max_extra'):
            ops.anchor_match(sgt, a64, pos, ign, cap)
    with pytest.raises(ValueError, match='SparseGT'):
        ops.anchor_match(tuple(sgt), a64, 0.5, 0.4, 1)
    with pytest.raises(ValueError, match='float64'):
        ops.anchor_match(sgt, a64.float(), 0.5, 0.4, 1)
    with pytest.raises(ValueError, match='ignore must be int32'):
        ops.anchor_match(sgt, a64, 0.5, 0.4, 1, ignore=torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match='ignore must be int32'):
        ops.anchor_match(sgt, a64, 0.5, 0.4, 1, ignore=torch.zeros(2, 2))
    with pytest.raises(ValueError, match='2\\^31'):
        ops.anchor_match(sgt, a64, 0.5, 0.4, 2 ** 30)
    with pytest.raises(ValueError, match='agree on total'):
        ops.anchor_match(sgt._replace(deltas=torch.zeros(3, 4)), a64, 0.5, 0.4, 1)
    with pytest.raises(ValueError, match='GPU'):
        ops.anchor_match(sgt, a64, 0.5, 0.4, 1)
    with pytest.raises(ValueError):
        annotations.encode_annotations([np.array([0])], [np.array([[5, 5, 30, 30]], np.float32)], np.zeros((40, 4)), 3, match=(0.5, 0.4, 8))
    with pytest.raises(ValueError, match='return_overflow'):
        annotations.encode_annotations([np.array([0])], [np.array([[5, 5, 30, 30]], np.float32)], np.zeros((40, 4)), 3, dense=False,
                                       return_overflow=True)


def test_raw_entry_status_codes():
    """Malformed arguments and the limits are answered on the host, before any launch (no device is needed to ask)."""
    from squeezedet_pytorch_amd import _native as nat
    buf = (ctypes.c_int * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)

    def call(thr=(0.5, 0.4), total=1, B=1, A=4, cap=2, **nulls):
        names = ('boxes', 'class_ids', 'box_offsets', 'anchor_idx', 'deltas', 'anchors', 'ignore_in', 'thresholds', 'workspace', 'out_anchor_idx',
                 'out_boxes', 'out_deltas', 'out_class_ids', 'out_offsets', 'ignore_out', 'overflow')
        args = [null if nulls.get(n) else p for n in names]
        args[7] = None if nulls.get('thresholds') else (ctypes.c_double * 2)(*thr)
        return nat.lib().sqd_anchor_match_fwd(*args, total, B, A, cap, null)
    for name in ('boxes', 'class_ids', 'box_offsets', 'anchor_idx', 'deltas', 'anchors', 'thresholds', 'workspace', 'out_anchor_idx', 'out_boxes',
                 'out_deltas', 'out_class_ids', 'out_offsets', 'ignore_out', 'overflow'):
        assert call(**{name: True}) == nat.ERR_BAD_ARG, name
    for thr in ((0.0, 0.0), (0.5, 0.0), (0.5, 0.6), (1.5, 0.5), (float('nan'), 0.5), (0.5, float('nan')), (-0.5, -0.6)):
        assert call(thr=thr) == nat.ERR_BAD_ARG, thr
    assert call(cap=-1) == nat.ERR_BAD_ARG and call(total=-1) == nat.ERR_BAD_ARG and call(B=0) == nat.ERR_BAD_ARG and call(A=0) == nat.ERR_BAD_ARG
    assert call(A=2 ** 20 + 1) == nat.ERR_UNSUPPORTED and call(B=65536) == nat.ERR_UNSUPPORTED
    assert call(total=2 ** 31 - 1, cap=1) == nat.ERR_UNSUPPORTED and call(total=0, B=2, cap=2 ** 30) == nat.ERR_UNSUPPORTED


# ---- the feature switched off --------------------------------------------------------------------------------------------------------------

def test_off_defaults_leave_the_collate_helper_as_it_was(monkeypatch):
    """``match_iou`` None (the default), or a cfg without the fields: ``encode_sparse_batch`` asks ``encode_annotations`` exactly what it
    asked before the matcher existed -- no ``match`` argument at all -- and returns the same keys; with ``match_iou`` set it asks for the
    matcher and the batch gains ``'gt_ignore'`` and ``'gt_match_overflow'``."""
    from squeezedet_pytorch_amd.trainer import encode_sparse_batch
    asked = []

    def fake(class_ids, boxes_list, anchors, num_classes, **kw):
        asked.append(kw)
        if kw.get('match') is not None:
            return 'sgt+', 'bits', 'overflow'
        return ('sgt', 'bits') if kw.get('ignore_overlap') is not None else ('sgt' if not kw.get('dense', True) else 'gt')
    monkeypatch.setattr(annotations, 'encode_annotations', fake)
    batch = {'image': torch.zeros(1, 3, 70, 100), 'gt_boxes': [np.array([[5, 5, 30, 30]], np.float32)], 'gt_class_ids': [np.array([0])],
             'gt_ignore_boxes': [np.zeros((0, 4), np.float32)]}
    bare = sqd.make_cfg(input_size=(70, 100), device='cpu')
    for k in ('match_iou', 'match_ignore_iou', 'match_max_extra'):
        delattr(bare, k)
    for cfg in (sqd.make_cfg(input_size=(70, 100), device='cpu'), bare):
        asked.clear()
        out = encode_sparse_batch(batch, cfg)
        assert set(out) == {'image', 'gt'} and out['gt'] == 'gt' and asked == [{'device': 'cpu', 'dense': True}]
        cfg.sparse_gt = True
        asked.clear()
        out = encode_sparse_batch(batch, cfg)
        assert set(out) == {'image', 'gt_sparse'} and out['gt_sparse'] == 'sgt' and asked == [{'device': 'cpu', 'dense': False}]
        cfg.ignore_overlap = 0.5
        asked.clear()
        out = encode_sparse_batch(batch, cfg)
        assert set(out) == {'image', 'gt_sparse', 'gt_ignore'} and (out['gt_sparse'], out['gt_ignore']) == ('sgt', 'bits')
        assert len(asked) == 1 and set(asked[0]) == {'device', 'dense', 'ignore_boxes_list', 'ignore_overlap'}
        dense = {'image': batch['image'], 'gt': torch.zeros(1, 4, 12)}
        assert encode_sparse_batch(dense, cfg) is dense and len(asked) == 1
    on = sqd.make_cfg(input_size=(70, 100), device='cpu', sparse_gt=True, match_iou=0.5, match_ignore_iou=0.4, match_max_extra=16)
    asked.clear()
    out = encode_sparse_batch(batch, on)
    assert set(out) == {'image', 'gt_sparse', 'gt_ignore', 'gt_match_overflow'}
    assert (out['gt_sparse'], out['gt_ignore'], out['gt_match_overflow']) == ('sgt+', 'bits', 'overflow')
    assert asked[0]['match'] == (0.5, 0.4, 16) and asked[0]['ignore_boxes_list'] is None and asked[0]['ignore_overlap'] is None
    on.ignore_overlap = 0.5
    asked.clear()
    encode_sparse_batch(batch, on)
    assert asked[0]['match'] == (0.5, 0.4, 16) and asked[0]['ignore_overlap'] == 0.5 and len(asked[0]['ignore_boxes_list']) == 1
