"""CPU tier: the NMS modes' reference and host side (tests/nms_ref.py, config.check_nms, ops.nms_mode_index, the C ABI's refusals, the
lane executor's parameter signature).  The reference is itself held to the oracle where the oracle has an answer: ('hard', class-wise)
is ``oracle.filter_detections``, ('hard', agnostic) is ``oracle.nms`` over all top-K boxes."""
import ctypes
import types

import numpy as np
import pytest

import nms_ref as ref
import oracle

NMS, THR = 0.4, 0.3
CASES = [(0, 3, 300, 3, 64), (1, 3, 300, 1, 64), (2, 2, 2000, 20, 200)]      # (seed, B, A, C, K): the GPU tests' generator


def _cases():
    for seed, B, A, C, K in CASES:
        cls, sc, bx = ref.make_case(seed, B, A, C)
        for b in range(B):
            yield (seed, b), cls[b], sc[b], bx[b], C, K


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _same_rows(got, c, s, b, i, case):
    assert np.array_equal(got['anchor_idx'], i), case
    assert np.array_equal(got['class_ids'], c), case
    assert np.array_equal(_bits(got['scores']), _bits(s)), case
    assert np.array_equal(_bits(got['boxes']), _bits(b)), case


def test_hard_classwise_is_the_oracle_filter():
    for case, c, s, bx, C, K in _cases():
        got = ref.soft_filter(c, s, bx, K, NMS, THR, C, 'hard', 0.5, False)
        exp = oracle.filter_detections(c, s, bx, K, NMS, THR, C)
        assert exp is not None and 0 < len(exp['scores']) < K and got['lost'] > 0, case
        _same_rows(got, exp['class_ids'], exp['scores'], exp['boxes'], exp['anchor_idx'], case)


def test_hard_agnostic_is_the_oracle_nms_over_all_top_k_boxes():
    for case, c, s, bx, C, K in _cases():
        got = ref.soft_filter(c, s, bx, K, NMS, THR, C, 'hard', 0.5, True)
        order = np.argsort(-s, kind='stable')[:K]
        keep = order[oracle.nms(bx[order], s[order], NMS)]
        keep = keep[s[keep] > np.float32(THR)]
        assert 0 < len(keep) < K, case
        _same_rows(got, c[keep], s[keep], bx[keep], keep, case)


def test_linear_with_a_threshold_of_one_is_top_k_plus_the_score_threshold():
    for case, c, s, bx, C, K in _cases():
        order = ref.candidates(s, K, THR)
        for agnostic in (False, True):
            for nt in (1.0, 1.5):
                got = ref.soft_filter(c, s, bx, K, nt, THR, C, 'linear', 0.5, agnostic)
                want = order if agnostic else np.concatenate([order[c[order] == k] for k in range(C)])
                _same_rows(got, c[want], s[want], bx[want], want, (case, agnostic, nt))
                assert got['total_decays'] == 0 and got['lost'] == 0


def test_gaussian_against_linear_where_the_two_can_be_ordered():
    """"Every Gaussian score is at most the linear score at the same pick" holds where the linear factor is 1, i.e. for u <=
    nms_thresh: a Gaussian factor is always <= 1.  It does NOT hold where the linear mode decays -- exp(-u^2 / 0.5) > 1 - u for
    every u in (0.4, 1]: 0.726 against 0.6 at u = 0.4, 0.607 against 0.5 at u = 0.5 -- so with nms_thresh = 0.4 neither mode bounds
    the other (this generator's class 7 of case (2, 0) emits 0.679 in Gaussian mode where linear emits 0.561 for the same box at the
    same pick).  What is checked: with nms_thresh >= 1 (linear never decays) every Gaussian row is at most the linear row of the same
    anchor; at nms_thresh = 0.4 no score of either mode exceeds the anchor's own, the first pick of every group is the same
    undecayed box in both, and the per-decay factors order as stated above."""
    seen = 0
    for case, c, s, bx, C, K in _cases():
        for agnostic in (False, True):
            lin1 = ref.soft_filter(c, s, bx, K, 1.0, THR, C, 'linear', 0.5, agnostic)
            gau = ref.soft_filter(c, s, bx, K, NMS, THR, C, 'gaussian', 0.5, agnostic)
            lin = ref.soft_filter(c, s, bx, K, NMS, THR, C, 'linear', 0.5, agnostic)
            score_of = dict(zip(lin1['anchor_idx'].tolist(), lin1['scores'].tolist()))
            for a, sc in zip(gau['anchor_idx'].tolist(), gau['scores'].tolist()):
                assert sc <= score_of[a], (case, agnostic, a)
                seen += 1
            for r in (gau, lin):
                assert np.all(r['scores'] <= s[r['anchor_idx']]) and np.all(r['scores'] > np.float32(THR))
                fresh = r['decays'] == 0
                assert np.array_equal(r['scores'][fresh], s[r['anchor_idx']][fresh])
            for g in ([None] if agnostic else range(C)):
                li = np.arange(len(lin['scores'])) if g is None else np.nonzero(lin['class_ids'] == g)[0]
                gi = np.arange(len(gau['scores'])) if g is None else np.nonzero(gau['class_ids'] == g)[0]
                assert (len(li) == 0) == (len(gi) == 0)
                if len(li):
                    assert lin['anchor_idx'][li[0]] == gau['anchor_idx'][gi[0]] and lin['decays'][li[0]] == 0 == gau['decays'][gi[0]]
    assert seen > 100
    u = np.linspace(0, 1, 1001).astype(np.float32)
    w = np.exp(ref.gauss_arg(u, 0.5).astype(np.float64))
    assert np.all(w <= 1.0) and np.all(w[u > 0.4] > 1.0 - u[u > 0.4].astype(np.float64))


def _rows(r, sel=None):
    sel = np.arange(len(r['scores'])) if sel is None else np.asarray(sel)
    return {k: np.array(r[k][sel]) for k in ('class_ids', 'scores', 'boxes', 'anchor_idx')}


def test_verify_replay_accepts_the_reference_and_rejects_what_is_wrong():
    checked = {'swap': 0, 'score': 0, 'drop': 0, 'class': 0}
    for case, c, s, bx, C, K in _cases():
        for mode in ref.MODES:
            for agnostic in (False, True):
                args = (c, s, bx, K, NMS, THR, C, mode, 0.5, agnostic)
                r = ref.soft_filter(*args)
                n = len(r['scores'])
                assert ref.verify_replay(_rows(r), *args) == n and n > 3, (case, mode, agnostic)
                # two swapped rows of one group whose scores differ by more than the tolerance
                pairs = [i for i in range(n - 1) if (agnostic or r['class_ids'][i] == r['class_ids'][i + 1])
                         and r['scores'][i] > r['scores'][i + 1] * (1 + 1e-3)]
                if pairs and mode != 'hard':                   # (in hard mode the second may be a box the first suppresses: also refused)
                    i = pairs[len(pairs) // 2]
                    sel = np.arange(n); sel[[i, i + 1]] = sel[[i + 1, i]]
                    with pytest.raises(AssertionError):
                        ref.verify_replay(_rows(r, sel), *args)
                    checked['swap'] += 1
                # a score off by 1e-4 relative
                bad = _rows(r)
                bad['scores'][n // 2] = np.float32(bad['scores'][n // 2] * np.float32(1 + 1e-4))
                with pytest.raises(AssertionError, match='score'):
                    ref.verify_replay(bad, *args)
                checked['score'] += 1
                # a dropped row
                for k in (0, n // 2, n - 1):
                    with pytest.raises(AssertionError):
                        ref.verify_replay(_rows(r, np.delete(np.arange(n), k)), *args)
                    checked['drop'] += 1
                # class-wise: a row of the wrong class -- the row of another group moved into this one, and a forged class id
                if not agnostic and C > 1:
                    other = [i for i in range(n) if r['class_ids'][i] != r['class_ids'][0]]
                    if other:
                        sel = np.concatenate([[other[0]], np.delete(np.arange(n), other[0])])
                        with pytest.raises(AssertionError):
                            ref.verify_replay(_rows(r, sel), *args)
                        forged = _rows(r)
                        forged['class_ids'][other[0]] = r['class_ids'][0]
                        with pytest.raises(AssertionError, match='class'):
                            ref.verify_replay(forged, *args)
                        checked['class'] += 1
    assert all(v > 5 for v in checked.values()), checked


def test_the_generator_gives_what_the_gpu_cases_rely_on():
    """decays in every image, soft-kept counts that differ from hard-kept, rows lost after decay -- in every mode x agnostic."""
    for case, c, s, bx, C, K in _cases():
        for agnostic in (False, True):
            hard = ref.soft_filter(c, s, bx, K, NMS, THR, C, 'hard', 0.5, agnostic)
            for mode in ('linear', 'gaussian'):
                soft = ref.soft_filter(c, s, bx, K, NMS, THR, C, mode, 0.5, agnostic)
                assert soft['total_decays'] >= 30 and soft['lost'] > 0, (case, mode, agnostic, soft['total_decays'], soft['lost'])
                assert len(soft['scores']) - len(hard['scores']) >= 3, (case, mode, agnostic)


def test_check_nms_and_make_cfg():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import config
    cfg = sqd.make_cfg(device='cpu')
    assert (cfg.nms_mode, cfg.nms_sigma, cfg.nms_agnostic) == ('hard', 0.5, False)
    assert config.check_nms(cfg, 't') == ('hard', 0.5, False)
    assert config.check_nms(types.SimpleNamespace(), 't') == ('hard', 0.5, False)        # the reference's own namespace
    cfg = sqd.make_cfg(device='cpu', nms_mode='gaussian', nms_sigma=0.25, nms_agnostic=True)
    assert config.check_nms(cfg, 't') == ('gaussian', 0.25, True)
    assert config.NMS_MODES == ('hard', 'linear', 'gaussian')
    for kw in ({'nms_mode': 'soft'}, {'nms_mode': None}, {'nms_mode': 1}, {'nms_sigma': 0.0}, {'nms_sigma': -1.0},
               {'nms_sigma': float('nan')}, {'nms_sigma': float('inf')}, {'nms_sigma': '0.5'}, {'nms_sigma': True},
               {'nms_agnostic': 1}, {'nms_agnostic': 'yes'}, {'nms_agnostic': None}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            sqd.make_cfg(device='cpu', **kw)


def test_ops_mode_names_and_refusals_without_a_gpu():
    from squeezedet_pytorch_amd import _native as nat, ops
    assert ops.NMS_MODES == ('hard', 'linear', 'gaussian')
    assert ops.nms_mode_index('t', 'gaussian', 0.25, True) == (2, 0.25, 1)
    for bad in (('soft', 0.5, False), ('hard', 0.0, False), ('linear', float('nan'), False), ('gaussian', -1.0, False),
                ('hard', 0.5, 1)):
        with pytest.raises(ValueError):
            ops.nms_mode_index('t', *bad)
    # detect_fn / filter_fn: the plain rule is what it always was, every other rule is the new path with the rule bound
    assert ops.detect_fn(3, 64, 16848) is ops.detect and ops.detect_fn(3, 64, 16848, 'hard', False) is ops.detect
    assert ops.detect_fn(3, 256, 16848) is ops.detect_wide and ops.detect_fn(20, 64, 16848) is ops.detect_many
    assert ops.filter_fn(3, 64, 16848) is ops.filter_dense and ops.filter_fn(80, 64, 100) is ops.filter_dense_many
    for C, K, A in ((3, 64, 16848), (3, 1024, 1 << 20), (80, 1, 1)):
        for mode, agn in (('linear', False), ('gaussian', True), ('hard', True)):
            f = ops.detect_fn(C, K, A, mode, agn, 0.7)
            assert f.func is ops.detect_nms and f.keywords == {'nms_mode': mode, 'nms_sigma': 0.7, 'nms_agnostic': agn}
            g = ops.filter_fn(C, K, A, mode, agn, 0.7)
            assert g.func is ops.filter_dense_nms and g.keywords == f.keywords
    with pytest.raises(ValueError):
        ops.detect_fn(3, 1025, 100, 'linear')
    with pytest.raises(ValueError):
        ops.detect_fn(3, 64, 100, 'nope')
    # the C ABI: status 1 / 2 are decided on the host, nothing is launched (there is no GPU here)
    lib = nat.lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    null = ctypes.c_void_p(0)

    def det(B=1, A=4, C=3, K=4, thr=0.3, ws=4, mode=0, sigma=0.5, agn=0, ready=0, pred=p, keys=p):
        return lib.sqd_detect_nms_fwd(pred, p, null, null, keys, p, p, p, p, p, B, A, C, 64, 64, K, 0.4, thr, ws, mode, sigma, agn, ready, null)

    def fil(B=1, A=4, C=3, K=4, thr=0.3, ws=4, mode=0, sigma=0.5, agn=0, ready=0, keys=p):
        return lib.sqd_filter_nms_fwd(p, p, p, keys, p, p, p, p, p, B, A, C, K, 0.4, thr, ws, mode, sigma, agn, ready, null)
    for f in (det, fil):
        assert f(mode=3) == nat.ERR_BAD_ARG and f(mode=-1) == nat.ERR_BAD_ARG
        for sg in (0.0, -1.0, float('nan'), float('inf')):
            assert f(mode=2, sigma=sg) == nat.ERR_BAD_ARG
        assert f(keys=null) == nat.ERR_BAD_ARG and f(ws=3) == nat.ERR_BAD_ARG and f(K=0) == nat.ERR_BAD_ARG
        assert f(thr=-0.1) == nat.ERR_BAD_ARG
        assert f(K=1025, ws=1 << 20) == nat.ERR_UNSUPPORTED and f(A=(1 << 20) + 1, ws=1 << 22) == nat.ERR_UNSUPPORTED
        assert f(C=257) == nat.ERR_UNSUPPORTED
    assert det(pred=null) == nat.ERR_BAD_ARG and det(C=17, ready=1) == nat.ERR_BAD_ARG and fil(ready=1) == nat.ERR_BAD_ARG


def test_the_lane_signature_follows_the_three_fields():
    """``DetectStream._params_signature`` without a GPU: what it touches of a stream is its cfg and the model's base."""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import lanes
    cfg = sqd.make_cfg(device='cpu')
    fake = types.SimpleNamespace(cfg=cfg, det=types.SimpleNamespace(model=types.SimpleNamespace(base=types.SimpleNamespace(fuse_detect_keys=True))))
    sig = lanes.DetectStream._params_signature
    base = sig(fake)
    seen = {base}
    for field, value in (('nms_mode', 'linear'), ('nms_mode', 'gaussian'), ('nms_sigma', 0.25), ('nms_agnostic', True)):
        setattr(cfg, field, value)
        s = sig(fake)
        assert s not in seen, (field, value)
        seen.add(s)
    cfg.nms_mode, cfg.nms_sigma, cfg.nms_agnostic = 'hard', 0.5, False
    assert sig(fake) == base
