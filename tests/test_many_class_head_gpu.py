"""GPU tier: the many-class head (csrc/many_class.h: a 16-lane group per anchor row, 1 <= C <= 256) -- ``ops.decode_many`` /
``resolve_many`` / ``detect_many`` / ``filter_dense_many`` / ``loss_*_many`` -- against the oracle.

Decode and resolve are held to the oracle evaluated in float64 with a bound computed here: max(4 e32, 2^-22), e32 = the float32
oracle's own maximum error against float64 on the same case (the lane tree sums in another order than torch and the device expf and
division are each within a few ulp of values <= 1: a factor of two for the independent roundings, a second one of slack).  The
fused detect and the dense filter equal ``oracle.filter_detections`` on the device's own dense decode exactly.  The loss is held to
``fp64_ref.loss`` exactly as tests/test_fp64_loss_gpu.py holds C <= 16 (its case builders and bars are imported)."""
import numpy as np
import pytest
import torch

import oracle
import test_detect_sweep_gpu as sweep
import test_fp64_loss_gpu as L
from squeezedet_pytorch_amd import ops
from squeezedet_pytorch_amd.boxes import KITTI_ANCHORS_SEED

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22


def _anchors(size):
    return oracle.generate_anchors((size[0] // 16, size[1] // 16), size, np.asarray(KITTI_ANCHORS_SEED))


def _pred(B, A, C, seed=None):
    """N(0,1) * [2] * (C+1) + [0.4] * 4, and +6 on one random class logit per anchor (without it almost no score passes 0.3 at 80
    classes)."""
    rs = np.random.RandomState(C if seed is None else seed)
    p = rs.standard_normal((B, A, C + 5)).astype(np.float32) * np.array([2.0] * (C + 1) + [0.4] * 4, np.float32)
    boost = rs.randint(0, C, (B, A))
    np.put_along_axis(p[..., :C], boost[..., None], np.take_along_axis(p[..., :C], boost[..., None], 2) + np.float32(6.0), 2)
    return torch.from_numpy(p)


_CASES = {}


def _case(C, B, size):
    """pred, anchors and the float64 / float32 oracle outputs of one case, computed once."""
    key = (C, B, size)
    if key not in _CASES:
        anc = _anchors(size)
        pred = _pred(B, anc.shape[0], C)
        p64 = pred.double()
        r64 = oracle.resolve_predictions(p64, anc, size, C, log_softmax=True)
        r32 = oracle.resolve_predictions(pred, anc, size, C, log_softmax=True)
        h64 = oracle.inference_head(p64, anc, size, C)
        h32 = oracle.inference_head(pred, anc, size, C)
        _CASES[key] = dict(pred=pred, anc=anc, r64=r64, r32=r32, h64=h64, h32=h32)
    return _CASES[key]


def _bound(ref32, ref64):
    e32 = float((ref32.double() - ref64).abs().max())
    return e32, max(4.0 * e32, FLOOR)


def _check_ids(tag, ids, r64, C, bound):
    """Class ids equal the float64 arg-max wherever the float64 top two of p_c * conf differ by more than twice the score bound."""
    probs, _, conf, _, _ = r64
    v = probs * conf
    top2 = torch.topk(v, 2, dim=2)[0] if C > 1 else torch.cat([v, v - 1.0], 2)
    clear = (top2[..., 0] - top2[..., 1]) > 2.0 * bound
    want = torch.argmax(v, dim=2)
    left_out = 1.0 - float(clear.double().mean())
    print(f'{tag}: anchors left out as ambiguous {left_out:.4%}')
    assert left_out <= 0.005, (tag, left_out)
    assert torch.equal(ids[clear], want[clear]), tag


@pytest.mark.parametrize('B,size', [(2, (64, 96)), (1, (16, 16))])
@pytest.mark.parametrize('C', [17, 20, 80, 255, 256])
def test_decode_resolve_vs_float64_oracle(C, B, size):
    cs = _case(C, B, size)
    pred, anc = cs['pred'].cuda(), torch.from_numpy(cs['anc']).float().cuda()
    tag = f'many head C{C} B{B} {size[0]}x{size[1]}'
    ids, sc, bx = ops.decode_many(pred, anc, size, C)
    probs, logp, conf, deltas, boxes = ops.resolve_many(pred, anc, size, C, log_softmax=True)
    assert ops.resolve_many(pred, anc, size, C)[1] is None
    torch.cuda.synchronize()
    ids64, sc64, bx64 = cs['h64']
    for name, got, r32, r64 in (('score', sc, cs['h32'][1], sc64), ('probs', probs, cs['r32'][0], cs['r64'][0]),
                                ('logp', logp, cs['r32'][1], cs['r64'][1]), ('conf', conf, cs['r32'][2], cs['r64'][2])):
        e32, bound = _bound(r32, r64)
        err = float((got.cpu().double() - r64).abs().max())
        print(f'{tag} {name:6s}: e32 {e32:.3e}  bound {bound:.3e}  kernel err {err:.3e}')
        assert err <= bound, (tag, name, err, bound)
    _, sbound = _bound(cs['h32'][1], sc64)
    np.testing.assert_allclose(bx.cpu().numpy(), cs['h32'][2].numpy(), atol=1e-3)
    np.testing.assert_allclose(boxes.cpu().numpy(), cs['r32'][4].numpy(), atol=1e-3)
    np.testing.assert_allclose(deltas.cpu().numpy(), cs['r32'][3].numpy(), atol=1e-3)
    assert torch.equal(bx, boxes)
    _check_ids(tag, ids.cpu(), cs['r64'], C, sbound)


@pytest.mark.parametrize('C,pairs', [(17, [(0, 16), (15, 16)]), (40, [(0, 39), (15, 16), (16, 32), (3, 19, 35)]),
                                     (256, [(0, 255), (15, 16), (16, 32), (254, 255), (15, 16, 255)])])
def test_exact_ties_lowest_index_wins(C, pairs):
    """Two or three equal maximal class logits at positions that straddle the lane group's seams: equal logits give equal products,
    and the lowest index must win -- in the dense decode and in the fused detect's re-decode."""
    size = (64, 96)
    anc = _anchors(size)
    A = anc.shape[0]
    pred = _pred(1, A, C, seed=900 + C)
    pred[..., :C] = pred[..., :C].clamp(max=3.0)
    want = np.full(A, -1)
    for a in range(A):
        t = pairs[a % len(pairs)]
        pred[0, a, list(t)] = 5.0 + 0.125 * (a % 7)
        pred[0, a, C] = 4.0                                       # every anchor above the threshold
        want[a] = min(t)
    ancd = torch.from_numpy(anc).float().cuda()
    ids, sc, bx = ops.decode_many(pred.cuda(), ancd, size, C)
    assert np.array_equal(ids.cpu().numpy()[0], want)
    cnt, cls, s2, b2, idx = (t.cpu().numpy() for t in ops.detect_many(pred.cuda(), ancd, size, C, 1024, 0.4, 0.0))
    n = int(cnt[0])
    assert n > 0 and np.array_equal(cls[0, :n], want[idx[0, :n]])


def test_sixteen_classes_against_the_narrow_kernels():
    """C = 16 through the many-class functions against ops.decode on the same input: same bound, identical class ids outside the
    ambiguous set (bitwise equality is not required: the summation order differs)."""
    C, size = 16, (64, 96)
    cs = _case(C, 2, size)
    pred, anc = cs['pred'].cuda(), torch.from_numpy(cs['anc']).float().cuda()
    ids, sc, bx = ops.decode_many(pred, anc, size, C)
    idn, scn, bxn = ops.decode(pred, anc, size, C)
    e32, bound = _bound(cs['h32'][1], cs['h64'][1])
    err = float((sc.cpu().double() - cs['h64'][1]).abs().max())
    print(f'many head C16 vs narrow: e32 {e32:.3e} bound {bound:.3e} kernel err {err:.3e} '
          f'many-narrow {float((sc - scn).abs().max()):.3e}')
    assert err <= bound and float((sc - scn).abs().max()) <= 2 * bound
    assert torch.equal(bx, bxn)
    v = cs['r64'][0] * cs['r64'][2]
    top2 = torch.topk(v, 2, dim=2)[0]
    clear = (top2[..., 0] - top2[..., 1]) > 2.0 * bound
    assert float(clear.double().mean()) >= 0.995
    assert torch.equal(ids.cpu()[clear], idn.cpu()[clear])
    _check_ids('many head C16', ids.cpu(), cs['r64'], C, bound)


@pytest.mark.parametrize('size', [(64, 96), (128, 256)])
@pytest.mark.parametrize('C', [17, 80, 256])
def test_detect_and_filter_equal_oracle_on_own_decode(C, size):
    """K in {1, 64, 65, 1024} (A < K among them), scales / shifts present, image 1 all below the threshold: the fused detect and the
    dense filter are exactly oracle.filter_detections of ops.decode_many."""
    anc = _anchors(size)
    A, B = anc.shape[0], 2
    pred = _pred(B, A, C, seed=1000 + C)
    pred[1, :, C] = -20.0                                         # image 1: nothing above the threshold
    predd, ancd = pred.cuda(), torch.from_numpy(anc).float().cuda()
    idsd, scd, bxd = ops.decode_many(predd, ancd, size, C)
    ids, scores, boxes = (t.cpu().numpy() for t in (idsd, scd, bxd))
    rs = np.random.RandomState(C)
    distinct = set()
    for K in (1, 64, 65, 1024):
        for post in ('none', 'scales', 'shifts'):
            aux, padcrop = sweep._post(rs, post, B)
            kw = {} if aux is None else {post: torch.from_numpy(aux).cuda()}
            case = dict(mode='many pred', A=A, C=C, K=K, post=post)
            got = tuple(t.cpu().numpy() for t in ops.detect_many(predd, ancd, size, C, K, 0.4, 0.3, **kw))
            for b in range(B):
                exp = oracle.filter_detections(ids[b], scores[b], boxes[b], K, 0.4, 0.3, C)
                want = None
                if exp is not None and post == 'scales':
                    want = oracle.boxes_postprocess(exp['boxes'], aux[b])
                elif exp is not None and post == 'shifts':
                    want = oracle.boxes_unpad_uncrop(exp['boxes'], padcrop[0][b], padcrop[1][b])
                sweep._expect(case, got, b, exp, want)
                if exp is not None and K == 1024:
                    distinct.add(len(set(exp['class_ids'].tolist())))
            assert int(got[0][1]) == 0
        case = dict(mode='many dense', A=A, C=C, K=K)
        got = tuple(t.cpu().numpy() for t in ops.filter_dense_many(idsd, scd, bxd, C, K, 0.4, 0.3))
        for b in range(B):
            sweep._expect(case, got, b, oracle.filter_detections(ids[b], scores[b], boxes[b], K, 0.4, 0.3, C))
    if C == 256 and A > 1024:
        assert max(distinct) > 64, f'no image kept more than 64 distinct classes at K = 1024 ({distinct})'


def test_detect_many_rejects_wrong_out_buffers():
    C, size = 20, (64, 96)
    anc = _anchors(size)
    pred, ancd = _pred(2, anc.shape[0], C).cuda(), torch.from_numpy(anc).float().cuda()
    good = ops._det_buffers(2, 100, pred.device, anc.shape[0], C)
    assert good[5].numel() >= ops.det_workspace_words_wide(2, anc.shape[0], 100)
    a = ops.detect_many(pred, ancd, size, C, 100, 0.4, 0.3, out=good)
    b = ops.detect_many(pred, ancd, size, C, 100, 0.4, 0.3)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[0].sum()) > 0
    with pytest.raises(ValueError, match='out'):
        ops.detect_many(pred, ancd, size, C, 100, 0.4, 0.3, out=ops._det_buffers(2, 64, pred.device))
    with pytest.raises(ValueError, match='out'):
        ops.detect_many(pred, ancd, size, C, 100, 0.4, 0.3, out=ops._det_buffers(3, 100, pred.device))
    with pytest.raises(ValueError, match='256'):
        ops.detect_many(torch.zeros(1, 4, 262, device='cuda'), ancd[:4], size, 257)


def _run_loss_many(pred, gt, anchors, C, monkeypatch):
    """test_fp64_loss_gpu.run_loss with the many-class launches in place of the <= 16-class ones."""
    for name in ('loss_fwd', 'loss_mean_fwd', 'loss_mean_bwd', 'loss_bwd'):
        monkeypatch.setattr(ops, name, getattr(ops, name + '_many'))
    return L.run_loss(pred, gt, anchors, C)


@pytest.mark.parametrize('C', [17, 80, 256])
def test_loss_edges_and_saturation(C, monkeypatch):
    pred, gt, anchors = L.edge_case(C=C)
    res = _run_loss_many(pred, gt, anchors, C, monkeypatch)
    L._report(f'many edges C{C}', res)
    assert res['flips'] == 0
    pred, gt, anchors = L.saturated_case(C=C)
    L._report(f'many saturated C{C}', _run_loss_many(pred, gt, anchors, C, monkeypatch))


@pytest.mark.parametrize('A', [1, 63, 257])
@pytest.mark.parametrize('C', [17, 80, 256])
def test_loss_anchor_counts_and_rerun(C, A, monkeypatch):
    pred, gt, anchors = L.random_case(2, A, C, seed=100 + A + C)
    L._report(f'many A{A} B2 C{C}', _run_loss_many(pred, gt, anchors, C, monkeypatch))
    # a second launch on the same operands: bitwise-equal outputs
    p, g, a = pred.cuda(), gt.cuda(), anchors.cuda()
    outs = []
    for _ in range(2):
        losses, nobj, mean4 = ops.loss_mean_fwd_many(p, g, a, L.SIZE, C, L.WEIGHTS)
        dc = ops.loss_bwd_many(p, g, a, nobj, L.make_coef(2, 3).cuda(), L.SIZE, C, L.WEIGHTS)
        outs.append((losses, nobj, mean4, dc))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
