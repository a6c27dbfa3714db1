"""Deterministic oracle sweep of the fused detection kernel (csrc/postproc.hip ``detect_kernel``) in its three launch forms:

  * dense filter (``ops.filter_dense``) on the oracle's own inputs;
  * pred mode, one workgroup per image (``ops.detect`` with a too-small workspace placeholder), against ``oracle.filter_detections``
    applied to ``ops.decode`` of the same ``pred`` -- decode_kernel shares ``anchor_score`` / ``anchor_box`` with detect_kernel, so
    this isolates selection and NMS from device-vs-host ``expf`` ULPs (decode-vs-oracle tolerances are tested elsewhere);
  * pred mode, split (eight scoring workgroups per image, key workspace), bitwise equal to the one-workgroup result.

Fixed seeds and a fixed case list: every run covers the same ground.  The generators aim at the kernel's branches: tie-heavy scores
(the K-th key tied across many of the 1024 threads' chunks: step 3b with chunk2 > 1), keys equal in their upper 16-24 bits (radix
passes 3 and 4 decide the K-th key), candidate counts M in {0, 1, K-1, K, K+1, all} (thresholds set to existing scores), duplicate /
nested / touching / zero-area boxes at NMS thresholds 0, 0.4 and 1, the boxes_postprocess scale division and the un-pad / un-crop
shift.  Every comparison is exact: counts, class ids and anchor indices equal, scores and boxes bit for bit, rows past the count
untouched.  A failing assertion names the case."""
import numpy as np
import pytest
import torch

import oracle
from squeezedet_pytorch_amd import ops

pytestmark = pytest.mark.gpu

A_LIST = (1, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049, 16848, 25596)
K_LIST = (1, 2, 63, 64)
C_LIST = (1, 2, 3, 8, 16)
NMS_LIST = (0.0, 0.4, 1.0)
M_TARGETS = ('0', '1', 'K-1', 'K', 'K+1', 'all')
SIZE = (384, 1248)                    # network input (H, W): decoded boxes are clamped to [0, W-1] x [0, H-1]
A_MAX = 25596                         # largest A whose LDS footprint 4 ceil4(A) + 2 A + 16 fits the kernel's 150 KB cap
SUBCASES = 60                         # (K, M target, NMS threshold, C) combinations per anchor count and score distribution
SPLIT_SUBCASES = 8                    # the same for the split launch (B = 20)


def _rotation(ai, d, i, n):
    """(K, M target, NMS threshold, C) of sub-case i: over the anchor counts every (K, M target) pair comes up."""
    j = (ai * n + i) * 7 + d
    return K_LIST[j % 4], M_TARGETS[(j // 4) % 6], NMS_LIST[j % 3], C_LIST[j % 5]


def _thresh(s0, target, K):
    """score_thresh that leaves ``target`` candidates (scores > threshold) in image 0 when its scores are distinct: an existing
    score (the (t+1)-th largest), or 0 for all of them (thresholds are >= 0)."""
    A = s0.size
    t = {'0': 0, '1': 1, 'K-1': K - 1, 'K': K, 'K+1': K + 1, 'all': A}[target]
    thr = float(np.sort(s0)[::-1][t]) if t < A else 0.0
    return thr if thr > 0 else 0.0


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _expect(case, got, b, exp, boxes=None):
    """Kernel result ``got`` (numpy count / class_ids / scores / boxes / anchor_idx of the batch) for image b == oracle dict ``exp``
    (``boxes``: the expected boxes if not exp's own), exactly; rows past the count stay as allocated (zero)."""
    cnt, cls, sc, bx, idx = got
    n = int(cnt[b])
    where = f'{case}, image {b}'
    if exp is None:
        assert n == 0, f'{where}: kernel kept {n} detections, the oracle none'
    else:
        assert n == len(exp['scores']), f'{where}: count {n} != oracle {len(exp["scores"])}'
        assert np.array_equal(idx[b, :n].astype(np.int64), exp['anchor_idx']), \
            f'{where}: anchor indices\n kernel {idx[b, :n].tolist()}\n oracle {exp["anchor_idx"].tolist()}'
        assert np.array_equal(cls[b, :n], exp['class_ids']), f'{where}: class ids'
        assert np.array_equal(_bits(sc[b, :n]), _bits(exp['scores'])), f'{where}: scores not bitwise equal'
        want = exp['boxes'] if boxes is None else boxes
        assert np.array_equal(_bits(bx[b, :n]), _bits(want)), f'{where}: boxes not bitwise equal'
    assert not cls[b, n:].any() and not _bits(sc[b, n:]).any() and not _bits(bx[b, n:]).any() and not idx[b, n:].any(), \
        f'{where}: rows past the count were written'


# ---- dense filter ------------------------------------------------------------------------------------------------------------------
_BOX_POOL = np.array([[0, 0, 10, 10], [0, 0, 10, 10],            # exact duplicates
                      [2, 2, 8, 8], [0, 0, 20, 20],              # nested
                      [10, 0, 20, 10], [0, 10, 10, 20],          # touching [0,0,10,10] (IoU 0)
                      [5, 5, 5, 5], [3, 3, 3, 9],                # zero area
                      [4, 0, 14, 10], [1, 1, 11, 11]], np.float32)


def _dense_boxes(rs, A):
    """Half the anchors from the pool above (in one of four clusters that do not overlap each other), half random boxes."""
    pool = _BOX_POOL[rs.randint(0, len(_BOX_POOL), A)] + (rs.randint(0, 4, A) * 100).astype(np.float32)[:, None]
    x1 = rs.uniform(0, 400, A).astype(np.float32)
    y1 = rs.uniform(0, 400, A).astype(np.float32)
    rnd = np.stack([x1, y1, x1 + rs.uniform(1, 60, A).astype(np.float32), y1 + rs.uniform(1, 60, A).astype(np.float32)], 1)
    return np.where((rs.rand(A) < 0.5)[:, None], pool, rnd).astype(np.float32)


def _dense_scores(rs, dist, A):
    if dist == 'distinct':
        return ((rs.permutation(A) + 1) / (A + 1)).astype(np.float32)
    if dist == 'grid':                  # a handful of values, negative and signed zeros included (never candidates)
        vals = np.array([-0.125, -0.0, 0.0, 0.125, 0.25, 0.375, 0.5], np.float32)
        return vals[rs.randint(0, len(vals), A)]
    if dist == 'ulp':                   # runs of np.nextafter neighbours of one value: keys equal in their upper 16-24 bits
        base = np.float32([0.3, 0.5, 0.875][rs.randint(0, 3)])
        return (base.view(np.uint32) + rs.randint(-300, 301, A)).astype(np.uint32).view(np.float32)
    assert dist == 'equal'
    return np.full(A, 0.5, np.float32)


@pytest.mark.parametrize('A', A_LIST)
def test_filter_dense_sweep_vs_oracle(A):
    ai = A_LIST.index(A)
    M_hit = set()
    for d, dist in enumerate(('distinct', 'grid', 'ulp', 'equal')):
        for i in range(SUBCASES):
            K, target, nms, C = _rotation(ai, d, i, SUBCASES)
            B = 3 if i % 2 else 1
            rs = np.random.RandomState(1000 * ai + 100 * d + i)
            s = np.stack([_dense_scores(rs, dist, A) for _ in range(B)])
            c = rs.randint(0, C, (B, A)).astype(np.int64)
            bx = np.stack([_dense_boxes(rs, A) for _ in range(B)])
            st = _thresh(s[0], target, K)
            case = dict(mode='dense', A=A, B=B, C=C, K=K, dist=dist, M_target=target, nms=nms, score_thresh=st)
            got = tuple(t.cpu().numpy() for t in ops.filter_dense(torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(),
                                                                  torch.from_numpy(bx).cuda(), C, K, nms, st))
            for b in range(B):
                exp = oracle.filter_detections(c[b], s[b], bx[b], K, nms, st, C)
                _expect(case, got, b, exp)
            M = int((s[0] > np.float32(st)).sum())
            if dist == 'distinct':
                M_hit.add(target)
                assert M == min({'0': 0, '1': 1, 'K-1': K - 1, 'K': K, 'K+1': K + 1, 'all': A}[target], A), case
            if M > K:
                M_hit.add('radix')
    assert 'radix' in M_hit or A <= 64


# ---- pred mode -------------------------------------------------------------------------------------------------------------------
# anchors (cx, cy, w, h): with zero deltas a box spans [c - (w-1)/2, c + (w-1)/2] -- duplicates, nested, touching, zero-area, clamped
_ANCHOR_POOL = np.array([[100, 100, 11, 11], [110, 100, 11, 11], [100, 110, 11, 11],   # touching neighbours
                         [100, 100, 21, 21], [100, 100, 5, 11],                           # nested
                         [100, 100, 1, 11], [100, 100, 1, 1],                             # zero width / a point
                         [300, 200, 41, 41], [310, 200, 41, 41], [330, 200, 41, 41],      # IoU 0.6 / 0.14 with the first
                         [0, 0, 11, 11], [SIZE[1] - 1, SIZE[0] - 1, 11, 11]], np.float32)  # clamped at the image border


def _pred_case(rs, dist, B, A, C):
    """pred [B, A, C+5] and anchors [A, 4] (fp32 numpy) of one score distribution."""
    anchors = np.where((rs.rand(A) < 0.5)[:, None], _ANCHOR_POOL[rs.randint(0, len(_ANCHOR_POOL), A)],
                       np.stack([rs.uniform(0, SIZE[1], A), rs.uniform(0, SIZE[0], A), rs.uniform(1, 120, A), rs.uniform(1, 120, A)], 1))
    pred = np.empty((B, A, C + 5), np.float32)
    if dist == 'normal':
        pred[..., :C + 1] = rs.standard_normal((B, A, C + 1)) * 1.5
        pred[..., C + 1:] = rs.standard_normal((B, A, 4)) * 0.3
        return pred, anchors.astype(np.float32)
    # deltas on a coarse grid, mostly zero: boxes repeat the pool's exactly
    pred[..., C + 1:] = np.where(rs.rand(B, A, 4) < 0.7, 0.0, rs.randint(-2, 3, (B, A, 4)) * 0.25)
    if dist == 'grid':                  # class and confidence logits on a coarse grid: thousands of anchors share a few scores
        pred[..., :C + 1] = rs.randint(-2, 3, (B, A, C + 1))
    else:
        assert dist == 'sat'            # saturated confidence (logit >= 20: conf == 1.0f) and equal class logits: score == 1/C
        sat = rs.rand(B, A) < 0.6
        pred[..., :C] = np.where(sat[..., None], rs.randint(-2, 3, (B, A, 1)), rs.standard_normal((B, A, C)) * 1.5)
        pred[..., C] = np.where(sat, 20 + rs.randint(0, 5, (B, A)), rs.standard_normal((B, A)) - 1.0)
    return pred, anchors.astype(np.float32)


def _post(rs, kind, B):
    """None, scales [B,2] = (sy, sx), or shifts [B,2] = (dy, dx) with the (padding, crops) they stand for (one of the two zero per
    axis, as the forbid_resize pre-processing makes them)."""
    if kind == 'scales':
        return rs.uniform(0.5, 2.0, (B, 2)).astype(np.float32), None
    if kind == 'shifts':
        pads, crops = np.zeros((B, 4), np.int16), np.zeros((B, 4), np.int16)
        for b in range(B):
            for k in (0, 2):
                (pads if rs.rand() < 0.5 else crops)[b, k] = rs.randint(0, 40)
        sh = np.stack([crops[:, 0].astype(np.float32) - pads[:, 0], crops[:, 2].astype(np.float32) - pads[:, 2]], 1)
        return sh.astype(np.float32), (pads, crops)
    return None, None


def _pred_run(case, rs, dist, B, A, C, K, nms, target, post):
    """One pred-mode case: the one-workgroup launch against the oracle; with B == 20 the split launch as well, bitwise."""
    pred_np, anc_np = _pred_case(rs, dist, B, A, C)
    pred, anchors = torch.from_numpy(pred_np).cuda(), torch.from_numpy(anc_np).cuda()
    ids, scores, boxes = (t.cpu().numpy() for t in ops.decode(pred, anchors, SIZE, C))
    st = _thresh(scores[0], target, K)
    case.update(score_thresh=st, post=post)
    aux, padcrop = _post(rs, post, B)
    kw = {} if aux is None else {post: torch.from_numpy(aux).cuda()}
    one = ops._det_buffers(B, K, pred.device) + (torch.zeros(4, device=pred.device, dtype=torch.int32),)    # placeholder: one WG / image
    got = tuple(t.cpu().numpy() for t in ops.detect(pred, anchors, SIZE, C, K, nms, st, out=one, **kw))
    for b in range(B):
        exp = oracle.filter_detections(ids[b], scores[b], boxes[b], K, nms, st, C)
        want = None
        if exp is not None and post == 'scales':
            want = oracle.boxes_postprocess(exp['boxes'], aux[b])
        elif exp is not None and post == 'shifts':
            want = oracle.boxes_unpad_uncrop(exp['boxes'], padcrop[0][b], padcrop[1][b])
        _expect(case, got, b, exp, want)
    if B == 20:
        split = ops._det_buffers(B, K, pred.device, A)
        assert split[5].numel() == ops.det_workspace_words(B, A)
        for it in range(2):                                   # launch after launch: the arrival counters return to zero
            for t in split[:5]:
                t.zero_()
            res = ops.detect(pred, anchors, SIZE, C, K, nms, st, out=split, **kw)
            torch.cuda.synchronize()
            assert int(split[5][-B:].abs().sum()) == 0, f'{case}, launch {it}: arrival counters not back at zero'
            for name, g, r in zip(('count', 'class_ids', 'scores', 'boxes', 'anchor_idx'), res, one[:5]):
                assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                                   r.view(torch.int32) if r.dtype == torch.float32 else r), \
                    f'{case}, launch {it}: split {name} differs from one workgroup per image'
    return scores


@pytest.mark.parametrize('A', A_LIST)
def test_detect_pred_sweep_vs_oracle(A):
    ai = A_LIST.index(A)
    for d, dist in enumerate(('normal', 'grid', 'sat')):
        for i in range(SUBCASES):
            K, target, nms, C = _rotation(ai, d, i, SUBCASES)
            B = 3 if i % 2 else 1
            post = ('none', 'scales', 'shifts')[(i + d) % 3]
            rs = np.random.RandomState(50000 + 1000 * ai + 100 * d + i)
            case = dict(mode='pred', A=A, B=B, C=C, K=K, dist=dist, M_target=target, nms=nms)
            scores = _pred_run(case, rs, dist, B, A, C, K, nms, target, post)
            if dist == 'normal' and np.unique(scores[0]).size == A:
                M = int((scores[0] > np.float32(case['score_thresh'])).sum())
                assert M == min({'0': 0, '1': 1, 'K-1': K - 1, 'K': K, 'K+1': K + 1, 'all': A}[target], A), case


@pytest.mark.parametrize('A', A_LIST)
def test_detect_split_sweep_vs_oracle(A):
    ai = A_LIST.index(A)
    for d, dist in enumerate(('normal', 'grid', 'sat')):
        for i in range(SPLIT_SUBCASES):
            K, target, nms, C = _rotation(ai, d, i, SPLIT_SUBCASES)
            post = ('none', 'scales', 'shifts')[(ai + d + i) % 3]
            rs = np.random.RandomState(90000 + 100 * ai + 10 * d + i)
            case = dict(mode='split', A=A, B=20, C=C, K=K, dist=dist, M_target=target, nms=nms)
            _pred_run(case, rs, dist, 20, A, C, K, nms, target, post)


def test_detect_tie_across_thread_chunks():
    """All-tied candidates at the K-th key, thousands of them: the tie pick (ascending anchor index) spans many threads' chunks."""
    for A, C, K in ((16848, 3, 64), (25596, 1, 63), (2049, 16, 2)):
        rs = np.random.RandomState(A + K)
        pred_np, anc_np = _pred_case(rs, 'sat', 2, A, C)
        pred_np[..., C] = 25.0
        pred_np[..., :C] = 0.0                                          # every anchor scores exactly 1/C
        pred_np[1, ::7, C] = -1.0                                       # image 1: every 7th anchor drops out
        pred, anchors = torch.from_numpy(pred_np).cuda(), torch.from_numpy(anc_np).cuda()
        ids, scores, boxes = (t.cpu().numpy() for t in ops.decode(pred, anchors, SIZE, C))
        assert (scores[0] == np.float32(1.0) / np.float32(C)).all()
        for nms in NMS_LIST:
            one = ops._det_buffers(2, K, pred.device) + (torch.zeros(4, device=pred.device, dtype=torch.int32),)
            got = tuple(t.cpu().numpy() for t in ops.detect(pred, anchors, SIZE, C, K, nms, 0.0, out=one))
            for b in range(2):
                exp = oracle.filter_detections(ids[b], scores[b], boxes[b], K, nms, 0.0, C)
                _expect(dict(mode='ties', A=A, C=C, K=K, nms=nms), got, b, exp)


# ---- limits and refusals ---------------------------------------------------------------------------------------------------------
def test_detect_anchor_limit():
    """A = 25596 runs (the sweeps above); one more anchor exceeds the LDS cap and is refused (status 2), in every launch form."""
    for A in (A_MAX + 1, A_MAX + 4):
        pred = torch.zeros(1, A, 8, device='cuda')
        anchors = torch.ones(A, 4, device='cuda')
        with pytest.raises(RuntimeError, match='status 2'):
            ops.detect(pred, anchors, SIZE, 3)
        with pytest.raises(RuntimeError, match='status 2'):
            ops.detect(pred, anchors, SIZE, 3, out=ops._det_buffers(1, 64, pred.device) + (torch.zeros(4, device='cuda', dtype=torch.int32),))
        with pytest.raises(RuntimeError, match='status 2'):
            ops.filter_dense(torch.zeros(1, A, dtype=torch.int64, device='cuda'), torch.zeros(1, A, device='cuda'),
                             torch.zeros(1, A, 4, device='cuda'), 3)


def test_detect_rejects_result_buffers_it_cannot_fill():
    """``out`` must be exactly the (B,) / (B,K) / (B,K) / (B,K,4) / (B,K) int32 / int64 / fp32 / fp32 / int32 tensors the kernel
    writes: anything else is a ValueError before any launch, the buffers untouched."""
    B, A, C, K = 2, 300, 3, 64
    rs = np.random.RandomState(7)
    pred = torch.from_numpy((rs.standard_normal((B, A, C + 5)) * 1.5).astype(np.float32)).cuda()
    anchors = torch.from_numpy(np.abs(rs.standard_normal((A, 4)) * 50 + 100).astype(np.float32)).cuda()
    dev = pred.device

    def filled(bufs):
        for t in bufs:
            t.fill_(7)
        return bufs

    def misaligned_boxes():
        bufs = list(ops._det_buffers(B, K, dev))
        bufs[3] = torch.zeros(B * K * 4 + 1, device=dev)[1:].view(B, K, 4)
        return bufs

    def strided_scores():
        bufs = list(ops._det_buffers(B, K, dev))
        bufs[2] = torch.zeros(K, B, device=dev).t()
        return bufs

    def wrong_dtype():
        bufs = list(ops._det_buffers(B, K, dev))
        bufs[1] = torch.zeros(B, K, device=dev, dtype=torch.int32)
        return bufs

    def on_host():
        bufs = list(ops._det_buffers(B, K, dev))
        bufs[4] = torch.zeros(B, K, dtype=torch.int32)
        return bufs

    bad = [('K 8 buffers, keep_top_k 64', lambda: list(ops.det_buffers_packed(B, 8, dev, A)[0])),
           ('K 32 buffers', lambda: list(ops._det_buffers(B, 32, dev))),
           ('B + 1 rows', lambda: list(ops._det_buffers(B + 1, K, dev))),
           ('misaligned boxes', misaligned_boxes), ('non-contiguous scores', strided_scores), ('int32 class ids', wrong_dtype),
           ('anchor indices on the host', on_host), ('four tensors', lambda: list(ops._det_buffers(B, K, dev))[:4])]
    for what, make in bad:
        bufs = filled(make())
        before = [t.clone() for t in bufs]
        with pytest.raises(ValueError):
            ops.detect(pred, anchors, SIZE, C, K, 0.4, 0.3, out=bufs)
        torch.cuda.synchronize()
        assert all(torch.equal(t, u) for t, u in zip(bufs, before)), f'{what}: buffers changed'
    # the right buffers (packed, with or without the workspace) are accepted and give the fresh-allocation result
    ref = ops.detect(pred, anchors, SIZE, C, K, 0.4, 0.3)
    for bufs in (ops.det_buffers_packed(B, K, dev, A)[0], ops.det_buffers_packed(B, K, dev)[0]):
        got = ops.detect(pred, anchors, SIZE, C, K, 0.4, 0.3, out=bufs)
        assert int(ref[0].sum()) > 0 and all(torch.equal(g, r) for g, r in zip(got, ref))


def test_negative_score_thresh_is_refused():
    """The candidate key is the score's bits if score > score_thresh, else 0: exact for thresholds >= 0 only (a negative one would
    drop scores of exactly 0, and the dense filter would rank negative scores first).  Such thresholds (and NaN) are refused; 0 runs."""
    A = 100
    pred = torch.zeros(1, A, 8, device='cuda')
    pred[0, :, 3] = -200.0                                     # conf == 0: every score is exactly 0
    anchors = torch.ones(A, 4, device='cuda')
    ids = torch.zeros(1, A, dtype=torch.int64, device='cuda')
    sc = torch.zeros(1, A, device='cuda')
    sc[0, ::2] = -0.5
    bx = torch.zeros(1, A, 4, device='cuda')
    for st in (-0.1, -1e-30, float('-inf'), float('nan')):
        with pytest.raises(ValueError, match='score_thresh'):
            ops.detect(pred, anchors, SIZE, 3, 64, 0.4, st)
        with pytest.raises(ValueError, match='score_thresh'):
            ops.filter_dense(ids, sc, bx, 3, 64, 0.4, st)
    for st in (0.0, -0.0):
        assert int(ops.detect(pred, anchors, SIZE, 3, 64, 0.4, st)[0][0]) == 0
        assert int(ops.filter_dense(ids, sc, bx, 3, 64, 0.4, st)[0][0]) == 0
        assert oracle.filter_detections(ids[0].cpu().numpy(), sc[0].cpu().numpy(), bx[0].cpu().numpy(), 64, 0.4, st) is None
