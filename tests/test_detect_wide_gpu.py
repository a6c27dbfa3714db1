"""The wide fused detect (csrc/detect_wide.hip ``detect_wide_score_kernel`` + ``detect_wide_select_kernel``: 1 <= K <= 1024, up to 2^20
anchors) against ``oracle.filter_detections``, and every layer above it: ``ops.detect_wide`` / ``ops.filter_dense_wide``, the
``Detector`` entry points that choose the path with ``ops.detect_path``, and the lane executor.

The sweeps use the score and box generators of tests/test_detect_sweep_gpu.py (distinct / grid / ulp / equal scores, normal / grid /
sat logits) on a fixed case list.  Every comparison is exact: counts, class ids and anchor indices equal, scores and boxes bit for
bit, rows past the count untouched.  Each sweep also asserts that it reached the ground the wide path exists for: more than 64 kept
detections at every K >= 128, candidate counts on both sides of K at every K, thousands of ties at the 1024th key.

Pred mode compares with the oracle applied to ``ops.decode`` of the same ``pred`` (decode_kernel shares ``anchor_score`` /
``anchor_box`` with both detect paths), which isolates selection and NMS from device-vs-host ``expf`` ULPs.

The 720p cases assume that every convolution launch takes an 80 x 45 grid; should one refuse it by a limit of its own, that is a
finding for the convolution code, not something to work around here."""
import numpy as np
import pytest
import torch

import oracle
import test_detect_sweep_gpu as sweep
from squeezedet_pytorch_amd import ops

pytestmark = pytest.mark.gpu

A_LIST = (1, 64, 65, 1025, 16848, 25596, 25597, 32400, 65535, 65536, 73440)     # 65535 | 65536: the narrow kernel's uint16 indices end
K_LIST = (1, 64, 65, 127, 128, 256, 1000, 1024)
C_LIST = (1, 2, 3, 8, 16)
NMS_LIST = sweep.NMS_LIST
M_TARGETS = sweep.M_TARGETS
SIZE = sweep.SIZE
SUBCASES = 6                          # (K, M target, NMS threshold, C) combinations per anchor count and score distribution


def _rotation(ai, d, i):
    """(K, M target, NMS threshold, C) of sub-case i of anchor count ai and distribution d.  n counts the cases of one distribution;
    K walks with n, the M target with n // 8 (so each K meets each target), the NMS threshold and C on strides of their own."""
    n = ai * SUBCASES + i
    return K_LIST[(n + 3 * d) % 8], M_TARGETS[(n // 8 + n + d) % 6], NMS_LIST[(n // 2 + d) % 3], C_LIST[(n + 2 * d) % 5]


def _batch(K, i):
    """Images per launch: several where the host oracle is cheap, so that the image index reaches every per-image offset."""
    if K >= 1000:
        return 2 if i % 3 == 0 else 1
    return 3 if i % 2 else 1


class _Coverage:
    """What a sweep has to reach (asserted at its end, so that it cannot pass emptily)."""

    def __init__(self):
        self.above, self.below, self.kept = set(), set(), {}

    def see(self, K, M, kept):
        (self.above if M > K else self.below).add(K)
        self.kept[K] = max(self.kept.get(K, 0), kept)

    def check(self, kept_over_64=True):
        for K in K_LIST:
            assert K in self.above, f'no case with more than K = {K} candidates'
            assert K in self.below, f'no case with at most K = {K} candidates'
            if kept_over_64 and K >= 128:
                assert self.kept[K] > 64, f'K = {K}: no image kept more than 64 detections (most: {self.kept[K]})'


def test_filter_dense_wide_sweep_vs_oracle():
    cov = _Coverage()
    for ai, A in enumerate(A_LIST):
        for d, dist in enumerate(('distinct', 'grid', 'ulp', 'equal')):
            for i in range(SUBCASES):
                K, target, nms, C = _rotation(ai, d, i)
                B = _batch(K, i)
                rs = np.random.RandomState(200000 + 1000 * ai + 100 * d + i)
                s = np.stack([sweep._dense_scores(rs, dist, A) for _ in range(B)])
                c = rs.randint(0, C, (B, A)).astype(np.int64)
                bx = np.stack([sweep._dense_boxes(rs, A) for _ in range(B)])
                st = sweep._thresh(s[0], target, K)
                case = dict(mode='dense wide', A=A, B=B, C=C, K=K, dist=dist, M_target=target, nms=nms, score_thresh=st)
                got = tuple(t.cpu().numpy() for t in ops.filter_dense_wide(torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(),
                                                                           torch.from_numpy(bx).cuda(), C, K, nms, st))
                for b in range(B):
                    exp = oracle.filter_detections(c[b], s[b], bx[b], K, nms, st, C)
                    sweep._expect(case, got, b, exp)
                    cov.see(K, int((s[b] > np.float32(st)).sum()), int(got[0][b]))
                if dist == 'distinct':
                    M = int((s[0] > np.float32(st)).sum())
                    assert M == min({'0': 0, '1': 1, 'K-1': K - 1, 'K': K, 'K+1': K + 1, 'all': A}[target], A), case
    cov.check()


def _wide_pred_run(case, rs, dist, B, A, C, K, nms, target, post):
    """One pred-mode case of ``ops.detect_wide`` against the oracle on ``ops.decode`` of the same pred.  -> (scores, threshold, counts)"""
    pred_np, anc_np = sweep._pred_case(rs, dist, B, A, C)
    pred, anchors = torch.from_numpy(pred_np).cuda(), torch.from_numpy(anc_np).cuda()
    ids, scores, boxes = (t.cpu().numpy() for t in ops.decode(pred, anchors, SIZE, C))
    st = sweep._thresh(scores[0], target, K)
    case.update(score_thresh=st, post=post)
    aux, padcrop = sweep._post(rs, post, B)
    kw = {} if aux is None else {post: torch.from_numpy(aux).cuda()}
    got = tuple(t.cpu().numpy() for t in ops.detect_wide(pred, anchors, SIZE, C, K, nms, st, **kw))
    for b in range(B):
        exp = oracle.filter_detections(ids[b], scores[b], boxes[b], K, nms, st, C)
        want = None
        if exp is not None and post == 'scales':
            want = oracle.boxes_postprocess(exp['boxes'], aux[b])
        elif exp is not None and post == 'shifts':
            want = oracle.boxes_unpad_uncrop(exp['boxes'], padcrop[0][b], padcrop[1][b])
        sweep._expect(case, got, b, exp, want)
    return scores, st, got[0]


def test_detect_wide_pred_sweep_vs_oracle():
    cov = _Coverage()
    posts = set()
    for ai, A in enumerate(A_LIST):
        for d, dist in enumerate(('normal', 'grid', 'sat')):
            for i in range(SUBCASES):
                K, target, nms, C = _rotation(ai, d, i)
                B = _batch(K, i)
                post = ('none', 'scales', 'shifts')[(ai + i + d) % 3]
                rs = np.random.RandomState(300000 + 1000 * ai + 100 * d + i)
                case = dict(mode='pred wide', A=A, B=B, C=C, K=K, dist=dist, M_target=target, nms=nms)
                scores, st, cnt = _wide_pred_run(case, rs, dist, B, A, C, K, nms, target, post)
                posts.add(post)
                for b in range(B):
                    cov.see(K, int((scores[b] > np.float32(st)).sum()), int(cnt[b]))
                if dist == 'normal' and np.unique(scores[0]).size == A:
                    M = int((scores[0] > np.float32(st)).sum())
                    assert M == min({'0': 0, '1': 1, 'K-1': K - 1, 'K': K, 'K+1': K + 1, 'all': A}[target], A), case
    assert posts == {'none', 'scales', 'shifts'}
    cov.check()


def test_detect_wide_ties_at_the_kth_key():
    """Every anchor (image 1: six of seven) scores exactly 1/C: thousands of ties at the K-th key, picked in ascending anchor order
    over many threads' runs of the ordered sweep."""
    for A, C, K in ((16848, 3, 1024), (73440, 2, 1024), (32400, 16, 65)):
        rs = np.random.RandomState(A + K)
        pred_np, anc_np = sweep._pred_case(rs, 'sat', 2, A, C)
        pred_np[..., C] = 25.0
        pred_np[..., :C] = 0.0
        pred_np[1, ::7, C] = -1.0
        pred, anchors = torch.from_numpy(pred_np).cuda(), torch.from_numpy(anc_np).cuda()
        ids, scores, boxes = (t.cpu().numpy() for t in ops.decode(pred, anchors, SIZE, C))
        tie = np.float32(1.0) / np.float32(C)
        assert (scores[0] == tie).all() and int((scores[1] == tie).sum()) - K >= 2000      # thousands of ties at the K-th key
        for nms in NMS_LIST:
            got = tuple(t.cpu().numpy() for t in ops.detect_wide(pred, anchors, SIZE, C, K, nms, 0.0))
            for b in range(2):
                exp = oracle.filter_detections(ids[b], scores[b], boxes[b], K, nms, 0.0, C)
                sweep._expect(dict(mode='wide ties', A=A, C=C, K=K, nms=nms), got, b, exp)
            if nms == 1.0:
                assert int(got[0][0]) == K                                # nothing suppressed: the first K anchors, all of them kept


def _eq(name, g, r, case):
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t      # noqa: E731
    assert torch.equal(bits(g), bits(r)), f'{case}: wide {name} differs from the narrow kernel'


def test_wide_equals_narrow_where_both_run():
    """Second witness: for K <= 64 and A <= 25 596 the two paths give the same bits, on 20-image batches, in both modes."""
    names = ('count', 'class_ids', 'scores', 'boxes', 'anchor_idx')
    n = 0
    for ai, A in enumerate((1, 64, 65, 1025, 16848, 25596)):
        for d, dist in enumerate(('normal', 'grid', 'sat')):
            for K in (1, 63, 64):
                n += 1
                C, nms, target = C_LIST[n % 5], NMS_LIST[n % 3], M_TARGETS[n % 6]
                post = ('none', 'scales', 'shifts')[n % 3]
                rs = np.random.RandomState(400000 + n)
                pred_np, anc_np = sweep._pred_case(rs, dist, 20, A, C)
                pred, anchors = torch.from_numpy(pred_np).cuda(), torch.from_numpy(anc_np).cuda()
                ids, scores, boxes = ops.decode(pred, anchors, SIZE, C)
                st = sweep._thresh(scores[0].cpu().numpy(), target, K)
                aux, _ = sweep._post(rs, post, 20)
                kw = {} if aux is None else {post: torch.from_numpy(aux).cuda()}
                case = dict(A=A, C=C, K=K, dist=dist, nms=nms, M_target=target, post=post)
                for name, g, r in zip(names, ops.detect_wide(pred, anchors, SIZE, C, K, nms, st, **kw),
                                      ops.detect(pred, anchors, SIZE, C, K, nms, st, **kw)):
                    _eq(name, g, r, case)
                for name, g, r in zip(names, ops.filter_dense_wide(ids, scores, boxes, C, K, nms, st),
                                      ops.filter_dense(ids, scores, boxes, C, K, nms, st)):
                    _eq(name + ' (dense)', g, r, case)


def test_wide_buffers_are_reusable_and_refusals_write_nothing():
    B, A, C, K = 3, 32400, 3, 256
    dev = torch.device('cuda')
    bufs = ops._det_buffers(B, K, dev, A)
    assert bufs[5].numel() == ops.det_workspace_words_wide(B, A, K)
    bufs[5].fill_(-1)                                                   # the workspace needs no particular contents
    fresh = []
    for it, (dist, st) in enumerate((('normal', 0.05), ('grid', 0.0), ('sat', 0.3), ('normal', 0.9))):
        rs = np.random.RandomState(500 + it)
        pred_np, anc_np = sweep._pred_case(rs, dist, B, A, C)
        pred, anchors = torch.from_numpy(pred_np).cuda(), torch.from_numpy(anc_np).cuda()
        want = ops.detect_wide(pred, anchors, SIZE, C, K, 0.4, st)      # fresh result buffers, fresh workspace
        for t in bufs[:5]:
            t.zero_()
        got = ops.detect_wide(pred, anchors, SIZE, C, K, 0.4, st, out=bufs)
        assert all(g.data_ptr() == t.data_ptr() for g, t in zip(got, bufs))
        for name, g, r in zip(('count', 'class_ids', 'scores', 'boxes', 'anchor_idx'), got, want):
            _eq(name, g, r, f'launch {it} into reused buffers')
        ids, scores, boxes = (t.cpu().numpy() for t in ops.decode(pred, anchors, SIZE, C))
        res = tuple(t.cpu().numpy() for t in got)
        for b in range(B):
            sweep._expect(f'reuse, launch {it}', res, b, oracle.filter_detections(ids[b], scores[b], boxes[b], K, 0.4, st, C))
        fresh.append(int(got[0].max()))
    assert max(fresh) > 64 and len(set(fresh)) > 1
    # K = 1025: refused before anything is written, whatever buffers come with it
    big = tuple(t.fill_(7) for t in ops._det_buffers(B, 1025, dev)) + (torch.full((B * A,), 7, device=dev, dtype=torch.int32),)
    before = [t.clone() for t in big]
    with pytest.raises(ValueError, match='1024'):
        ops.detect_wide(pred, anchors, SIZE, C, 1025, 0.4, 0.3, out=big)
    with pytest.raises(ValueError, match='1024'):
        ops.filter_dense_wide(torch.from_numpy(ids).cuda(), torch.from_numpy(scores).cuda(), torch.from_numpy(boxes).cuda(), C, 1025)
    torch.cuda.synchronize()
    assert all(torch.equal(t, u) for t, u in zip(big, before))
    # result buffers of the wrong shape are refused as the narrow call refuses them
    small = tuple(t.fill_(7) for t in ops._det_buffers(B, 64, dev))
    with pytest.raises(ValueError):
        ops.detect_wide(pred, anchors, SIZE, C, K, 0.4, 0.3, out=small)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in small)


# ---- Detector ------------------------------------------------------------------------------------------------------------------------
def _detector(input_size, K, batch_size=2, seed=1234):
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    cfg = sqd.make_cfg(input_size=input_size)
    cfg.batch_size = batch_size
    cfg.keep_top_k = K
    m = SqueezeDet(cfg)
    sd = synthetic.make_state_dict('squeezedet', seed=seed)
    m.load_state_dict(sd)
    return Detector(m, cfg), cfg, sd


def _detect_device_vs_oracle(det, cfg, x, what):
    """``detect_device`` == the oracle on ``ops.decode`` of the device's own pred, exactly.  -> kept per image"""
    with torch.no_grad():
        pred = det.model.base(x)
        got = tuple(t.cpu().numpy() for t in det.detect_device(x))
    anchors = det.model.resolver.anchors_on(pred.device)
    ids, scores, boxes = (t.cpu().numpy() for t in ops.decode(pred, anchors, cfg.input_size, cfg.num_classes))
    for b in range(x.shape[0]):
        exp = oracle.filter_detections(ids[b], scores[b], boxes[b], cfg.keep_top_k, cfg.nms_thresh, cfg.score_thresh, cfg.num_classes)
        sweep._expect(what, got, b, exp)
    return [int(n) for n in got[0]], pred


def test_detector_kitti_size_keep_top_k_256():
    from squeezedet_pytorch_amd import synthetic
    det, cfg, _ = _detector((384, 1248), 256)
    assert ops.detect_path(cfg.keep_top_k, cfg.num_anchors) == 'wide'
    x = synthetic.make_images(2, cfg.input_size, seed=5).cuda()
    kept, _ = _detect_device_vs_oracle(det, cfg, x, 'Detector 384x1248 K=256')
    assert min(kept) > 64, kept                                         # (the CPU oracle keeps 88 and 89 on its own predictions)


@pytest.mark.parametrize('K', (64, 256))
def test_detector_720p(K):
    """A = 80 x 45 x 9 = 32 400 anchors: past the narrow kernel's anchor cap at any K."""
    from squeezedet_pytorch_amd import synthetic
    size = (720, 1280)
    det, cfg, sd = _detector(size, K)
    assert cfg.num_anchors == 32400 and ops.detect_path(K, cfg.num_anchors) == 'wide'
    x = synthetic.make_images(2, size, seed=5)
    kept, pred = _detect_device_vs_oracle(det, cfg, x.cuda(), f'Detector 720x1280 K={K}')
    ref = oracle.backbone_forward(x, sd)
    assert tuple(pred.shape) == tuple(ref.shape) == (2, 32400, 8)
    assert (pred.cpu() - ref).abs().max().item() <= 1e-4
    if K == 256:
        assert min(kept) > 64, kept                                     # (the CPU oracle keeps 129 and 108 on its own predictions)
    else:
        assert max(kept) <= 64 and min(kept) > 0, kept


def test_detector_filter_keep_top_k_128():
    det, cfg, _ = _detector((384, 1248), 128)
    A, C = cfg.num_anchors, cfg.num_classes
    for seed, st in ((0, 0.0), (1, 0.3)):
        rs = np.random.RandomState(600 + seed)
        s = sweep._dense_scores(rs, 'distinct', A)
        c = rs.randint(0, C, A).astype(np.int64)
        bx = sweep._dense_boxes(rs, A)
        cfg.score_thresh = st
        got = det.filter({'class_ids': torch.from_numpy(c).cuda(), 'scores': torch.from_numpy(s).cuda(), 'boxes': torch.from_numpy(bx).cuda()})
        exp = oracle.filter_detections(c, s, bx, 128, cfg.nms_thresh, st, C)
        assert len(exp['scores']) > 64
        assert np.array_equal(got['anchor_idx'].cpu().numpy(), exp['anchor_idx'])
        assert np.array_equal(got['class_ids'].cpu().numpy(), exp['class_ids'])
        assert np.array_equal(sweep._bits(got['scores'].cpu().numpy()), sweep._bits(exp['scores']))
        assert np.array_equal(sweep._bits(got['boxes'].cpu().numpy()), sweep._bits(exp['boxes']))


def _images(n, sizes, seed=5):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        base = rs.standard_normal((-(-h // 8), -(-w // 8), 3)) * 60 + 100
        out.append(np.clip(np.kron(base, np.ones((8, 8, 1))), 0, 255).astype(np.uint8)[:h, :w])
    return out


def _same(r, w):
    assert ('boxes' in r) == ('boxes' in w)
    if 'boxes' in r:
        for k in ('anchor_idx', 'boxes', 'scores', 'class_ids'):
            assert np.array_equal(r[k], w[k]) and r[k].dtype == w[k].dtype, k
    assert r['image_meta']['orig_size'].tolist() == w['image_meta']['orig_size'].tolist()


def test_detect_stream_keep_top_k_256_and_path_switches():
    """The lane executor on the wide path: eager first use, capture, replay -- bit for bit ``detect_images`` -- and one Detector
    switched 64 -> 256 -> 64: the path changes under the lanes, whose graphs and buffers are dropped and re-captured each time."""
    det, cfg, _ = _detector((384, 1248), 256)
    images = _images(2, [(375, 1242), (370, 1224)])
    ex = det.stream()

    def stream_equals_detect_images():
        want = det.detect_images(images)
        got = list(det.detect_stream([images] * 5))                     # 2 lanes: eager, eager, capture, capture, replay
        assert len(got) == 5 and not ex.degraded
        for res in got:
            for r, w in zip(res, want):
                _same(r, w)
        return [len(w.get('scores', ())) for w in want]

    n256 = stream_equals_detect_images()
    assert ex.captures == 2 and ex.replayed_batches == 3, (ex.captures, ex.replayed_batches)
    assert stream_equals_detect_images() == n256 and ex.captures == 2   # second pass: replays only
    cfg.keep_top_k = 64
    n64 = stream_equals_detect_images()
    assert ex.captures == 4 and max(n64) <= 64
    cfg.keep_top_k = 256
    assert stream_equals_detect_images() == n256 and ex.captures == 6
    cfg.keep_top_k = 64
    assert stream_equals_detect_images() == n64 and ex.captures == 8
