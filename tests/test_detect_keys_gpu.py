"""GPU tier: the keys form of the detection tail -- ConvDet's V-shared Winograd launch (csrc/conv_wino_vs.hip,
``sqd_conv_wino_vs_keys_fwd``) stores every anchor's score key next to ``pred``, and the fused detect (csrc/postproc.hip,
``sqd_detect_keys_fwd``) loads them instead of scoring ``pred`` again.  Everything is compared bit for bit with the forms that were
there before: ``pred`` with the plain ConvDet entry, the keys with ``where(score > thr, bits(score), 0)`` of ``ops.decode`` (the same
``anchor_score``), the detections with the split form, the one-workgroup form and the dense filter.

Shapes are small: the failure modes are at group, quad and tie edges (exact groups, partial rows and columns, a map smaller than a
group), not at size.  The threshold of a case is an existing score -- the one that 15 % of the batch's anchors exceed -- so the share
of anchors that pass is 5-30 % whatever the zero padding does to the logits of a small map, and one anchor sits exactly AT the
threshold.  Rule for the workspace words that are no key (A .. ceil4(A)-1 of an image, the arrival counters behind the keys): the
ConvDet launch leaves them untouched and the detect launch never looks at them -- they are pre-filled with a sentinel here."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, APC, NC, N = 3, 9, 3, 72
SIZE = (384, 1248)
SENTINEL = 0x5eadbeef
SHAPES = [(C, H, W) for C in (8, 24) for (H, W) in ((4, 16), (5, 7), (9, 33), (1, 1))]


def _u32(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


class _Head:
    """One ConvDet + detect problem on the device: input x [B,H,W,C], a three-class ConvDet (weights w, bias b), anchors."""

    def __init__(self, C, H, W, seed=0, w=None, b=None):
        from squeezedet_pytorch_amd import ops
        rs = np.random.RandomState(1000 * C + 10 * H + W + seed)
        self.H, self.W, self.C, self.A = H, W, C, H * W * APC
        self.x = torch.from_numpy(rs.standard_normal((B, H, W, C)).astype(np.float32)).cuda()
        if w is None:
            w = (rs.standard_normal((N, C, 3, 3)) * (1.0 / (9 * C)) ** 0.5).astype(np.float32)      # logits ~ N(0, 1) inside the map
            b = (rs.standard_normal(N) * 0.1).astype(np.float32)
            b[3::8] -= 1.0                                                                        # confidence logits centred at -1
        self.w_np, self.b_np = w, b
        self.plan = ops.WinoPlan(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(), ops.WINO_VS_CFG)
        cx, cy = rs.uniform(0, SIZE[1], self.A), rs.uniform(0, SIZE[0], self.A)
        self.anchors = torch.from_numpy(np.stack([cx, cy, rs.uniform(20, 200, self.A), rs.uniform(20, 200, self.A)], 1).astype(np.float32)).cuda()
        self.words = ops.det_workspace_words(B, self.A)
        y = torch.empty(B, H, W, N, device='cuda')
        ops.conv_wino(self.x, 0, self.plan, y, 0)                        # the plain entry: the reference pred
        self.pred = y.view(B, self.A, NC + 5)
        self.dec = ops.decode(self.pred, self.anchors, SIZE, NC)         # (class_ids, scores, boxes): the same anchor_score
        torch.cuda.synchronize()

    def quantile_thresh(self, share=0.15):
        s = np.sort(self.dec[1].cpu().numpy().reshape(-1))[::-1]
        return float(s[int(share * s.size)])

    def workspace(self):
        return torch.full((self.words,), SENTINEL, device='cuda', dtype=torch.int32)

    def convdet_keys(self, thr, ws, y=None):
        from squeezedet_pytorch_amd import ops
        y = torch.full((B, self.H, self.W, N), 7.0, device='cuda') if y is None else y
        with ops.det_keys_request(ops.DetKeys(ws, thr, APC, NC)) as req:
            ops.conv_wino(self.x, 0, self.plan, y, 0)
        assert req.written and ops.det_keys_request.current() is None
        return y.view(B, self.A, NC + 5)

    def want_keys(self, thr):
        s = self.dec[1].cpu().numpy()
        return np.where(s > np.float32(thr), s.view(np.uint32), np.uint32(0))

    def detect(self, form, thr, K=64, nms=0.4, scales=None, shifts=None, out=None, pred=None, ws=None):
        """The five outputs + count of one launch form, as numpy arrays."""
        from squeezedet_pytorch_amd import ops
        pred = self.pred if pred is None else pred
        if form == 'dense':
            got = ops.filter_dense(self.dec[0], self.dec[1], self.dec[2], NC, K, nms, thr)
        else:
            if out is None:
                out = ops._det_buffers(B, K, 'cuda')
            ws = {'keys': ws, 'split': torch.zeros(self.words, device='cuda', dtype=torch.int32),
                  'one': torch.zeros(1, device='cuda', dtype=torch.int32)}[form]
            got = ops.detect(pred, self.anchors, SIZE, NC, K, nms, thr, scales=scales, shifts=shifts, out=tuple(out[:5]) + (ws,),
                             keys_ready=(form == 'keys'))
        return tuple(t.cpu().numpy() for t in got)


@functools.lru_cache(maxsize=None)
def _head(C, H, W):
    return _Head(C, H, W)


def _same_rows(case, got, want):
    cnt, cntw = got[0], want[0]
    assert np.array_equal(cnt, cntw), f'{case}: det_count {cnt.tolist()} != {cntw.tolist()}'
    for b in range(B):
        n = int(cnt[b])
        for name, g, w in zip(('class_ids', 'scores', 'boxes', 'anchor_idx'), got[1:], want[1:]):
            assert g[b, :n].tobytes() == w[b, :n].tobytes(), f'{case}, image {b}: {name} differ'


def _check_all_forms(h, thr, K=64, nms=0.4, scales=None, shifts=None, case=''):
    ws = h.workspace()
    pred = h.convdet_keys(thr, ws)
    assert torch.equal(pred, h.pred), f'{case}: pred of the keys entry differs from the plain entry'
    kw = _u32(ws)
    A4 = -(-h.A // 4) * 4
    keys = kw[:B * A4].reshape(B, A4)
    assert np.array_equal(keys[:, :h.A], h.want_keys(thr)), f'{case}: keys'
    assert (keys[:, h.A:] == SENTINEL).all() and (kw[B * A4:] == SENTINEL).all(), f'{case}: words that are no key were written'
    got = h.detect('keys', thr, K, nms, scales, shifts, pred=pred, ws=ws)
    assert np.array_equal(_u32(ws), kw), f'{case}: the detect launch wrote to the key workspace'
    _same_rows(f'{case} keys vs split', got, h.detect('split', thr, K, nms, scales, shifts))
    _same_rows(f'{case} keys vs one workgroup', got, h.detect('one', thr, K, nms, scales, shifts))
    if scales is None and shifts is None:
        _same_rows(f'{case} keys vs dense filter', got, h.detect('dense', thr, K, nms))
    return got, keys[:, :h.A]


@pytest.mark.parametrize('C,H,W', SHAPES)
def test_pred_keys_and_detections_equal_the_existing_forms(C, H, W):
    h = _head(C, H, W)
    thr = h.quantile_thresh()
    got, keys = _check_all_forms(h, thr, case=f'C{C} {H}x{W} thr {thr!r}')
    share = float((keys != 0).mean())
    assert 0.05 <= share <= 0.30, share
    assert int(got[0].sum()) > 0
    assert bool((h.dec[1] == thr).any())                         # an anchor exactly at the threshold: not a candidate


def test_no_anchor_above_the_threshold():
    h = _head(8, 9, 33)
    got, keys = _check_all_forms(h, 0.99999, case='count 0')
    assert not keys.any() and not got[0].any()


@pytest.mark.parametrize('K', [1, 64])
def test_ties_at_the_kth_key_and_keep_top_k(K):
    """Every anchor of a cell carries the weights of anchor 0: nine exactly equal scores per pixel, far more than K candidates, the
    K-th key tied (64 = 7 x 9 + 1).  The tie rule (ascending anchor index) must hold through the keys form as well."""
    base = _head(8, 9, 33)
    w, b = base.w_np.copy(), base.b_np.copy()
    for k in range(1, APC):
        w[8 * k:8 * k + 8], b[8 * k:8 * k + 8] = w[:8], b[:8]
    h = _Head(8, 9, 33, w=w, b=b)
    got, keys = _check_all_forms(h, 0.05, K=K, nms=1.0, case=f'ties K{K}')          # (nms 1: nothing suppressed, all K survive)
    assert ((keys != 0).sum(1) > 64).all()
    k3 = keys.reshape(B, -1, APC)
    assert (k3 == k3[:, :, :1]).all()
    assert (got[0] == K).all()


def test_confidence_and_score_exactly_at_the_threshold():
    """Anchor 0 of every cell has zero weights and the biases (40, 0, 0 | 0): softmax = 1 exactly, confidence = 0.5 exactly, score
    = 0.5 exactly.  At score_thresh = 0.5 neither `conf > thr` nor `score > thr` holds (key 0); one ulp below both hold."""
    base = _head(8, 9, 33)
    w, b = base.w_np.copy(), base.b_np.copy()
    w[:4] = 0.0
    b[:4] = (40.0, 0.0, 0.0, 0.0)
    h = _Head(8, 9, 33, w=w, b=b)
    half = np.float32(0.5)
    _, keys = _check_all_forms(h, 0.5, case='conf == thr')
    assert not keys.reshape(B, -1, APC)[:, :, 0].any()
    _, keys = _check_all_forms(h, float(np.nextafter(half, np.float32(0))), case='conf one ulp above thr')
    assert (keys.reshape(B, -1, APC)[:, :, 0] == half.view(np.uint32)).all()


def test_scales_and_shifts():
    h = _head(24, 9, 33)
    rs = np.random.RandomState(5)
    scales = torch.from_numpy(rs.uniform(0.5, 2.0, (B, 2)).astype(np.float32)).cuda()
    shifts = torch.from_numpy(rs.uniform(-30, 30, (B, 2)).astype(np.float32)).cuda()
    thr = h.quantile_thresh()
    for sc, sh in ((scales, None), (None, shifts), (scales, shifts)):
        _check_all_forms(h, thr, scales=sc, shifts=sh, case=f'scales {sc is not None} shifts {sh is not None}')


def test_run_to_run_with_stale_buffers():
    from squeezedet_pytorch_amd import ops
    h, other = _head(24, 9, 33), _Head(24, 9, 33, seed=77)
    thr = h.quantile_thresh()
    ws = h.workspace()
    out = ops._det_buffers(B, 64, 'cuda')
    y = torch.empty(B, h.H, h.W, N, device='cuda')
    other.detect('keys', thr, out=out, pred=other.convdet_keys(thr, ws, y), ws=ws)       # another batch leaves its keys and rows behind
    runs = []
    for _ in range(3):
        pred = h.convdet_keys(thr, ws, y)
        got = h.detect('keys', thr, out=out, pred=pred, ws=ws)
        runs.append((_u32(ws).copy(), _u32(y).copy()) + tuple(g.tobytes() for g in got))
    for r in runs[1:]:
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(r, runs[0]))
    _same_rows('stale buffers', got, h.detect('split', thr))


def test_unsupported_heads_are_refused_and_nothing_is_written():
    from squeezedet_pytorch_amd import _native as nat
    h = _head(8, 4, 16)
    ws = h.workspace()
    y = torch.full((B, h.H, h.W, N), 7.0, device='cuda')

    def call(N_=N, Npad=80, pitch=N, coff=0, relu=0, apc=APC, nc=NC, keys=ws, thr=0.3):
        return nat.lib().sqd_conv_wino_vs_keys_fwd(nat.ptr(h.x), nat.ptr(h.plan.w), nat.ptr(h.plan.bias), nat.ptr(y), B, h.H, h.W, h.C, h.C, 0,
                                                   N_, Npad, pitch, coff, relu, nat.ptr(keys), thr, apc, nc, nat.stream_handle(h.x.device))
    assert call(nc=4) == nat.ERR_UNSUPPORTED
    assert call(apc=8) == nat.ERR_UNSUPPORTED                           # N != 8 * anchors_per_cell
    assert call(N_=64, apc=9) == nat.ERR_UNSUPPORTED
    assert call(relu=1) == nat.ERR_UNSUPPORTED
    assert call(keys=None) == nat.ERR_BAD_ARG
    assert call(thr=-0.1) == nat.ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and (_u32(ws) == SENTINEL).all()
    assert call() == 0                                                  # (the same arguments, supported: it does run)
    torch.cuda.synchronize()
    assert torch.equal(y.view(B, h.A, NC + 5), h.pred)


def test_detector_and_two_lane_stream_with_the_keys_form_on_and_off(monkeypatch):
    """Detector.detect_device and a two-lane Detector.stream() on a 2-image 64x96 input, ``fuse_detect_keys`` on and off: the same bytes
    and the same recorded launches.  The measured table sends so small a ConvDet to another Winograd kernel (the keys request is
    then simply not honoured); the second round sends it to the V-shared kernel, as at the benchmarked shape, so the keys form runs."""
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import model as model_mod, ops, synthetic, tiles, timing
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet
    size = (64, 96)
    cfg = sqd.make_cfg(input_size=size, device='cuda:0')
    cfg.score_thresh = 0.05
    model = SqueezeDet(cfg)
    model.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    det = Detector(model, cfg)
    x = synthetic.make_images(2, size, seed=0).cuda()
    table_cfg = model_mod.conv3x3_cfg

    def run():
        kt = timing.KernelTimer()
        timing.set_timer(kt)
        try:
            one = tuple(t.cpu().numpy() for t in det.detect_device(x))
        finally:
            timing.set_timer(None)
        names = [(r[0], r[1]) for r in kt.records]
        ex = det.stream(lanes=2)
        for i in range(6):                                              # per lane: eager, capture, replay
            ex.submit_device(x, tag=i)
        res = [r for _t, r in ex.drain()]
        assert not ex.degraded and ex.replayed_batches > 0
        return one, names, res

    for force_vs in (False, True):
        if force_vs:
            monkeypatch.setattr(model_mod, 'conv3x3_cfg',
                                lambda C, Nn, npix, use: (True, tiles.WINO_VS_CFG) if Nn == N else table_cfg(C, Nn, npix, use))
        wrote = []
        real = ops.detect

        def spy(*a, **k):
            wrote.append(bool(k.get('keys_ready')))
            return real(*a, **k)
        monkeypatch.setattr(ops, 'detect', spy)
        model.base.fuse_detect_keys = True
        on = run()
        assert all(wrote) == force_vs and any(wrote) == force_vs, wrote
        del wrote[:]
        model.base.fuse_detect_keys = False
        off = run()
        assert not any(wrote)
        monkeypatch.setattr(ops, 'detect', real)
        assert on[1] == off[1] and on[1][-1][0] == 'detect' and (not force_vs or on[1][-2][0] == 'conv_wino_vs')
        cnt = off[0][0]
        assert int(cnt.sum()) > 0
        for got in (on[0],) + tuple((r.count, r.class_ids, r.scores, r.boxes, r.anchor_idx) for r in on[2] + off[2]):
            assert np.array_equal(got[0], cnt)
            for b in range(2):
                n = int(cnt[b])
                for g, w in zip(got[1:], off[0][1:]):
                    assert g[b, :n].tobytes() == w[b, :n].tobytes()
