"""CPU tier: tests/test_fp64_launches_gpu.py has one case per (arch, batch, kernel, shape tag) entry of the four benchmarked launch plans
(recomputed here on the host with the shipped tuning table), and no case that the plans no longer contain.  A new kernel, tuning row
or fusion that changes a plan fails here until it has a float64 case.  The plain references of tests/fp64_ref.py are checked against
torch's own convolution, pooling and autograd on small shapes; the loss reference against float64 autograd, its bound against the
float32 oracle chain (attainability), and each wrong branch convention against the loss edge cases (teeth); the clip + SGD reference
against torch.optim.SGD + clip_grad_norm_, and the norm bar against a norm that drops the tail or a part."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ref as R  # noqa: E402
import test_fp64_launches_gpu as L  # noqa: E402
import test_fp64_loss_gpu as LG  # noqa: E402
import test_fp64_optim_gpu as OG  # noqa: E402

# launches outside the float64 sweep, each with the test that covers it
ALLOWED = {
    'detect': 'tests/test_detect_sweep_gpu.py (exact against oracle.filter_detections)',
}


def plan_entries():
    from squeezedet_pytorch_amd import plan
    out = []
    for arch, batch in L.STEPS:
        for planner in (plan.inference_launch_plan, plan.training_launch_plan):
            for kernel, tag in planner(arch, batch, L.INPUT):
                e = (arch, batch, kernel, tag)
                if e not in out:
                    out.append(e)
    return out


def test_every_plan_entry_has_a_case():
    entries = plan_entries()
    cases = set(L.CASES)
    assert len(cases) == len(L.CASES), 'duplicate cases'
    missing = [e for e in entries if e not in cases and e[2] not in ALLOWED]
    assert not missing, f'launches of the benchmarked steps without a float64 case: {missing}'
    stale = [c for c in L.CASES if c not in entries]
    assert not stale, f'cases the benchmarked plans no longer launch: {stale}'
    assert all(c[2] not in ALLOWED for c in L.CASES)


def test_every_case_family_has_a_bar():
    for c in L.CASES:
        f = L.family(c[2])
        assert f == 'maxpool_fwd' or f == 'wgrad_reduce_batched' or f in L.FAMILIES or f in L.LOSS_FAMILIES, c


def _rand(*shape, seed, relu=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g, dtype=torch.float64)
    return t.clamp_min(0) if relu else t


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('k', [1, 3])
def test_reference_conv_dgrad_wgrad(k):
    x = _rand(2, 5, 6, 7, seed=1, relu=True)
    w = _rand(8, 5, k, k, seed=2)
    b = _rand(8, seed=3)
    want = F.conv2d(x, w, b, padding=k // 2)
    r = R.conv(_nhwc(x), w, b)
    assert torch.allclose(r.ref64, _nhwc(want), atol=1e-12)
    assert (r.M >= r.ref64.abs() - 1e-12).all()
    assert torch.allclose(r.b32.double(), r.ref64, atol=1e-5)
    xg = x.clone().requires_grad_(True); wg = w.clone().requires_grad_(True); bg = b.clone().requires_grad_(True)
    dy = _rand(*want.shape, seed=4)
    F.conv2d(xg, wg, bg, padding=k // 2).backward(dy)
    assert torch.allclose(R.conv(_nhwc(dy), R.dgrad_weight(w)).ref64, _nhwc(xg.grad), atol=1e-12)
    dW, db = R.wgrad(_nhwc(dy), _nhwc(x), k * k)
    assert torch.allclose(dW.ref64, wg.grad, atol=1e-12) and torch.allclose(db.ref64, bg.grad, atol=1e-12)


@pytest.mark.parametrize('k,H,W', [(3, 13, 18), (7, 14, 17)])
def test_reference_stem_pool_and_backward(k, H, W):
    img = _rand(2, 3, H, W, seed=5)
    w = _rand(6, 3, k, k, seed=6).requires_grad_(True)
    b = _rand(6, seed=7).requires_grad_(True)
    s = F.relu(F.conv2d(img, w, b, stride=2, padding=k // 2))
    p, idx = F.max_pool2d(s, 3, 2, ceil_mode=True, return_indices=True)
    r = R.stem_pool(img, w.detach(), b.detach())
    assert torch.allclose(r.ref64, _nhwc(p.detach()), atol=1e-12)
    # the kernel's codes: tap of the window (15 where the pooled value is not > 0, the ReLU mask)
    Ho, Wo = p.shape[2:]
    Ws = s.shape[3]
    oy = torch.arange(Ho).view(1, 1, Ho, 1) * 2
    ox = torch.arange(Wo).view(1, 1, 1, Wo) * 2
    codes = (idx // Ws - oy) * 3 + (idx % Ws - ox)
    codes = torch.where(p > 0, codes, torch.full_like(codes, 15)).to(torch.uint8)
    dp = _rand(*p.shape, seed=8)
    p.backward(dp)
    dW, db = R.stem_wgrad_pooled(_nhwc(dp), _nhwc(codes), img, 6, k)
    assert torch.allclose(dW.ref64, w.grad, atol=1e-10) and torch.allclose(db.ref64, b.grad, atol=1e-10)
    sp = _nhwc(s.detach())
    dx = R.maxpool_bwd(_nhwc(dp), _nhwc(codes), sp.shape[1:3])
    sg = s.detach().clone().requires_grad_(True)
    F.max_pool2d(sg, 3, 2, ceil_mode=True).backward(dp * (p > 0))
    assert torch.allclose(dx.ref64, _nhwc(sg.grad), atol=1e-12)


def test_reference_bridge_magnitude_bounds_the_fp32_chain():
    x = _rand(2, 9, 11, 8, seed=9, relu=True).float()
    ws = [_rand(*s, seed=10 + i).float() * 0.3 for i, s in enumerate([(4, 8, 1, 1), (4,), (4, 8, 3, 3), (4,), (8, 8, 1, 1), (8,)])]
    for y, mid in (R.fire_bridge(x, *ws), R.fire_pool_bridge(x, *ws)):
        for r in (y, mid):
            assert ((r.b32.double() - r.ref64).abs() <= R.BAR_L * r.M).all()
            assert R.bars(r.b32, r, 'act', 2)['p_ok']


def test_bars_reject_a_misplaced_term_and_the_emulations():
    x = _rand(4, 12, 12, 64, seed=20).abs().float()
    w = _rand(64, 64, 3, 3, seed=21).float() * 0.05
    b = _rand(64, seed=22).float()
    r = R.conv(x, w, b)
    got = r.b32.clone()
    assert R.bars(got, r, 'act', 2)['l_ok']
    got[1, 5, 7, 3] += float(w[3, 7, 1, 1] * x[1, 5, 7, 7])          # one duplicated product
    assert not R.bars(got, r, 'act', 2)['l_ok']
    for emu in ('bf16', 'split3'):
        assert not R.bars(R.conv(x, w, b, emu=emu).b32, r, 'act', 4)['p_ok'], emu


@pytest.mark.parametrize('taps,S,blocking,step', [(1, 3, ('px', 32), 4), (1, 5, ('px', 128), 4), (9, 4, 'tile', 16), (9, 1, 'tile', 16)])
def test_reference_split_k_restatement(taps, S, blocking, step):
    dy = _rand(2, 9, 37, 8, seed=30, relu=True)
    x = _rand(2, 9, 37, 12, seed=31, relu=True)
    dW, db = R.wgrad(dy, x, taps)
    w32, b32 = R.wgrad_split_k(dy, x, taps, S, blocking, step)
    assert w32.dtype == torch.float32 and tuple(w32.shape) == tuple(dW.ref64.shape)
    assert ((w32.double() - dW.ref64).abs() <= R.BAR_L * dW.M).all()
    assert ((b32.double() - db.ref64).abs() <= R.BAR_L * db.M).all()
    assert R.bars(w32, R.Ref(dW.ref64, dW.M, w32), 'wgrad', 2)['p_ok']


# ---- the loss ----

def _bench_like(B=4, seed=11):
    """Operands shaped like the benchmarked loss launch: the KITTI anchors (A = 16848), the synthetic head's scales, synthetic gt."""
    import numpy as np
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    cfg = sqd.make_cfg()
    rs = np.random.RandomState(seed)
    pred = (rs.standard_normal((B, cfg.num_anchors, 8)) * np.array([2, 2, 2, 1.5, .4, .4, .4, .4])).astype(np.float32)
    pred[..., 3] -= 2.0
    gt = synthetic.make_gt(B, cfg.anchors, cfg.input_size, seed=1)
    return torch.from_numpy(pred), gt, torch.from_numpy(cfg.anchors).float(), cfg.input_size


def _loss_cases():
    yield 'bench', _bench_like(), 3
    for C in (1, 3, 16):
        yield f'edges C{C}', LG.edge_case(C=C) + (LG.SIZE,), C
    yield 'saturated', LG.saturated_case() + (LG.SIZE,), 3
    yield 'n_obj 0 and A', LG.random_case(4, 500, 3, seed=300, nobj=[37, 0, 500, 11]) + (LG.SIZE,), 3
    yield 'A1', LG.random_case(2, 1, 3, seed=101) + (LG.SIZE,), 3


_LOSS_REFS = {}


def _loss_ref(name, ops, C, mutant=None):
    key = (name, mutant)
    if key not in _LOSS_REFS:
        pred, gt, anchors, size = ops
        _LOSS_REFS[key] = R.loss(pred, gt, anchors, size, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=LG.make_coef(pred.shape[0], 3), mutant=mutant)
    return _LOSS_REFS[key]


@pytest.mark.parametrize('name,ops,C', list(_loss_cases()), ids=[c[0] for c in _loss_cases()])
def test_loss_reference_attainable(name, ops, C):
    """The float32 oracle chain (torch autograd in float32 on the host) holds bar L with 4x headroom on every output of every edge case
    and on bench-shaped operands, and bar P trivially; nobj is exact; no exact construction flips a branch."""
    ref = _loss_ref(name, ops, C)
    for out in ('losses', 'mean4', 'dmean', 'dcoef'):
        r = ref[out]
        b = R.bars_nan(r.b32, r, 'dpred' if out[0] == 'd' else 'vec', 2)
        print(f'{name:16s} {out:7s} float32 chain max err/M {b["l_ratio"]:.2e}')
        assert b['nan_ok'] and b['l_ratio'] <= R.BAR_L / 4, (name, out, b)
    assert torch.equal(ref['nobj'], ops[1][..., 0].double().sum(1))
    assert int(ref['flips'].sum()) <= (4 if name == 'bench' else 0)


def test_loss_reference_matches_autograd():
    """The analytic chain (which M and the flipped-branch and mutant references come from) equals float64 autograd of the oracle, and
    torch 2.10's conventions are the ones it pins: clamp inclusive, ties split, clamp_min inclusive."""
    x = torch.tensor([0.0, 1.0, 5.0], dtype=torch.float64, requires_grad=True)
    x.clamp(0, 5).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 1.0]
    a = torch.tensor([1.0, 2.0], dtype=torch.float64, requires_grad=True)
    torch.min(a, torch.ones(2, dtype=torch.float64)).sum().backward()
    assert a.grad.tolist() == [0.5, 0.0]
    y = torch.tensor([0.0, -1.0], dtype=torch.float64, requires_grad=True)
    torch.clamp_min(y, 0).sum().backward()
    assert y.grad.tolist() == [1.0, 0.0]
    for name, ops, C in _loss_cases():
        pred, gt, anchors, size = ops
        B = pred.shape[0]
        ref = _loss_ref(name, ops, C)
        br = R._branches(*R._box64(pred, anchors, C), gt, size[1] - 1, size[0] - 1)
        for out, u in (('dmean', torch.full((3, B), float(torch.tensor(LG.GMEAN, dtype=torch.float32)) / B, dtype=torch.float64)),
                       ('dcoef', LG.make_coef(B, 3).double())):
            losses, _n, dp, _ = R._loss_chain(pred, gt, anchors, size, C, LG.WEIGHTS, u, br)
            r = ref[out].ref64
            fin = ~torch.isnan(r)
            assert torch.equal(torch.isnan(dp.v), ~fin), name
            assert bool(((dp.v[fin] - r[fin]).abs() <= 1e-12 * (dp.m[fin] + r[fin].abs())).all()), (name, out)
        lr = ref['losses'].ref64
        fin = ~torch.isnan(lr)
        assert torch.equal(torch.isnan(losses.v), ~fin)
        assert bool(((losses.v[fin] - lr[fin]).abs() <= 1e-12 * lr[fin].abs()).all()), name


@pytest.mark.parametrize('mutant', R.LOSS_MUTANTS)
def test_loss_mutants_fail_the_edge_cases(mutant):
    """Teeth of the GPU edge tests: a kernel that implemented a wrong convention (exclusive clamp, no tie split, clamp_min passing only
    above 0, a detached IoU path, A as the negative term's denominator) would move at least one element of the edge cases beyond bar
    L.  The reference under that convention stands in for the kernel."""
    moved = []
    for name, ops, C in _loss_cases():
        if name == 'bench':
            continue
        ref, mut = _loss_ref(name, ops, C), _loss_ref(name, ops, C, mutant)
        for out in ('losses', 'dmean', 'dcoef'):
            r = ref[out]
            if not R.bars_nan(mut[out].ref64, r, 'dpred' if out[0] == 'd' else 'vec', 2)['l_ok']:
                moved.append((name, out))
    print(mutant, moved)
    assert moved, f'{mutant}: no edge case tells it from the pinned convention'
    if mutant in ('clamp_exclusive', 'no_tie_split', 'clamp_min_strict'):
        assert ('edges C3', 'dmean') in moved


def test_loss_bar_p_rejects_bf16_operands():
    pred, gt, anchors, size = _bench_like(B=2)
    ref = R.loss(pred, gt, anchors, size, 3, LG.WEIGHTS, gmean=1.0)
    l16, d16, _ = R.loss_bf16(pred, gt, anchors, size, 3, LG.WEIGHTS, gmean=1.0)
    assert not R.bars(l16, ref['losses'], 'vec', 2)['p_ok']
    assert not R.bars(d16, ref['dmean'], 'dpred', 2)['p_ok']


# ---- clip + SGD ----

@pytest.mark.parametrize('max_norm,momentum,wd', [(5.0, 0.875, 2.0 ** -13), (0.5, 0.875, 0.0), (0.0, 0.0, 2.0 ** -13), (1e3, 0.875, 2.0 ** -13)])
def test_clip_sgd_reference_matches_torch(max_norm, momentum, wd):
    """R.clip_sgd against torch's own clip_grad_norm_ + SGD (float64), over two steps (zero buffer, then a carried one); the
    hyper-parameters are float32 values (the reference rounds them as the kernel receives them)."""
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 3), (5,), (2, 3, 3, 3), (1,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    mine = [p.detach().clone() for p in ps]
    bufs = [torch.zeros_like(p) for p in mine]
    lr = 2.0 ** -7
    opt = torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=wd)
    for _ in range(2):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        tn = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm > 0 else None
        opt.step()
        tn64, _coef, newp, newb = R.clip_sgd(mine, grads, bufs, lr, momentum, wd, max_norm)
        if tn is not None:
            assert abs(float(tn) - tn64) <= 1e-12 * tn64
        for p, r in zip(ps, newp):
            assert torch.allclose(p.detach(), r.ref64, rtol=1e-12, atol=1e-15)
            assert (r.M >= r.ref64.abs() - 1e-12).all()
        mine = [r.ref64 for r in newp]
        bufs = [r.ref64 for r in newb]
        if momentum > 0:
            for p, b in zip(ps, bufs):
                assert torch.allclose(opt.state[p]['momentum_buffer'], b, rtol=1e-12, atol=1e-15)


def test_norm_bar_rejects_dropped_tail_and_parts():
    """Teeth of the norm bar (2^-18 relative): a norm without the n & 3 tail fails it on the layout of total 3 and on one whose tail
    holds large values; a norm without one of the 256 partial sums fails it on the [1021] layout."""
    for sizes, big in (([3], False), (OG.TAIL_BIG, True), ([1021], False)):
        flat = OG.flat_values(sum(sizes), seed=1, big_tail=big)
        tn64 = float(flat.double().norm())
        n = flat.numel()
        nq = n >> 2
        no_tail = float(flat[:4 * nq].double().norm())
        assert abs(no_tail - tn64) > 2.0 ** -18 * tn64, sizes
        if sizes == [1021]:
            per = -(-nq // 256)
            for k in range(256):
                lo, hi = k * per, min(nq, (k + 1) * per)
                if hi <= lo:
                    continue
                keep = torch.ones(n, dtype=torch.bool)
                keep[4 * lo:4 * hi] = False
                assert abs(float(flat[keep].double().norm()) - tn64) > 2.0 ** -18 * tn64, k
