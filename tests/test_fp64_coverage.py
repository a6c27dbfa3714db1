"""CPU tier: tests/test_fp64_launches_gpu.py has one case per (arch, batch, kernel, shape tag) entry of the four benchmarked launch plans
(recomputed here on the host with the shipped tuning table), and no case that the plans no longer contain.  A new kernel, tuning row
or fusion that changes a plan fails here until it has a float64 case.  The plain references of tests/fp64_ref.py are checked against
torch's own convolution, pooling and autograd on small shapes."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ref as R  # noqa: E402
import test_fp64_launches_gpu as L  # noqa: E402

# launches outside the float64 sweep, each with the test that covers it
ALLOWED = {
    'detect': 'tests/test_detect_sweep_gpu.py (exact against oracle.filter_detections)',
    'loss_fwd': 'tests/test_training_gpu.py (loss against the oracle) and tests/test_headline_gpu.py',
    'loss_bwd': 'tests/test_training_gpu.py (loss gradient against the oracle) and tests/test_headline_gpu.py',
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
        assert f == 'maxpool_fwd' or f == 'wgrad_reduce_batched' or f in L.FAMILIES, c


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
