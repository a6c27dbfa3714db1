"""CPU tier: the mask stream of the counter-based dropout in front of ConvDet (csrc/sqd_common.h ``sqd_drop_key`` / ``sqd_drop_mul4``),
through its host restatement ``ops.dropout_mask_reference``.  tests/test_dropout_gpu.py pins the stand-alone kernel and both fused
epilogues to the restatement bit for bit, so what holds for it holds for every kernel that applies the dropout.

The keep indicators of n = 2^20 elements are held to the independent-Bernoulli(q = 1 - p) null, p in {0.5, 0.2, 0.75}, seeds and steps
fixed (the tests are deterministic).  Every statistic is a z-score under that null:
* single statistics, |z| <= 5 (P(|z| > 5) = 6e-7 for a Gaussian): the overall keep rate; products of the centred indicators at lags 1,
  2, 3 (inside a quad of one hash), 4, 8 (across quads), 768 (across a pixel of the 768-channel tensor) and 768 * 6 (across a row of
  the 70x100 input's 4x6 grid); the same product between the masks of step t and t + 1, of t and t + 2^32, and of seed s and
  s ^ (1 << b) for b in {0, 15, 16, 31, 32, 40, 47, 62};
* maxima over many statistics, max |z| <= 6 (P = 2e-9 each, at most 1365 of them): the keep rate of every channel and of every pixel
  (the first 1365 * 768 elements viewed [1365, 768]);
* the joint distribution of the four fields of a quad: chi-square of the 16 keep patterns against q^k (1 - q)^(4 - k), 15 degrees of
  freedom, bound 50 (P = 1e-5).
The bounds are tail bounds of the null, not measurements.  The first key derivation fed the high words of seed and step into the second
hash word only, so that masks of steps 2^32 apart, or of seeds that differ in bits 32..62 only, shared fields x and y of every quad
(correlation 0.5, z about 500 at this n): those cases failed here and changed ``sqd_drop_key``.

Also: kept values are unbiased to the 16-bit threshold's rounding; ``DropState`` refuses rates whose threshold rounds to never / always
keep; and the teeth of the GPU tier's comparisons, shown once with the restatement standing in for a kernel.
"""
import numpy as np
import pytest
import torch

import fp64_ref as R
from squeezedet_pytorch_amd import ops

N = 1 << 20
RATES = [0.5, 0.2, 0.75]
SEED, STEP = 0x123456789abc, 3
LAGS = [1, 2, 3, 4, 8, 768, 768 * 6]
SEED_BITS = [0, 15, 16, 31, 32, 40, 47, 62]
Z_ONE, Z_MAX, CHI2_BOUND = 5.0, 6.0, 50.0

_KEEP = {}


def _keep(p, seed=SEED, step=STEP):
    """The centred keep indicators (keep - q, float64) of the first N elements of the stream (seed, step) at rate p (computed once)."""
    key = (p, seed, step)
    if key not in _KEEP:
        d = ops.DropState(p, seed, 'cpu', step=step)
        m = ops.dropout_mask_reference(seed, step, d.keep16, d.scale, N)
        assert m.shape == (N,) and set(np.unique(m).tolist()) <= {0.0, float(np.float32(d.scale))}
        _KEEP[key] = (m > 0).astype(np.float64) - (1.0 - p)
    return _KEEP[key]


def _z_product(a, b, p):
    """z-score of sum(a * b) for centred indicators a, b that are independent Bernoulli(q) under the null: each product has mean 0 and
    variance (q (1 - q))^2, and distinct products are uncorrelated."""
    q = 1.0 - p
    return float((a * b).sum() / (q * (1.0 - q) * np.sqrt(a.size)))


@pytest.mark.parametrize('p', RATES)
def test_keep_rate(p):
    q = 1.0 - p
    z = float(_keep(p).sum() / np.sqrt(N * q * (1.0 - q)))
    print(f'p {p}: keep rate z {z:+.2f}')
    assert abs(z) <= Z_ONE


@pytest.mark.parametrize('lag', LAGS)
@pytest.mark.parametrize('p', RATES)
def test_neighbouring_elements_are_independent(p, lag):
    k = _keep(p)
    z = _z_product(k[:-lag], k[lag:], p)
    print(f'p {p} lag {lag}: z {z:+.2f}')
    assert abs(z) <= Z_ONE


@pytest.mark.parametrize('dstep', [1, 1 << 32], ids=['t+1', 't+2^32'])
@pytest.mark.parametrize('p', RATES)
def test_steps_are_independent(p, dstep):
    z = _z_product(_keep(p), _keep(p, step=STEP + dstep), p)
    print(f'p {p} step {STEP} against {STEP} + {dstep}: z {z:+.2f}')
    assert abs(z) <= Z_ONE


@pytest.mark.parametrize('bit', SEED_BITS)
@pytest.mark.parametrize('p', RATES)
def test_seeds_one_bit_apart_are_independent(p, bit):
    z = _z_product(_keep(p), _keep(p, seed=SEED ^ (1 << bit)), p)
    print(f'p {p} seed bit {bit}: z {z:+.2f}')
    assert abs(z) <= Z_ONE


@pytest.mark.parametrize('p', RATES)
def test_keep_rate_of_every_channel_and_pixel(p):
    q = 1.0 - p
    C = 768
    npx = N // C
    k = _keep(p)[:npx * C].reshape(npx, C)
    z_ch = k.sum(0) / np.sqrt(npx * q * (1.0 - q))
    z_px = k.sum(1) / np.sqrt(C * q * (1.0 - q))
    print(f'p {p}: max |z| over {C} channels {np.abs(z_ch).max():.2f}, over {npx} pixels {np.abs(z_px).max():.2f}')
    assert np.abs(z_ch).max() <= Z_MAX and np.abs(z_px).max() <= Z_MAX


@pytest.mark.parametrize('p', RATES)
def test_the_four_fields_of_a_quad_are_jointly_independent(p):
    q = 1.0 - p
    bits = (_keep(p) > 0).astype(np.int64).reshape(-1, 4)
    pattern = bits[:, 0] + 2 * bits[:, 1] + 4 * bits[:, 2] + 8 * bits[:, 3]
    got = np.bincount(pattern, minlength=16).astype(np.float64)
    ones = np.array([bin(i).count('1') for i in range(16)])
    want = (N // 4) * q ** ones * (1.0 - q) ** (4 - ones)
    chi2 = float(((got - want) ** 2 / want).sum())
    print(f'p {p}: chi-square of the 16 quad patterns {chi2:.1f} (15 dof)')
    assert chi2 <= CHI2_BOUND


@pytest.mark.parametrize('p', RATES)
def test_kept_values_are_unbiased(p):
    """E[mask] = keep16 / 65536 * scale is 1 up to the rounding of the 16-bit threshold: half a step of 2^-16, relative to 1 - p."""
    d = ops.DropState(p, 1, 'cpu')
    assert d.keep16 == int(round((1.0 - p) * 65536))
    assert abs(d.keep16 / 65536 * d.scale - 1.0) <= 2.0 ** -17 / (1.0 - p)


def test_dropstate_refuses_rates_whose_threshold_degenerates():
    """A p whose keep16 rounds to 0 would never keep anything while the scale stays finite; a p > 0 whose keep16 rounds to 65536 keeps
    everything but scales it.  p = 0 (keep all, scale 1) stays legal."""
    for p in (1.0 - 2.0 ** -18, 1.0 - 2.0 ** -30, 2.0 ** -18, 1e-9):
        with pytest.raises(ValueError):
            ops.DropState(p, 1, 'cpu')
    for p in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            ops.DropState(p, 1, 'cpu')
    d = ops.DropState(0.0, 1, 'cpu')
    assert (d.keep16, d.scale) == (65536, 1.0)
    for p in (2.0 ** -16, 1.0 - 2.0 ** -16):                # the extreme rates that still have a threshold inside (0, 65536)
        d = ops.DropState(p, 1, 'cpu')
        assert 0 < d.keep16 < 65536


# ---- teeth of the GPU tier's comparisons, the restatement standing in for a kernel ----

def _mask(d, shape, step=None):
    seed, st = d.get()
    n = int(np.prod(shape))
    return torch.from_numpy(ops.dropout_mask_reference(seed, st if step is None else step, d.keep16, d.scale, n)).view(shape)


def test_teeth_window_pitch_and_step():
    """tests/test_dropout_gpu.py compares ``dropped == plain * mask[window]`` bit for bit, mask indexed by the BUFFER's flat element.
    An epilogue that indexed the mask at the window's own pitch N, or drew the mask of step + 1, fails that comparison."""
    B, H, W, N, coff = 3, 5, 17, 80, 8
    d = ops.DropState(0.5, 777, 'cpu', step=11)
    plain = torch.from_numpy(np.random.RandomState(0).standard_normal((B, H, W, N)).astype(np.float32)).clamp_min(0)
    window = _mask(d, (B, H, W, N + 24))[..., coff:coff + N]
    want = plain * window
    assert torch.equal(plain * _mask(d, (B, H, W, N + 24))[..., coff:coff + N], want)
    assert not torch.equal(plain * _mask(d, (B, H, W, N)), want), 'a mask at pitch N passed'
    assert not torch.equal(plain * _mask(d, (B, H, W, N + 24), step=12)[..., coff:coff + N], want), 'the mask of step + 1 passed'


def test_teeth_data_gradient_without_relu_derivative_fails_bar_l():
    """The end-to-end reference of ConvDet's data gradient (fp64_ref.dropped_dgrad: plain gradient * mask * relu'(pre-activation))
    rejects a gradient masked by the dropout mask alone, and accepts the float32 chain of the correct one."""
    B, H, W, C, Ncd = 3, 4, 6, 768, 72
    g = torch.Generator().manual_seed(5)
    dpred = torch.randn(B, H, W, Ncd, generator=g)
    w = torch.randn(Ncd, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    sq = torch.randn(B, H, W, 96, generator=g).clamp_min(0)
    w1 = torch.randn(C, 96, 1, 1, generator=g) * (2.0 / 96) ** 0.5
    pre = R.conv(sq, w1, torch.randn(C, generator=g) * 0.1)
    d = ops.DropState(0.5, 777, 'cpu', step=11)
    mask = _mask(d, (B, H, W, C))
    r, exclude = R.dropped_dgrad(dpred, w, mask, pre, d.scale)
    good = R.bar_l_excluding(r.b32, r, exclude)
    assert good['l_ok'] and good['cap_ok'], good
    no_relu = R.conv(dpred, R.dgrad_weight(w)).b32 * mask
    bad = R.bar_l_excluding(no_relu, r, exclude)
    print(f'correct chain: max err/M {good["l_ratio"]:.2e}; mask alone: {bad["l_ratio"]:.2e} (bar {R.BAR_L:.2e}); excluded {good["excluded"]}')
    assert not bad['l_ok'], bad
