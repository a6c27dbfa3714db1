"""Plain float64 references of the GEMM-type launches (helper module of tests/test_fp64_launches_gpu.py; no project kernels).

Every function runs plain torch ops on the device over NHWC tensors (the stem's image is NCHW, weights are OIHW) and returns a
``Ref(ref64, M, b32)``:

* ``ref64``: the operation in float64;
* ``M``: the same operation in float64 on ``|a|``, ``|b|`` plus ``|bias|`` -- the per-element magnitude that bounds the rounding
  error of any summation order (bar L);
* ``b32``: the same plain chain in float32: the error a correct fp32 kernel is measured against (bar P).

Convolutions are tap-shifted matmuls summed in fixed tap order; fused launches compose stages, propagating the magnitude as
``M_next = |W| * (|h64| + M_h) + |b|`` (ReLU is 1-Lipschitz; a window max moves by at most the largest error in its window).

``emu`` ('bf16' | 'split3') replaces the float32 chain by an emulation of a degraded kernel (bf16-rounded operands, or the
3-product bf16 split ``hi*hi + hi*mid + mid*hi``); only the teeth test uses it.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

F64 = torch.float64
F32 = torch.float32


def assert_full_fp32():
    """The float32 chain must be full fp32 (no TF32 / xf32 fast path): torch's defaults, asserted (not set) here and before every
    reference."""
    assert torch.backends.cuda.matmul.allow_tf32 is False
    assert torch.get_float32_matmul_precision() == 'highest'


assert_full_fp32()


class Ref(NamedTuple):
    ref64: torch.Tensor
    M: torch.Tensor
    b32: torch.Tensor


def _bf16(t):
    return t.to(torch.bfloat16).to(F32)


def _mm(a, b, dtype, emu=None):
    """a @ b in ``dtype``; ``emu``: the degraded float32 products."""
    if emu is None or dtype == F64:
        return a.to(dtype) @ b.to(dtype)
    a = a.to(F32); b = b.to(F32)
    if emu == 'bf16':
        return _bf16(a) @ _bf16(b)
    if emu == 'split3':
        ah, bh = _bf16(a), _bf16(b)
        am, bm = _bf16(a - ah), _bf16(b - bh)
        return ah @ bh + ah @ bm + am @ bh
    raise ValueError(emu)


def _three(fn, emu=None):
    """Run ``fn(dtype, absval, emu)`` as (float64, float64 on magnitudes, float32 chain)."""
    assert_full_fp32()
    return Ref(fn(F64, False, None), fn(F64, True, None), fn(F32, False, emu))


def _cast(t, dtype, absval):
    t = t.to(dtype)
    return t.abs() if absval else t


def _conv_core(x, w, dtype, absval, emu):
    """Stride-1 'same' convolution, NHWC x [B,H,W,C] and OIHW w [N,C,k,k] (k = 1 or 3): sum over taps of shifted matmuls."""
    B, H, W, C = x.shape
    N, Cw, k, _ = w.shape
    assert Cw == C and k in (1, 3)
    x = _cast(x, dtype, absval); w = _cast(w, dtype, absval)
    p = k // 2
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p)) if p else x
    y = None
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, C)
            t = _mm(xs, w[:, :, ky, kx].t(), dtype, emu)
            y = t if y is None else y + t
    return y.view(B, H, W, N)


def conv(x, w, bias=None, relu=False, emu=None):
    """y = conv(x, w) (+ bias) (ReLU), 1x1 or 3x3 pad 1."""
    def f(dtype, absval, e):
        y = _conv_core(x, w, dtype, absval, e)
        if bias is not None:
            y = y + _cast(bias, dtype, absval)
        return y.clamp_min(0) if (relu and not absval) else y
    return _three(f, emu)


def dgrad_weight(w):
    """OIHW weight of the convolution that computes dX from dY (in/out swapped, taps flipped)."""
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


def epilogue(r, prev=None, ymul=None, yscale=1.0, ymask=None, relu=False):
    """The conv launches' epilogue on a Ref: (+= prev) (* ymul) (* yscale) (zero where ymask <= 0) (ReLU).  ``prev``, ``ymul`` and
    ``ymask`` are exact inputs."""
    ref64, M, b32 = r
    if prev is not None:
        ref64 = ref64 + prev.to(F64); M = M + prev.to(F64).abs(); b32 = b32 + prev.to(F32)
    if ymul is not None:
        ref64 = ref64 * ymul.to(F64); M = M * ymul.to(F64).abs(); b32 = b32 * ymul.to(F32)
    if yscale != 1.0:
        ref64 = ref64 * yscale; M = M * abs(yscale); b32 = b32 * F32_scalar(yscale)
    if ymask is not None:
        keep = ymask > 0
        ref64 = torch.where(keep, ref64, 0.0); M = torch.where(keep, M, 0.0); b32 = torch.where(keep, b32, 0.0)
    if relu:
        ref64 = ref64.clamp_min(0); b32 = b32.clamp_min(0)
    return Ref(ref64, M, b32)


def F32_scalar(v):
    return float(torch.tensor(v, dtype=F32))


def relu(r):
    return Ref(r.ref64.clamp_min(0), r.M, r.b32.clamp_min(0))


def cat(rs):
    return Ref(*(torch.cat([r[i] for r in rs], dim=-1) for i in range(3)))


def next_stage(r, w, bias, relu_out=True, emu=None):
    """A 1x1 conv applied to the output of a previous stage: M_next = |W| * (|h64| + M_h) + |b|."""
    ref64 = _conv_core(r.ref64, w, F64, False, None) + bias.to(F64)
    M = _conv_core(r.ref64.abs() + r.M, w, F64, True, None) + bias.to(F64).abs()
    b32 = _conv_core(r.b32, w, F32, False, emu) + bias.to(F32)
    if relu_out:
        ref64 = ref64.clamp_min(0); b32 = b32.clamp_min(0)
    return Ref(ref64, M, b32)


# ---- weight gradient ----

def wgrad(dy, x, taps, emu=None):
    """(dW OIHW [N,C,k,k], db [N]) of a stride-1 conv: dW[n,c,tap] = sum_p dy[p,n] x[p+tap,c], one matmul per tap over the pixel
    axis; db = sum_p dy."""
    B, H, W, N = dy.shape
    C = x.shape[3]
    k = 3 if taps == 9 else 1

    def fw(dtype, absval, e):
        d = _cast(dy, dtype, absval).reshape(-1, N)
        xx = _cast(x, dtype, absval)
        p = k // 2
        xp = torch.nn.functional.pad(xx, (0, 0, p, p, p, p)) if p else xx
        out = torch.empty(N, C, k, k, dtype=dtype, device=dy.device)
        for ky in range(k):
            for kx in range(k):
                out[:, :, ky, kx] = _mm(d.t(), xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, C), dtype, e)
        return out

    def fb(dtype, absval, e):
        d = _cast(dy, dtype, absval).reshape(-1, N)
        if e is not None:
            d = _bf16(d) if e == 'bf16' else _bf16(d) + _bf16(d - _bf16(d))
        return d.sum(0)
    return _three(fw, emu), _three(fb, emu)


def _pixel_blocks(t, blocking):
    """NHWC t [B,H,W,K] -> [nblocks, pixels per block, K] in the weight-gradient kernels' block order (zero padded):
    ``('px', P)``: runs of P consecutive pixels of the flat pixel axis; ``'tile'``: 4x16-pixel groups, image-major, then group row,
    then group column."""
    B, H, W, K = t.shape
    if blocking == 'tile':
        Hg, Wg = -(-H // 4), -(-W // 16)
        t = torch.nn.functional.pad(t, (0, 0, 0, 16 * Wg - W, 0, 4 * Hg - H))
        return t.view(B, Hg, 4, Wg, 16, K).permute(0, 1, 3, 2, 4, 5).reshape(B * Hg * Wg, 64, K)
    P = blocking[1]
    t = t.reshape(-1, K)
    n = t.shape[0]
    return torch.nn.functional.pad(t, (0, 0, 0, -(-n // P) * P - n)).view(-1, P, K)


def _in_order(parts, S, acc_out):
    """Step partials [nb, steps, ...] of the pixel blocks -> the S slabs: slab s adds the steps of blocks s, s + S, s + 2S, ... one by one
    in that order (fp32), accumulated into ``acc_out`` [S, ...]."""
    nb = parts.shape[0]
    parts = torch.nn.functional.pad(parts.reshape(nb, -1), (0, 0, 0, -(-nb // S) * S - nb)).view(-1, S, *parts.shape[1:])
    for r in range(parts.shape[0]):
        for j in range(parts.shape[2]):
            acc_out += parts[r, :, j]           # (a zero pad block adds exactly 0)
    return acc_out


def _reduce_slabs(slabs):
    """The shipped slab reduction (wgrad_reduce_batched): partition p = 0..3 sums slabs p, p + 4, ... in ascending order, then the four
    partitions are added 0, 1, 2, 3."""
    S = slabs.shape[0]
    parts = []
    for p in range(4):
        acc = torch.zeros_like(slabs[0])
        for k in range(p, S, 4):
            acc += slabs[k]
        parts.append(acc)
    return ((parts[0] + parts[1]) + parts[2]) + parts[3]


def wgrad_split_k(dy, x, taps, S, blocking, step, emu=None):
    """Float32 restatement of a split-K weight-gradient kernel with its own summation structure: the pixel axis cut into the kernel's
    blocks, slab s accumulating blocks s, s + S, ... in order, ``step`` pixels (one matrix-core K step) per fp32 accumulation, the S
    slabs reduced in the shipped order.  -> (dW [N,C,k,k], db [N]) in float32 (``emu``: degraded products, as ``wgrad``)."""
    assert_full_fp32()
    B, H, W, N = dy.shape
    C = x.shape[3]
    k = 3 if taps == 9 else 1
    p = k // 2
    d = dy.to(F32)
    db_in = d if emu is None else (_bf16(d) if emu == 'bf16' else _bf16(d) + _bf16(d - _bf16(d)))
    dyb = _pixel_blocks(d, blocking)
    nb, PB = dyb.shape[:2]
    dyb = dyb.view(nb, PB // step, step, N)
    xp = torch.nn.functional.pad(x.to(F32), (0, 0, p, p, p, p)) if p else x.to(F32)
    slabs_w = torch.zeros(S, N, C, k, k, dtype=F32, device=dy.device)
    chunk = max(1, (1 << 26) // (S * PB // step * N * C)) * S      # blocks per matmul batch (a multiple of S: slab order is kept)
    for ky in range(k):
        for kx in range(k):
            xb = _pixel_blocks(xp[:, ky:ky + H, kx:kx + W, :], blocking).view(nb, PB // step, step, C)
            acc = torch.zeros(S, N, C, dtype=F32, device=dy.device)
            for b0 in range(0, nb, chunk):
                _in_order(_mm(dyb[b0:b0 + chunk].transpose(2, 3), xb[b0:b0 + chunk], F32, emu), S, acc)
            slabs_w[:, :, :, ky, kx] = acc
    dbb = _pixel_blocks(db_in, blocking).view(nb, PB // step, step, N).sum(2)
    slabs_b = _in_order(dbb, S, torch.zeros(S, N, dtype=F32, device=dy.device))
    return _reduce_slabs(slabs_w), _reduce_slabs(slabs_b)


def wgrad_wino_magnitude(dy, x):
    """Bar L's magnitude for a Winograd F(2x2,3x3) weight gradient: the transforms mix every position of a 4x4 input tile with every
    position of its 2x2 output tile, so the rounding error of any tap of (n, c) is bounded by sum_p |dy[p,n]| |x[p+s,c]| over all 25
    offsets s in [-2, 2]^2, not by that tap's own sum.  -> [N,C,3,3] (the same value on the nine taps)."""
    B, H, W, N = dy.shape
    C = x.shape[3]
    d = dy.to(F64).abs().reshape(-1, N)
    xp = torch.nn.functional.pad(x.to(F64).abs(), (0, 0, 2, 2, 2, 2))
    m = torch.zeros(N, C, dtype=F64, device=dy.device)
    for ky in range(5):
        for kx in range(5):
            m += d.t() @ xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, C)
    return m.view(N, C, 1, 1).expand(N, C, 3, 3).contiguous()


# ---- stem, max pool ----

def _stem_core(img, w, dtype, absval, emu):
    """conv(3 -> N, k, stride 2, pad k // 2) of an NCHW image -> NHWC."""
    B, _, H, W = img.shape
    N, _, k, _ = w.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // 2 + 1, (W + 2 * p - k) // 2 + 1
    x = _cast(img, dtype, absval).permute(0, 2, 3, 1)
    x = torch.nn.functional.pad(x, (0, 0, p, p, p, p))
    w = _cast(w, dtype, absval)
    y = None
    for ky in range(k):
        for kx in range(k):
            xs = x[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :].reshape(-1, 3)
            t = _mm(xs, w[:, :, ky, kx].t(), dtype, emu)
            y = t if y is None else y + t
    return y.view(B, Ho, Wo, N)


def stem(img, w, bias, emu=None):
    """relu(conv(img, w, stride 2) + bias), NHWC."""
    def f(dtype, absval, e):
        y = _stem_core(img, w, dtype, absval, e) + _cast(bias, dtype, absval)
        return y if absval else y.clamp_min(0)
    return _three(f, emu)


def pool_out_size(H, W):
    return (H - 3 + 1) // 2 + 1, (W - 3 + 1) // 2 + 1


def _pool_max(x):
    """MaxPool2d(3, 2, ceil_mode=True) values of an NHWC tensor (no padding on the leading edges; ceil windows are clipped)."""
    B, H, W, C = x.shape
    Ho, Wo = pool_out_size(H, W)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 2 * Ho + 1 - H, 0, 2 * Wo + 1 - W), value=float('-inf'))
    y = None
    for ky in range(3):
        for kx in range(3):
            t = xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :]
            y = t if y is None else torch.maximum(y, t)
    return y


def maxpool(r):
    """Max pool of a stage output: values from ref64 / b32, magnitude = the largest M in the window."""
    return Ref(_pool_max(r.ref64), _pool_max(r.M), _pool_max(r.b32))


def maxpool_exact(x):
    """The max pool of an fp32 tensor, exact (what a pool kernel that does no arithmetic must reproduce bit for bit)."""
    return _pool_max(x)


def _pool_route(dy, codes, H, W):
    """dx[b,iy,ix,c] = sum of dy over the windows whose code selects (iy, ix) (code = tap 0..8 of the 3x3 window, 15 = none), in
    window order (oy, then ox, ascending)."""
    B, Ho, Wo, C = dy.shape
    dx = torch.zeros(B, 2 * Ho + 1, 2 * Wo + 1, C, dtype=dy.dtype, device=dy.device)
    codes = codes.to(torch.int16)
    for ky in range(3):
        for kx in range(3):
            sel = torch.where(codes == ky * 3 + kx, dy, torch.zeros((), dtype=dy.dtype, device=dy.device))
            dx[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :] += sel
    return dx[:, :H, :W, :].contiguous()


def maxpool_bwd(dy, codes, in_hw, emu=None):
    """Max-pool backward routed by the codes the kernel under test wrote."""
    H, W = in_hw

    def f(dtype, absval, e):
        d = _cast(dy, dtype, absval)
        if e is not None:
            d = _bf16(d) if e == 'bf16' else _bf16(d) + _bf16(d - _bf16(d))
        return _pool_route(d, codes, H, W)
    return _three(f, emu)


def stem_wgrad_pooled(dpool, codes, img, N, k, emu=None):
    """Stem (dW [N,3,k,k], db [N]) when the forward ran conv + ReLU + pool fused: the pool's codes route dpool back to the stem
    output (code 15 carries the ReLU mask), then dW[n,c,ky,kx] = sum_p dstem[p,n] img[c, 2p + (ky,kx) - pad]."""
    B, _, Hs, Ws = img.shape
    p = k // 2
    Ho, Wo = (Hs + 2 * p - k) // 2 + 1, (Ws + 2 * p - k) // 2 + 1

    def fw(dtype, absval, e):
        d = _pool_route(_cast(dpool, dtype, absval), codes, Ho, Wo).reshape(-1, N)
        x = torch.nn.functional.pad(_cast(img, dtype, absval).permute(0, 2, 3, 1), (0, 0, p, p, p, p))
        out = torch.empty(N, 3, k, k, dtype=dtype, device=dpool.device)
        for ky in range(k):
            for kx in range(k):
                out[:, :, ky, kx] = _mm(d.t(), x[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2, :].reshape(-1, 3), dtype, e)
        return out

    def fb(dtype, absval, e):
        return _pool_route(_cast(dpool, dtype, absval), codes, Ho, Wo).reshape(-1, N).sum(0)
    return _three(fw, emu), _three(fb, emu)


# ---- fused forward launches ----

def fire_expand(x, w1, b1, w3, b3, emu=None):
    """cat(relu(expand1x1(x)), relu(expand3x3(x)))."""
    return cat([conv(x, w1, b1, relu=True, emu=emu), conv(x, w3, b3, relu=True, emu=emu)])


def fire_bridge(x, w1, b1, w3, b3, wsq, bsq, emu=None):
    """-> (the next squeeze's output, the expand output)."""
    e = fire_expand(x, w1, b1, w3, b3, emu)
    return next_stage(e, wsq, bsq, emu=emu), e


def fire_pool_bridge(x, w1, b1, w3, b3, wsq, bsq, emu=None):
    """-> (the next squeeze's output on the pooled map, the pooled expand output)."""
    p = maxpool(fire_expand(x, w1, b1, w3, b3, emu))
    return next_stage(p, wsq, bsq, emu=emu), p


def stem_pool(img, w, b, emu=None):
    return maxpool(stem(img, w, b, emu))


def stem_pool_squeeze(img, w, b, wsq, bsq, emu=None):
    """-> (the squeeze output, the pooled stem output)."""
    p = stem_pool(img, w, b, emu)
    return next_stage(p, wsq, bsq, emu=emu), p


# ---- the two bars ----

BAR_L = 2.0 ** -18
FLOOR = 2.0 ** -24


def _rms(t):
    return float(t.double().pow(2).mean().sqrt()) if t.numel() else 0.0


def blocks(t, kind):
    """The 64-channel blocks of an output: activations [..., N] by 64 output channels; weight gradients [N, C, k, k] by
    (64 out x 64 in); vectors as one block."""
    if kind == 'act':
        N = t.shape[-1]
        return [t[..., i:i + 64] for i in range(0, N, 64)]
    if kind == 'wgrad':
        N, C = t.shape[:2]
        return [t[i:i + 64, j:j + 64] for i in range(0, N, 64) for j in range(0, C, 64)]
    return []


def bars(got, r, kind, k):
    """Bar L and bar P of one output against its Ref.  -> dict(l_ratio = max err/M, l_ok, p_block = max over blocks of
    rms(err) / max(rms(err32), floor), p_tensor = max|err| / max(max|err32|, floor), p_ok, ...)."""
    got = got.double()
    ref64, M = r.ref64, r.M
    err = got - ref64
    err32 = r.b32.double() - ref64
    aerr = err.abs()
    l_ok = bool((aerr <= BAR_L * M).all())
    pos = M > 0
    l_ratio = float((aerr[pos] / M[pos]).max()) if bool(pos.any()) else 0.0
    exact_zero_ok = bool((aerr[~pos] == 0).all())
    pb = 0.0
    for eb, e32b, rb in zip(blocks(err, kind), blocks(err32, kind), blocks(ref64, kind)):
        den = max(_rms(e32b), FLOOR * _rms(rb))
        num = _rms(eb)
        pb = max(pb, num / den if den > 0 else (0.0 if num == 0 else float('inf')))
    den = max(float(err32.abs().max()), FLOOR * _rms(ref64))
    num = float(aerr.max())
    pt = num / den if den > 0 else (0.0 if num == 0 else float('inf'))
    p_ok = pb <= k and pt <= 2 * k
    return dict(l_ratio=l_ratio, l_ok=l_ok and exact_zero_ok, p_block=pb, p_tensor=pt, p_ok=p_ok, k=k)
