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


def _conv_core(x, w, dtype, absval, emu, chain_kc=None):
    """Stride-1 'same' convolution, NHWC x [B,H,W,C] and OIHW w [N,C,k,k] (k = 1 or 3): sum over taps of shifted matmuls.
    ``chain_kc`` (float32 chain only): the direct kernels' own summation structure instead (``_conv_chain``)."""
    B, H, W, C = x.shape
    N, Cw, k, _ = w.shape
    assert Cw == C and k in (1, 3)
    x = _cast(x, dtype, absval); w = _cast(w, dtype, absval)
    p = k // 2
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p)) if p else x
    if chain_kc is not None and dtype == F32 and not absval:
        return _conv_chain(xp, w, H, W, k, chain_kc, emu)
    y = None
    for ky in range(k):
        for kx in range(k):
            xs = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, C)
            t = _mm(xs, w[:, :, ky, kx].t(), dtype, emu)
            y = t if y is None else y + t
    return y.view(B, H, W, N)


def _conv_chain(xp, w, H, W, k, kc, emu):
    """The float32 chain of the direct kernels (csrc/conv_igemm.hip: conv_igemm, conv_dma, conv_ws, fire_expand): ONE fp32 accumulator
    per output over input-channel chunks of ``kc``, inside a chunk over the taps, inside a tap over matrix-core steps of 4 channels
    (the 4 products of a step as one fp32 dot).  On a 3x3 layer one chain of 9 C / 4 additions errs 2-5x more than nine chains of
    C / 4 summed afterwards (the per-tap matmuls of the plain chain); on a 1x1 layer the two differ only where the matmul library picks
    another algorithm than the sequential one (it does for a few pixels: 3x3 grids at batch 1).  xp: the padded float32 input;
    ``emu``: the degraded products."""
    B, C = xp.shape[0], xp.shape[3]
    N = w.shape[0]

    acc = torch.zeros(B * H * W, N, dtype=F32, device=xp.device)
    for c0 in range(0, C, kc):
        for ky in range(k):
            for kx in range(k):
                for c in range(c0, min(c0 + kc, C), 4):
                    acc = acc + _mm(xp[:, ky:ky + H, kx:kx + W, c:c + 4].reshape(-1, min(4, C - c)), w[:, c:c + 4, ky, kx].t(), F32, emu)
    return acc.view(B, H, W, N)


def conv(x, w, bias=None, relu=False, emu=None, chain_kc=None):
    """y = conv(x, w) (+ bias) (ReLU), 1x1 or 3x3 pad 1.  ``chain_kc``: b32 restates the direct kernels' single accumulator
    (``_conv_core``); ref64 and M do not depend on it."""
    def f(dtype, absval, e):
        y = _conv_core(x, w, dtype, absval, e, chain_kc)
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


# ---- ConvDet's data gradient behind a live dropout, end to end ----

DROP_EXCLUDE_CAP = 0.005      # at most this fraction of the tensor may sit on the ReLU's edge (see ``dropped_dgrad``)


def dropped_dgrad(dpred, w_convdet, mask, pre, scale):
    """The gradient that leaves ConvDet towards the last Fire when the dropout in front of ConvDet is live, from first principles:
    (plain float64 data gradient of ``dpred``) * ``mask`` (the scaled keep mask, as the stand-alone kernel draws it) * relu'(pre),
    ``pre`` = Ref of the last Fire's PRE-activation expand output, recomputed in float64 -- not the dropped tensor the kernels use in
    its place.  -> (Ref with M = the plain data gradient's magnitude times ``scale`` = 1 / (1 - p), b32 = the plain chain times mask
    times relu'; exclude: the elements whose float64 pre-activation is within BAR_L * its own magnitude of zero, where a correct fp32
    forward may land on either side of the ReLU)."""
    r = conv(dpred, dgrad_weight(w_convdet))
    act = pre.ref64 > 0
    m64 = mask.to(F64)
    ref64 = torch.where(act, r.ref64 * m64, 0.0)
    b32 = torch.where(act, r.b32 * mask.to(F32), 0.0)
    exclude = pre.ref64.abs() <= BAR_L * pre.M
    return Ref(ref64, r.M * float(scale), b32), exclude


def bar_l_excluding(got, r, exclude):
    """Bar L of ``got`` against ``r`` on the elements outside ``exclude`` -> dict(l_ratio, l_ok, excluded, cap_ok): ``cap_ok`` = no more
    than DROP_EXCLUDE_CAP of the tensor is excluded."""
    err = (got.double() - r.ref64).abs()
    keep = ~exclude
    ok = bool((err[keep] <= BAR_L * r.M[keep]).all())
    pos = keep & (r.M > 0)
    ratio = float((err[pos] / r.M[pos]).max()) if bool(pos.any()) else 0.0
    n = int(exclude.sum())
    return dict(l_ratio=ratio, l_ok=ok, excluded=n, cap_ok=n <= DROP_EXCLUDE_CAP * exclude.numel())


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


def _reduce_slabs_ascending(slabs):
    """The row reduction of a padded ConvDet (wgrad_reduce_rows): one fp32 accumulator takes the slabs 0, 1, ... in ascending order."""
    acc = torch.zeros_like(slabs[0])
    for k in range(slabs.shape[0]):
        acc += slabs[k]
    return acc


def wgrad_split_k(dy, x, taps, S, blocking, step, emu=None, order='batched'):
    """Float32 restatement of a split-K weight-gradient kernel with its own summation structure: the pixel axis cut into the kernel's
    blocks, slab s accumulating blocks s, s + S, ... in order, ``step`` pixels (one matrix-core K step) per fp32 accumulation, the S
    slabs reduced in the shipped order (``order``: 'batched' = wgrad_reduce_batched's four partitions, 'ascending' = wgrad_reduce_rows').
    -> (dW [N,C,k,k], db [N]) in float32 (``emu``: degraded products, as ``wgrad``)."""
    red = {'batched': _reduce_slabs, 'ascending': _reduce_slabs_ascending}[order]
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
    return red(slabs_w), red(slabs_b)


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
    xp = torch.nn.functional.pad(x, (0, 0, 0, 2 * Wo + 1 - W, 0, 2 * Ho + 1 - H), value=float('-inf'))
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

def fire_expand(x, w1, b1, w3, b3, emu=None, chain_kc=None):
    """cat(relu(expand1x1(x)), relu(expand3x3(x))).  ``chain_kc``: the one-launch direct form (``ops.fire_expand``), which accumulates
    like the direct kernels (its 1x1 half runs the centre tap only)."""
    return cat([conv(x, w1, b1, relu=True, emu=emu, chain_kc=chain_kc), conv(x, w3, b3, relu=True, emu=emu, chain_kc=chain_kc)])


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
    (64 out x 64 in); a loss gradient [B, A, C+5] by class logits / conf / deltas; vectors as one block."""
    if kind == 'act':
        N = t.shape[-1]
        return [t[..., i:i + 64] for i in range(0, N, 64)]
    if kind == 'wgrad':
        N, C = t.shape[:2]
        return [t[i:i + 64, j:j + 64] for i in range(0, N, 64) for j in range(0, C, 64)]
    if kind == 'dpred':
        C = t.shape[-1] - 5
        return [t[..., :C], t[..., C:C + 1], t[..., C + 1:]]
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


def _finite(t):
    return torch.where(torch.isnan(t), torch.zeros((), dtype=t.dtype, device=t.device), t)


def bars_nan(got, r, kind, k):
    """``bars`` for outputs that hold NaN by design (an image with n_obj = 0 or n_obj = A): the NaN positions of ``got`` must equal
    those of ref64 (``nan_ok``); the bars then run on the other elements (NaN positions count as exact)."""
    nan = torch.isnan(r.ref64)
    nan_ok = bool(torch.equal(torch.isnan(got.double()), nan))
    keep = lambda t: torch.where(nan, torch.zeros((), dtype=t.dtype, device=t.device), t)    # noqa: E731
    b = bars(keep(got.double()), Ref(keep(r.ref64), keep(r.M), keep(_finite(r.b32.double()))), kind, k)
    b['nan_ok'] = nan_ok
    b['l_ok'] = b['l_ok'] and nan_ok
    return b


# ---- multi-task loss: forward, analytic backward ----

class _V(NamedTuple):
    """A float64 value and its running error bound M: a float32 evaluation of the same chain errs by about 2^-24 M at most (to first
    order; exact float32 inputs carry M = 0, every rounded operation adds |result|).  This is the magnitude of bar L for the loss: the
    plain chain on absolute values multiplies sums of coordinates (|x2| + |x1| for a 10-pixel width at x = 90) through areas and the
    squared IoU denominator, and left the IoU gradient's bar 10^3 - 10^6 times wider than the gradient itself."""
    v: torch.Tensor
    m: torch.Tensor


# a float32 exp / sigmoid flushes below 2^-126: an absolute floor under their bound keeps that error inside bar L
_TINY = 2.0 ** -100
# rounding depth of a sum over the anchors of an image (the kernel: a strided serial run per thread, a 64-lane tree, 4 waves, 16 parts
# in order) and over the images of a batch (a strided run per lane, a 64-lane tree)
SUM_DEPTH_A = 32
SUM_DEPTH_B = 16


def _c(x):
    return _V(x, 0.0 * abs(x))


def _lf(t):
    t = t.to(F64)
    return _V(t, torch.zeros_like(t))


def _add(a, b):
    v = a.v + b.v
    return _V(v, a.m + b.m + v.abs())


def _sub(a, b):
    v = a.v - b.v
    return _V(v, a.m + b.m + v.abs())


def _mul(a, b):
    v = a.v * b.v
    return _V(v, a.m * abs(b.v) + abs(a.v) * b.m + v.abs())


def _div(a, b):
    v = a.v / b.v
    return _V(v, (a.m + v.abs() * b.m) / abs(b.v) + v.abs())


def _neg(a):
    return _V(-a.v, a.m)


def _exp(a):
    v = torch.exp(a.v)
    return _V(v, v * (1 + a.m) + _TINY)


def _log(a):
    v = torch.log(a.v)
    return _V(v, v.abs() + a.m / a.v.abs())


def _sel(w, a):
    """A branch weight (an exact 0, 0.5 or 1) times a chain value; a cut branch is a selection, as in torch's backward (a NaN upstream
    stays out of it)."""
    w = w.to(F64)
    z = torch.zeros((), dtype=F64)
    return _V(torch.where(w == 0, z, w * a.v), torch.where(w == 0, z, w.abs() * a.m))


def _sum(a, dim, depth):
    return _V(a.v.sum(dim), a.m.sum(dim) + depth * a.v.abs().sum(dim))


LOSS_MUTANTS = ('clamp_exclusive', 'no_tie_split', 'clamp_min_strict', 'iou_detached', 'neg_den_A')


def _decode32(pred, anchors, C):
    """The kernel's box decode in float32 on the host, op for op (no contraction): -> x1u, y1u, x2u, y2u."""
    d = pred[..., C + 1:].to(F32)
    an = anchors.to(F32)
    ax, ay, aw, ah = an[:, 0], an[:, 1], an[:, 2], an[:, 3]
    cx = ax + aw * d[..., 0]
    cy = ay + ah * d[..., 1]
    w = aw * torch.exp(d[..., 2])
    h = ah * torch.exp(d[..., 3])
    hw, hh = 0.5 * (w - 1.0), 0.5 * (h - 1.0)
    return cx - hw, cy - hh, cx + hw, cy + hh


def _branches(x1u, y1u, x2u, y2u, gt, wmax, hmax, mutant=None):
    """The 10 branch weights of the IoU gradient of each anchor, from one precision's unclamped box (torch 2.10's conventions: clamp
    passes inclusively at its bounds, min / max ties split 0.5 / 0.5, clamp_min passes at 0) -> dict of [B, A] float64 weights."""
    dt = x1u.dtype
    t = lambda v: torch.tensor(v, dtype=dt)   # noqa: E731

    def clamp_pass(x, hi):
        if mutant == 'clamp_exclusive':
            return (x > 0) & (x < hi)
        return (x >= 0) & (x <= hi)

    def tie_min(mine, other):
        if mutant == 'no_tie_split':
            return (mine <= other).to(F64)
        return (mine < other).to(F64) + 0.5 * (mine == other).to(F64)

    def tie_max(mine, other):
        if mutant == 'no_tie_split':
            return (mine >= other).to(F64)
        return (mine > other).to(F64) + 0.5 * (mine == other).to(F64)

    wm, hm = t(wmax), t(hmax)
    px1, py1 = x1u.clamp(0, wm), y1u.clamp(0, hm)
    px2, py2 = x2u.clamp(0, wm), y2u.clamp(0, hm)
    g = gt[..., 1:5].to(dt)
    gx1, gy1, gx2, gy2 = g.unbind(-1)
    lr_raw = torch.minimum(gx2, px2) - torch.maximum(gx1, px1)
    tb_raw = torch.minimum(gy2, py2) - torch.maximum(gy1, py1)
    strict = mutant == 'clamp_min_strict'
    return dict(cx1=clamp_pass(x1u, wm).to(F64), cx2=clamp_pass(x2u, wm).to(F64), cy1=clamp_pass(y1u, hm).to(F64),
                cy2=clamp_pass(y2u, hm).to(F64), minx=tie_min(px2, gx2), maxx=tie_max(px1, gx1), miny=tie_min(py2, gy2), maxy=tie_max(py1, gy1),
                plr=((lr_raw > 0) if strict else (lr_raw >= 0)).to(F64), ptb=((tb_raw > 0) if strict else (tb_raw >= 0)).to(F64))


def _loss_chain(pred, gt, anchors, input_size, C, weights, u, br, mutant=None):
    """The loss and its analytic gradient in the V algebra (float64 values + magnitudes), on the host, with given branch weights ``br``.
    ``u`` = [3, B] upstream gradients of (class, score, bbox).  -> (terms [4, B, A] V, nobj [B], dpred V [B, A, C+5])."""
    p = pred.to(F64)
    g = gt.to(F64)
    an = anchors.to(F32).to(F64)
    B, A = p.shape[:2]
    wmax, hmax = float(input_size[1] - 1), float(input_size[0] - 1)
    w_c, w_p, w_n, w_b = (float(torch.tensor(w, dtype=F32)) for w in weights)
    mask = g[..., 0]
    onehot = g[..., 9:]
    # class: log-softmax
    mx = p[..., :C].max(-1, keepdim=True)[0]
    zc = _sub(_lf(p[..., :C]), _lf(mx))
    e = _exp(zc)
    s = _sum(e, -1, C)
    lse = _log(s)
    logp = _sub(zc, _V(lse.v.unsqueeze(-1), lse.m.unsqueeze(-1)))
    ce = _sum(_mul(_lf(onehot), _neg(logp)), -1, C)
    prob = _div(e, _V(s.v.unsqueeze(-1), s.m.unsqueeze(-1)))
    ohs = onehot.sum(-1)
    # confidence: 1 / (1 + exp(-z))
    conf = _div(_c(1.0), _add(_c(1.0), _exp(_neg(_lf(p[..., C])))))
    # decode
    d = [_lf(p[..., C + 1 + j]) for j in range(4)]
    ax, ay, aw, ah = (_lf(an[:, j]) for j in range(4))
    cx, cy = _add(ax, _mul(aw, d[0])), _add(ay, _mul(ah, d[1]))
    w, h = _mul(aw, _exp(d[2])), _mul(ah, _exp(d[3]))
    hw, hh = _mul(_c(0.5), _sub(w, _c(1.0))), _mul(_c(0.5), _sub(h, _c(1.0)))
    x1u, y1u, x2u, y2u = _sub(cx, hw), _sub(cy, hh), _add(cx, hw), _add(cy, hh)
    clampv = lambda a, hi: _V(a.v.clamp(0, hi), a.m)          # noqa: E731
    px1, py1, px2, py2 = clampv(x1u, wmax), clampv(y1u, hmax), clampv(x2u, wmax), clampv(y2u, hmax)
    gx1, gy1, gx2, gy2 = (_lf(g[..., 1 + j]) for j in range(4))
    vmin = lambda a, b: _V(torch.minimum(a.v, b.v), torch.maximum(a.m, b.m))    # noqa: E731
    vmax = lambda a, b: _V(torch.maximum(a.v, b.v), torch.maximum(a.m, b.m))    # noqa: E731
    lr_raw = _sub(vmin(gx2, px2), vmax(gx1, px1))
    tb_raw = _sub(vmin(gy2, py2), vmax(gy1, py1))
    lr, tb = _V(lr_raw.v.clamp_min(0), lr_raw.m), _V(tb_raw.v.clamp_min(0), tb_raw.m)
    inter = _mul(lr, tb)
    pw, ph = _sub(px2, px1), _sub(py2, py1)
    uni = _sub(_add(_mul(_sub(gx2, gx1), _sub(gy2, gy1)), _mul(pw, ph)), inter)
    den = _add(uni, _c(float(torch.tensor(1e-10, dtype=F32))))
    iou = _div(inter, den)
    mk = _lf(mask)
    ee = _sub(_mul(iou, mk), conf)
    bbd = [_sub(d[j], _lf(g[..., 5 + j])) for j in range(4)]
    bb = _add(_add(_mul(bbd[0], bbd[0]), _mul(bbd[1], bbd[1])), _add(_mul(bbd[2], bbd[2]), _mul(bbd[3], bbd[3])))
    e2 = _mul(ee, ee)
    omk = _sub(_c(1.0), mk)
    terms = [_mul(mk, ce), _mul(mk, e2), _mul(omk, e2), _mul(mk, bb)]
    nobj = mask.sum(1)
    n = _lf(nobj.unsqueeze(1))                                     # (exact: a count below 2^24)
    an_ = nobj.new_full((B, 1), float(A))
    nneg = _lf(an_ if mutant == 'neg_den_A' else an_ - nobj.unsqueeze(1))
    # backward, the upstream gradient per image and component
    uu = u.to(F64).view(3, B, 1).expand(3, B, A)
    uc, us, ub = (_V(uu[j], uu[j].abs()) for j in range(3))         # (gmean / B rounds once)
    kc = _div(_mul(_mul(uc, _c(w_c)), mk), n)
    kcx = _V(kc.v.unsqueeze(-1), kc.m.unsqueeze(-1))
    o_cls = _mul(kcx, _sub(_mul(_lf(ohs.unsqueeze(-1).expand_as(onehot)), prob), _lf(onehot)))
    k = _mul(us, _add(_div(_mul(_c(w_p), mk), n), _div(_mul(_c(w_n), omk), nneg)))
    dL_de = _mul(_mul(_c(2.0), k), ee)
    o_conf = _neg(_mul(_mul(dL_de, conf), _sub(_c(1.0), conf)))
    dL_dov = _mul(dL_de, mk)
    den2 = _mul(den, den)
    dov_dinter = _add(_div(_c(1.0), den), _div(inter, den2))
    dov_dap = _neg(_div(inter, den2))
    dlr = _sel(br['plr'], _mul(_mul(dL_dov, dov_dinter), tb))
    dtb = _sel(br['ptb'], _mul(_mul(dL_dov, dov_dinter), lr))
    dap = _mul(dL_dov, dov_dap)
    dpx2 = _sel(br['cx2'], _add(_sel(br['minx'], dlr), _mul(dap, ph)))
    dpx1 = _sel(br['cx1'], _sub(_neg(_sel(br['maxx'], dlr)), _mul(dap, ph)))
    dpy2 = _sel(br['cy2'], _add(_sel(br['miny'], dtb), _mul(dap, pw)))
    dpy1 = _sel(br['cy1'], _sub(_neg(_sel(br['maxy'], dtb)), _mul(dap, pw)))
    gd = [_mul(_add(dpx1, dpx2), aw), _mul(_add(dpy1, dpy2), ah),
          _mul(_mul(_sub(dpx2, dpx1), _c(0.5)), w), _mul(_mul(_sub(dpy2, dpy1), _c(0.5)), h)]
    if mutant == 'iou_detached':
        gd = [_V(torch.zeros_like(x.v), torch.zeros_like(x.m)) for x in gd]
    kb = _mul(_div(_mul(_mul(ub, _c(w_b)), mk), n), _c(2.0))
    o_d = [_add(gd[j], _mul(kb, bbd[j])) for j in range(4)]
    dp = _V(torch.cat([o_cls.v, o_conf.v.unsqueeze(-1)] + [x.v.unsqueeze(-1) for x in o_d], -1),
            torch.cat([o_cls.m, o_conf.m.unsqueeze(-1)] + [x.m.unsqueeze(-1) for x in o_d], -1))
    # per-image losses
    S = [_sum(t, 1, SUM_DEPTH_A) for t in terms]
    n1 = _lf(nobj)
    nneg1 = _V(nneg.v[:, 0], nneg.m[:, 0])
    cls = _div(_mul(_c(w_c), S[0]), n1)
    pos = _div(_mul(_c(w_p), S[1]), n1)
    neg = _div(_mul(_c(w_n), S[2]), nneg1)
    bbx = _div(_mul(_c(w_b), S[3]), n1)
    losses = [cls, _add(pos, neg), bbx, _add(_add(_add(cls, pos), neg), bbx)]
    losses = _V(torch.stack([x.v for x in losses]), torch.stack([x.m for x in losses]))
    return losses, nobj, dp, (x1u.v, y1u.v, x2u.v, y2u.v)


def _oracle_loss(pred, gt, anchors, input_size, C, weights, dtype, coef=None, gmean=None):
    """oracle.multitask_loss in ``dtype`` on the host (anchors rounded to float32 as the kernel sees them), with torch autograd for
    the gradient.  -> (losses [4, B], dpred for gmean or None, dpred for coef or None)."""
    import numpy as np
    import oracle
    an = anchors.detach().to(F32).cpu().numpy().astype(np.float32)
    wts = [float(torch.tensor(w, dtype=F32)) for w in weights]
    outs = []
    for up in ('mean', 'coef', 'none'):
        if (up == 'mean' and gmean is None) or (up == 'coef' and coef is None) or (up == 'none' and outs != [None, None]):
            outs.append(None)
            continue
        with torch.enable_grad():                       # (also when called from inside an autograd.Function's forward)
            p = pred.detach().cpu().to(dtype).requires_grad_(True)
            lv, st = oracle.multitask_loss(p, gt.detach().cpu().to(dtype), an, tuple(input_size), C, *wts)
            if up == 'mean':
                (lv.mean() * float(torch.tensor(float(gmean), dtype=F32))).backward()
            elif up == 'coef':
                cf = coef.detach().cpu().to(F32).to(dtype)
                (cf[0] * st['class_loss'] + cf[1] * st['score_loss'] + cf[2] * st['bbox_loss']).sum().backward()
        outs.append((torch.stack([st['class_loss'], st['score_loss'], st['bbox_loss'], lv]).detach(), p.grad))
    lo = next(o[0] for o in outs if o is not None)
    return lo, (outs[0][1] if outs[0] else None), (outs[1][1] if outs[1] else None)


def loss(pred, gt, anchors, input_size, C, weights, gmean=None, coef=None, mutant=None):
    """float64 references of one loss launch pair, on the host.  -> dict:

    * ``losses`` [4, B], ``mean4`` [4]: Ref (ref64: oracle.multitask_loss in float64; M: the chain on magnitudes; b32: the oracle in
      float32);
    * ``nobj`` [B]: exact;
    * ``dmean`` (upstream ``gmean`` at mean(total)) and ``dcoef`` (upstream ``coef`` [3, B] at class / score / bbox): Ref of dpred
      [B, A, C+5] (ref64 by float64 autograd);
    * ``dmean_alt`` / ``dcoef_alt``: the same gradient with every branch taken as a float32 evaluation of the kernel's decode takes
      it; ``flips`` [B, A]: the positive anchors where the two precisions take different branches (either reference is accepted
      there, ``pick``).

    ``mutant`` (one of LOSS_MUTANTS; the CPU teeth only): ref64 from the analytic chain under a wrong convention."""
    assert mutant is None or mutant in LOSS_MUTANTS
    pred, gt, anchors = pred.detach().cpu(), gt.detach().cpu(), anchors.detach().cpu()
    B, A = pred.shape[:2]
    wmax, hmax = float(input_size[1] - 1), float(input_size[0] - 1)
    lo64, dm64, dc64 = _oracle_loss(pred, gt, anchors, input_size, C, weights, F64, coef, gmean)
    lo32, dm32, dc32 = _oracle_loss(pred, gt, anchors, input_size, C, weights, F32, coef, gmean)
    mask = gt[..., 0].to(F64)
    out = {'nobj': mask.sum(1)}
    ups = {}
    if gmean is not None:
        g = float(torch.tensor(float(gmean), dtype=F32)) / B
        ups['dmean'] = (torch.full((3, B), g, dtype=F64), dm64, dm32)
    if coef is not None:
        ups['dcoef'] = (coef.detach().cpu().to(F32).to(F64), dc64, dc32)
    # the branches of float64 and of the kernel's float32 decode
    br64 = _branches(*_box64(pred, anchors, C), gt, wmax, hmax)
    br32 = _branches(*_decode32(pred, anchors, C), gt, wmax, hmax)
    flips = torch.zeros(B, A, dtype=torch.bool)
    for key in br64:
        flips |= (br64[key] != br32[key]) & (mask > 0)
    out['flips'] = flips
    brm = br64 if mutant is None else _branches(*_box64(pred, anchors, C), gt, wmax, hmax, mutant)
    losses = None
    for name, (u, ref64, b32) in ups.items():
        losses, _n, dp, _ = _loss_chain(pred, gt, anchors, input_size, C, weights, u, brm, mutant)
        _l, _n, dp32b, _ = _loss_chain(pred, gt, anchors, input_size, C, weights, u, br32)
        M = torch.where(flips.unsqueeze(-1), torch.maximum(dp.m, dp32b.m), dp.m)
        r64 = dp.v if mutant is not None else ref64
        out[name] = Ref(r64, M, b32)
        out[name + '_alt'] = torch.where(flips.unsqueeze(-1), dp32b.v, r64)
    if losses is None:
        losses = _loss_chain(pred, gt, anchors, input_size, C, weights, torch.zeros(3, B, dtype=F64), brm, mutant)[0]
    l64 = losses.v if mutant is not None else lo64
    out['losses'] = Ref(l64, losses.m, lo32)
    out['mean4'] = Ref(l64.mean(1), (losses.m.sum(1) + SUM_DEPTH_B * losses.v.abs().sum(1)) / B, lo32.mean(1))
    return out


def loss_bf16(pred, gt, anchors, input_size, C, weights, gmean=None, coef=None):
    """The float32 oracle chain on bf16-rounded ``pred`` and ``gt`` (the teeth of bar P) -> (losses [4, B], dpred for gmean, dpred for
    coef)."""
    return _oracle_loss(_bf16(pred.detach().cpu().float()), _bf16(gt.detach().cpu().float()), anchors, input_size, C, weights, F32,
                        coef, gmean)


def _box64(pred, anchors, C):
    """The unclamped box in float64 (the chain's own decode) -> x1u, y1u, x2u, y2u."""
    d = pred[..., C + 1:].to(F64)
    an = anchors.to(F32).to(F64)
    cx = an[:, 0] + an[:, 2] * d[..., 0]
    cy = an[:, 1] + an[:, 3] * d[..., 1]
    w = an[:, 2] * torch.exp(d[..., 2])
    h = an[:, 3] * torch.exp(d[..., 3])
    return cx - 0.5 * (w - 1), cy - 0.5 * (h - 1), cx + 0.5 * (w - 1), cy + 0.5 * (h - 1)


def pick(got, r, alt, flips):
    """dpred Ref with ref64 taken, on each flipped anchor row, from the branch (float64's or float32's) closer to ``got``."""
    got = got.detach().cpu().double()
    e64 = ((got - r.ref64).abs() / r.M.clamp_min(1e-300)).nan_to_num(0.0).amax(-1)
    e32 = ((got - alt).abs() / r.M.clamp_min(1e-300)).nan_to_num(0.0).amax(-1)
    use = flips & (e32 < e64)
    return Ref(torch.where(use.unsqueeze(-1), alt, r.ref64), r.M, r.b32)


# ---- gradient clipping + SGD with momentum ----

def clip_sgd(params, grads, bufs, lr, momentum, wd, max_norm):
    """clip_grad_norm_(max_norm) + torch.optim.SGD(lr, momentum, wd).step() in float64 from float32 snapshots (lists of tensors; bufs: the
    momentum buffers, zero on the first step).  -> (tn64, coef64, [Ref of each new parameter], [Ref of each new buffer]); b32 is None.
    M = |p| + lr (momentum |buf| + coef |g| + wd |p|) for a parameter, the bracket alone for a buffer."""
    g64 = [g.detach().double().cpu() for g in grads]
    tn64 = float(torch.sqrt(sum((g * g).sum() for g in g64)))
    coef = min(1.0, max_norm / (tn64 + 1e-6)) if max_norm > 0 else 1.0
    lr, momentum, wd = (float(torch.tensor(v, dtype=F32)) for v in (lr, momentum, wd))
    ps, bs = [], []
    for p, g, b in zip(params, g64, bufs):
        p = p.detach().double().cpu()
        g = g.reshape(p.shape)
        b = b.detach().double().cpu().reshape(p.shape)
        d = g * coef + wd * p
        nb = momentum * b + d
        mb = momentum * b.abs() + coef * g.abs() + wd * p.abs()
        ps.append(Ref(p - lr * nb, p.abs() + lr * mb, None))
        bs.append(Ref(nb, mb, None))
    return tn64, coef, ps, bs
