"""Thin, shape-checked Python wrappers over the C-ABI kernels (NHWC fp32 device tensors in,
NHWC fp32 device tensors out).  Every wrapper validates operand shapes against what the kernel
and its grid assume *before* launching -- an out-of-bounds access on the GPU can take the node down.

All launches go to the caller's current HIP stream; nothing synchronises.

Layout of the host side: ``tiles`` (which configuration runs a layer: measured table, heuristics, feasibility),
``plans`` (packed / transformed operand copies, slab workspaces), ``timing`` (optional HIP-event brackets) and this
module (marshalling: one function per C-ABI entry point).  Their public names are re-exported here, so callers keep
writing ``ops.choose_cfg`` / ``ops.ConvPlan`` / ``ops.KernelTimer``.
"""
from __future__ import annotations

import ctypes
import functools
import math
import threading
from typing import NamedTuple

import torch

from . import _native as nat
from . import timing
from .timing import KernelTimer, set_timer, _Bracket  # noqa: F401
from . import tiles
from .tiles import *  # noqa: F401,F403
from .tiles import (_tuning, _nearest_tuned, _CFG_DMA, _wino_wgrad_tc)  # noqa: F401
from . import plans
from .plans import (ConvPlan, repack_batched, dgrad_weight, FusedExpandPlan, WinoPlan, repack_wino_batched, FireWinoPlan,  # noqa: F401
                    FireBridgePlan, WgradBatch, wino_sk_schedule, wino_sk_host_schedule)


def _check_nhwc(t, name):
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f'{name} must be a contiguous fp32 CUDA tensor [B,H,W,C], got {tuple(t.shape)} {t.dtype} {t.device}')


class DropState:
    """Device state {seed, step} of the counter-based dropout in front of ConvDet (csrc/sqd_common.h; reference nn.Dropout,
    src/model/squeezedet.py:71-72,81-82) + its rate.  ``keep16`` = round((1 - p) * 65536), ``scale`` = 1 / (1 - p)."""
    __slots__ = ('state', 'p', 'keep16', 'scale')

    def __init__(self, p, seed, device, step=0):
        if not 0.0 <= p < 1.0:
            raise ValueError(f'dropout probability must be in [0, 1), got {p}')
        self.p = float(p)
        self.keep16 = int(round((1.0 - self.p) * 65536))
        self.scale = 1.0 / (1.0 - self.p)
        if self.keep16 == 0 or (self.p > 0.0 and self.keep16 == 65536):
            # the 16-bit threshold cannot express the rate: nothing would ever be kept (at a finite scale), or everything kept but scaled
            raise ValueError(f'dropout probability {p} is not representable: keep threshold round((1 - p) * 65536) = {self.keep16}')
        self.state = torch.tensor([int(seed) & 0x7fffffffffffffff, int(step)], dtype=torch.int64, device=device)

    def get(self):
        """(seed, step) as Python ints (one device-to-host copy: checkpoints, tests)."""
        s = self.state.cpu()
        return int(s[0]), int(s[1])

    def set(self, seed, step):
        self.state.copy_(torch.tensor([int(seed) & 0x7fffffffffffffff, int(step)], dtype=torch.int64))


def dropout_mask(drop, shape):
    """The scaled keep mask of ``drop``'s CURRENT (seed, step) for an NHWC tensor of ``shape`` (numel % 4 == 0), from the stand-alone
    kernel: element e = flat index.  Does not advance the step."""
    n = 1
    for d in shape:
        n *= int(d)
    if n % 4:
        raise ValueError('dropout_mask: number of elements must be a multiple of 4')
    m = torch.empty(shape, device=drop.state.device, dtype=torch.float32)
    br = _Bracket('dropout_mask', f'{n} elements', 0.0, 4.0 * n) if timing._timer is not None else None
    nat.check(nat.lib().sqd_dropout_mask_fwd(nat.ptr(drop.state), drop.keep16, float(drop.scale), nat.ptr(m), n // 4,
                                              nat.stream_handle(m.device)), 'sqd_dropout_mask_fwd')
    if br is not None:
        br.done()
    return m


def dropout_advance(drop):
    """step += 1 on the device (one forward consumed its mask) when no kernel of the forward carried the advance."""
    nat.check(nat.lib().sqd_dropout_advance(nat.ptr(drop.state), nat.stream_handle(drop.state.device)), 'sqd_dropout_advance')


def dropout_mask_reference(seed, step, keep16, scale, n):
    """Host restatement (numpy, uint32 arithmetic) of csrc/sqd_common.h's sqd_drop_mul4 for elements [0, n): what every kernel that
    applies the dropout -- fused epilogue or stand-alone -- must reproduce bit for bit."""
    import numpy as np

    def mix(x):
        x = x.astype(np.uint32)
        x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
        return x
    u = lambda v: np.array([v & 0xffffffff], dtype=np.uint32)
    with np.errstate(over='ignore'):
        s0, s1, t0, t1 = u(seed), u(seed >> 32), u(step), u(step >> 32)
        k0 = mix(s0 ^ mix(t0 ^ mix(s1 ^ mix(t1 + np.uint32(0x9e3779b9)))))      # sqd_drop_key: both words mix all 128 bits
        k1 = mix(t1 ^ mix(s1 ^ mix(t0 ^ mix(s0 + np.uint32(0x85ebca6b)))))
        e4 = np.arange((n + 3) // 4, dtype=np.uint64)
        lo = (e4 & np.uint64(0xffffffff)).astype(np.uint32) ^ ((e4 >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9e3779b9))
        h1 = mix(lo ^ k0)
        h2 = mix(h1 ^ k1)
    f = np.stack([h1 & np.uint32(0xffff), h1 >> np.uint32(16), h2 & np.uint32(0xffff), h2 >> np.uint32(16)], 1).reshape(-1)[:n]
    return np.where(f < np.uint32(keep16), np.float32(scale), np.float32(0.0)).astype(np.float32)


def conv_drop_cfg(C, N, npix):
    """A weight-stationary 1x1 configuration (the family whose epilogue carries the fused dropout) for a C -> N layer: the table's
    choice if it is one, else the widest slice whose weights fit the LDS; None if there is none."""
    hit = choose_cfg(1, C, N, npix)
    if _CFG_DMA.get(hit % 1000, 0) >= 3 and conv_cfg_ok(hit, C):
        return hit
    best = None
    for cid, (taps, kc, px, bn) in cfg_table().items():
        if taps == 1 and _CFG_DMA.get(cid, 0) >= 3 and conv_cfg_ok(cid, C):
            pad = -(-N // bn) * bn / N
            key = (pad, -bn, -(8 if _CFG_DMA[cid] == 4 else 4))
            if best is None or key < best[0]:
                best = (key, cid)
    return None if best is None else best[1]


def conv(x, x_coff, plan, y, y_coff, relu=False, accumulate=False, xmask=None, xmask_coff=0, ymask=None, ymask_coff=0,
         ymul=None, ymul_coff=0, drop=None):
    """y[..., y_coff:y_coff+N] (=|+=) conv(x[..., x_coff:x_coff+C] [* (xmask>0)]) (+bias) (ReLU).  ``drop`` (a DropState; forward
    only, ``plan`` on a weight-stationary 1x1 configuration): counter-based dropout of the output in the epilogue."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    if tuple(y.shape[:3]) != (B, H, W):
        raise ValueError(f'conv: x {tuple(x.shape)} and y {tuple(y.shape)} disagree on B,H,W')
    yp = y.shape[3]
    if x_coff < 0 or x_coff + plan.C > xp or y_coff < 0 or y_coff + plan.N > yp:
        raise ValueError('conv: channel window out of range')
    mp = 0
    if xmask is not None:
        if cfg_is_dma(plan.cfg_id):
            raise ValueError('conv: xmask needs a register-staged configuration')
        _check_nhwc(xmask, 'xmask')
        if tuple(xmask.shape[:3]) != (B, H, W) or xmask_coff + plan.C > xmask.shape[3]:
            raise ValueError('conv: xmask geometry mismatch')
        mp = xmask.shape[3]
    ymp = ylp = 0
    if ymask is not None:
        _check_nhwc(ymask, 'ymask')
        if tuple(ymask.shape[:3]) != (B, H, W) or ymask_coff + plan.N > ymask.shape[3]:
            raise ValueError('conv: ymask geometry mismatch')
        ymp = ymask.shape[3]
    if ymul is not None:
        _check_nhwc(ymul, 'ymul')
        if tuple(ymul.shape[:3]) != (B, H, W) or ymul_coff + plan.N > ymul.shape[3]:
            raise ValueError('conv: ymul geometry mismatch')
        ylp = ymul.shape[3]
    if B * H * W * max(xp, yp) >= 2 ** 40:
        raise ValueError('conv: tensor too large')
    br = None
    if timing._timer is not None:
        npix = B * H * W
        br = _Bracket(cfg_kernel_name(plan.cfg_id),
                      f'{plan.taps}tap C{plan.C} N{plan.N} {H}x{W}', 2.0 * npix * plan.N * plan.C * plan.taps,
                      4.0 * (npix * (plan.C + plan.N) + plan.N * plan.C * plan.taps))
    if drop is not None:
        if accumulate or xmask is not None or ymask is not None or ymul is not None:
            raise ValueError('conv: the fused dropout is a forward-only epilogue')
        rc = nat.lib().sqd_conv_drop_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), B, H, W, plan.C, xp, x_coff, plan.N,
                                         plan.Npad, yp, y_coff, int(relu), nat.ptr(drop.state), drop.keep16, float(drop.scale),
                                         plan.cfg_id, nat.stream_handle(x.device))
        nat.check(rc, 'sqd_conv_drop_fwd')
    else:
        rc = nat.lib().sqd_conv_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), nat.ptr(xmask),
                                    nat.ptr(ymask), nat.ptr(ymul), B, H, W, plan.C, xp, x_coff, plan.N, plan.Npad, yp, y_coff,
                                    int(relu), int(accumulate), mp, xmask_coff, ymp, ymask_coff, ylp, ymul_coff,
                                    plan.cfg_id, nat.stream_handle(x.device))
        nat.check(rc, 'sqd_conv_fwd')
    if br is not None:
        br.done()
    return y


def fire_expand(x, x_coff, fplan, y, y_coff):
    """y[..., y_coff:y_coff+E] = relu(expand1x1(x)), y[..., y_coff+E:y_coff+2E] = relu(expand3x3(x)), one launch."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    if tuple(y.shape[:3]) != (B, H, W):
        raise ValueError('fire_expand: x and y disagree on B,H,W')
    p = fplan.plan
    if x_coff + fplan.C > xp or y_coff + 2 * fplan.E > y.shape[3]:
        raise ValueError('fire_expand: channel window out of range')
    br = _Bracket(cfg_kernel_name(fplan.cfg_id).replace('conv_dma', 'fire_expand'), f'expand C{fplan.C} E{fplan.E} {H}x{W}',
                  2.0 * B * H * W * fplan.E * fplan.C * 10, 4.0 * B * H * W * (fplan.C + 2 * fplan.E)) if timing._timer is not None else None
    rc = nat.lib().sqd_fire_expand_fwd(nat.ptr(x), nat.ptr(p.w), nat.ptr(p.bias), nat.ptr(y), B, H, W, fplan.C, xp, x_coff, fplan.E,
                                       p.Npad, y.shape[3], y_coff, fplan.cfg_id, nat.stream_handle(x.device))
    nat.check(rc, 'sqd_fire_expand_fwd')
    if br is not None:
        br.done()
    return y


class DetKeys:
    """A request to ConvDet's launch: also store the detection key of every anchor (``sqd_conv_wino_vs_keys_fwd``) into ``ws`` -- the
    detect workspace of the batch (``det_workspace_words``; the keys occupy its first B x ceil4(A) words, the arrival counters behind
    them are left alone).  ``written`` tells the caller whether the launch that ran could honour it (three classes, ConvDet on the
    V-shared Winograd kernel writing ``pred`` itself): ``detect(..., keys_ready=True)`` then skips its scoring pass."""
    __slots__ = ('ws', 'score_thresh', 'anchors_per_cell', 'num_classes', 'written')

    def __init__(self, ws, score_thresh, anchors_per_cell, num_classes):
        self.ws, self.score_thresh = ws, float(score_thresh)
        self.anchors_per_cell, self.num_classes = int(anchors_per_cell), int(num_classes)
        self.written = False

    def fits(self, plan, y, y_coff, relu):
        B, H, W, yp = y.shape
        return (self.num_classes == 3 and plan.N == 8 * self.anchors_per_cell and yp == plan.N and y_coff == 0 and not relu
                and self.score_thresh >= 0.0 and isinstance(self.ws, torch.Tensor) and self.ws.dtype == torch.int32
                and self.ws.device == y.device and self.ws.is_contiguous() and self.ws.data_ptr() % 16 == 0
                and self.ws.numel() >= det_workspace_words(B, H * W * self.anchors_per_cell))


class det_keys_request:
    """``with det_keys_request(keys): <ConvDet's launch>``: the ``DetKeys`` request of the calling thread for the ``conv_wino`` launches
    inside the block (None: none).  Out of band on purpose: ConvDet reaches ``conv_wino`` through the same call, with the same
    arguments, as every other 3x3 layer, and wrappers around ``conv_wino`` (checkers, tracers) need not know about the request."""
    _tls = threading.local()

    def __init__(self, keys):
        self.keys = keys

    def __enter__(self):
        self.prev = getattr(self._tls, 'keys', None)
        self._tls.keys = self.keys
        return self.keys

    def __exit__(self, *exc):
        self._tls.keys = self.prev
        return False

    @classmethod
    def current(cls):
        return getattr(cls._tls, 'keys', None)


def conv_wino(x, x_coff, plan, y, y_coff, relu=False, accumulate=False, ymask=None, ymul=None, yscale=1.0, drop=None, drop_advance=None):
    """y[..., y_coff:y_coff+N] (=|+=) conv3x3(x[..., x_coff:x_coff+C]) (+bias) (* ymul) (* yscale) (zero where ymask <= 0) (ReLU),
    Winograd F(2x2,3x3) kernel.  ``ymask`` / ``ymul`` are read through y's own channel window (same shape as y).  ``yscale``
    (a constant factor, e.g. the dropout scale), ``drop`` (a DropState: counter-based dropout of the output) and ``drop_advance`` (a
    DropState whose step this launch advances; never the one ``drop`` names) need the balanced kernel (``plan.cfg_id`` = tiles.WINO_SK_CFG).
    Inside ``det_keys_request(keys)`` the V-shared kernel (tiles.WINO_VS_CFG) also stores the detection keys where ``keys.fits``;
    every other launch ignores the request and leaves ``keys.written`` False."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    if tuple(y.shape[:3]) != (B, H, W):
        raise ValueError(f'conv_wino: x {tuple(x.shape)} and y {tuple(y.shape)} disagree on B,H,W')
    yp = y.shape[3]
    if x_coff < 0 or x_coff + plan.C > xp or y_coff < 0 or y_coff + plan.N > yp:
        raise ValueError('conv_wino: channel window out of range')
    if B * H * W * max(xp, yp) >= 2 ** 40:
        raise ValueError('conv_wino: tensor too large')
    br = None
    if timing._timer is not None:
        npix = B * H * W
        # flops = what the MFMA pipe executes (16 element-wise GEMMs per 2x2 tile = direct form / 2.25): the roofline
        # fraction of this kernel is against that; bench.py also quotes the direct-form equivalent
        br = _Bracket(wino_kernel_name(plan.cfg_id), f'9tap C{plan.C} N{plan.N} {H}x{W}', 2.0 * npix * plan.N * plan.C * 4,
                      4.0 * (npix * (plan.C + plan.N) + plan.N * plan.C * 16))
    for t, nm in ((ymask, 'ymask'), (ymul, 'ymul')):
        if t is not None:
            _check_nhwc(t, nm)
            if tuple(t.shape) != tuple(y.shape):
                raise ValueError(f'conv_wino: {nm} must have the shape of y')
    if drop is not None and drop_advance is not None and drop.state.data_ptr() == drop_advance.state.data_ptr():
        # the advance is one lane's unordered write: the other workgroups of the same launch would key their masks with either step
        raise ValueError('conv_wino: a launch cannot advance the dropout state it draws its own mask from')
    if plan.cfg_id % 1000 == tiles.WINO_SK_CFG:
        sk = wino_sk_schedule(B * -(-H // 4) * -(-W // 16), plan.N, plan.C, x.device)
        sk_ws, sk_cnt = sk.workspace()               # (per launch stream: concurrent lanes must not share slabs / tickets)
        rc = nat.lib().sqd_conv_wino_sk_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), nat.ptr(ymask), nat.ptr(ymul),
                                            float(yscale), B, H, W, plan.C, xp, x_coff, plan.N, plan.Npad, yp, y_coff, int(relu),
                                            int(accumulate), nat.ptr(sk.seg_off), nat.ptr(sk.segs), sk.G, sk.nslabs, nat.ptr(sk_ws),
                                            nat.ptr(sk_cnt), nat.ptr(drop.state) if drop is not None else None,
                                            drop.keep16 if drop is not None else 0, float(drop.scale) if drop is not None else 0.0,
                                            nat.ptr(drop_advance.state) if drop_advance is not None else None, nat.stream_handle(x.device))
        nat.check(rc, 'sqd_conv_wino_sk_fwd')
    elif plan.cfg_id % 1000 == tiles.WINO_VS_CFG:
        if yscale != 1.0 or drop is not None or drop_advance is not None or accumulate or ymask is not None or ymul is not None:
            raise ValueError('conv_wino: the V-shared kernel (cfg tiles.WINO_VS_CFG) has the plain bias / ReLU epilogue only')
        if plan.N > 80 or plan.Npad != 80:
            raise ValueError('conv_wino: the V-shared kernel (cfg tiles.WINO_VS_CFG) runs N <= 80 packed 80 wide')
        det_keys = det_keys_request.current()
        if det_keys is not None and det_keys.fits(plan, y, y_coff, relu):
            rc = nat.lib().sqd_conv_wino_vs_keys_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), B, H, W, plan.C, xp, x_coff,
                                                     plan.N, plan.Npad, yp, y_coff, int(relu), nat.ptr(det_keys.ws), det_keys.score_thresh,
                                                     det_keys.anchors_per_cell, det_keys.num_classes, nat.stream_handle(x.device))
            nat.check(rc, 'sqd_conv_wino_vs_keys_fwd')
            det_keys.written = True
        else:
            rc = nat.lib().sqd_conv_wino_vs_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), B, H, W, plan.C, xp, x_coff,
                                                plan.N, plan.Npad, yp, y_coff, int(relu), nat.stream_handle(x.device))
            nat.check(rc, 'sqd_conv_wino_vs_fwd')
    else:
        if yscale != 1.0 or drop is not None or drop_advance is not None:
            raise ValueError('conv_wino: yscale / drop / drop_advance need the balanced kernel (cfg tiles.WINO_SK_CFG)')
        rc = nat.lib().sqd_conv_wino_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), nat.ptr(ymask), nat.ptr(ymul),
                                         B, H, W, plan.C, xp, x_coff, plan.N, plan.Npad, yp, y_coff, int(relu), int(accumulate),
                                         plan.cfg_id, nat.stream_handle(x.device))
        nat.check(rc, 'sqd_conv_wino_fwd')
    if br is not None:
        br.done()
    return y


def fire_wino(x, x_coff, plan, y, y_coff1, y_coff3):
    """y[..., y_coff1:+N1] = relu(expand1x1(x)), y[..., y_coff3:+N3] = relu(expand3x3(x)) in ONE Winograd launch."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    if tuple(y.shape[:3]) != (B, H, W):
        raise ValueError('fire_wino: x and y disagree on B,H,W')
    yp = y.shape[3]
    if x_coff < 0 or x_coff + plan.C > xp or min(y_coff1, y_coff3) < 0 or y_coff1 + plan.N1 > yp or y_coff3 + plan.N3 > yp:
        raise ValueError('fire_wino: channel window out of range')
    if not (y_coff1 + plan.N1 <= y_coff3 or y_coff3 + plan.N3 <= y_coff1):
        raise ValueError('fire_wino: output windows overlap')
    br = None
    if timing._timer is not None:
        npix = B * H * W
        br = _Bracket(fire_wino_kernel_name(plan.cfg_id), f'fire C{plan.C} E{plan.N1}+{plan.N3} {H}x{W}',
                      2.0 * npix * plan.C * (4 * plan.N3 + plan.N1), 4.0 * (npix * (plan.C + plan.N1 + plan.N3) + plan.C * (16 * plan.N3 + plan.N1)))
    rc = nat.lib().sqd_fire_wino_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.b3), nat.ptr(plan.b1), nat.ptr(y), B, H, W, plan.C, xp, x_coff,
                                     plan.N3, y_coff3, plan.N1, y_coff1, plan.Npad, yp, plan.cfg_id, nat.stream_handle(x.device))
    nat.check(rc, 'sqd_fire_wino_fwd')
    if br is not None:
        br.done()
    return y


def fire_bridge(x, x_coff, plan, y, y_coff, save=None, save_coff1=0, save_coff3=None):
    """y[..., y_coff:+Nsq] = relu(squeeze'(cat(relu(expand1x1(x)), relu(expand3x3(x))))) in ONE launch.  Inference: the concatenated
    expand output is never written.  Training (``save``: [B,H,W,>=N1+N3]): it is stored too -- expand1x1 at ``save_coff1``, expand3x3 at
    ``save_coff3`` (default: right behind the expand1x1 window) -- for the backward; only the small-C form (plan.cfg_id 12) has it."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    if tuple(y.shape[:3]) != (B, H, W) or plan.pooled:
        raise ValueError('fire_bridge: x and y disagree on B,H,W (or the plan is a pooled one)')
    yp = y.shape[3]
    if x_coff < 0 or x_coff + plan.C > xp or y_coff < 0 or y_coff + plan.Nsq > yp:
        raise ValueError('fire_bridge: channel window out of range')
    if save is not None:
        _check_nhwc(save, 'save')
        if save_coff3 is None:
            save_coff3 = save_coff1 + plan.N1
        sp = save.shape[3]
        if tuple(save.shape[:3]) != (B, H, W) or min(save_coff1, save_coff3) < 0 or save_coff1 + plan.N1 > sp or save_coff3 + plan.N3 > sp:
            raise ValueError('fire_bridge: save must be [B,H,W,.] with both expand windows inside')
        if not (save_coff1 + plan.N1 <= save_coff3 or save_coff3 + plan.N3 <= save_coff1):
            raise ValueError('fire_bridge: the two windows of save overlap')
        if plan.cfg_id % 1000 != 12:
            raise ValueError('fire_bridge: only the small-C form (cfg 12) stores the expand output')
    br = None
    if timing._timer is not None:
        npix = B * H * W
        br = _Bracket('fire_bridge_save' if save is not None else 'fire_bridge', f'fire C{plan.C} E{plan.N1}+{plan.N3} -> S{plan.Nsq} {H}x{W}',
                      2.0 * npix * (plan.C * (4 * plan.N3 + plan.N1) + (plan.N1 + plan.N3) * plan.Nsq),
                      4.0 * (npix * (plan.C + plan.Nsq + (plan.N1 + plan.N3 if save is not None else 0))
                             + plan.C * (16 * plan.N3 + plan.N1) + (plan.N1 + plan.N3) * plan.Nsq))
    if save is not None:
        rc = nat.lib().sqd_fire_bridge_save_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias_tab), nat.ptr(plan.sq_ops), nat.ptr(plan.sq_bias),
                                                nat.ptr(y), nat.ptr(save), B, H, W, plan.C, xp, x_coff, plan.N3, plan.N1, plan.Npad, plan.Nsq,
                                                yp, y_coff, sp, save_coff3, save_coff1, nat.stream_handle(x.device))
        nat.check(rc, 'sqd_fire_bridge_save_fwd')
    else:
        rc = nat.lib().sqd_fire_bridge_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias_tab), nat.ptr(plan.sq_ops), nat.ptr(plan.sq_bias),
                                           nat.ptr(y), B, H, W, plan.C, xp, x_coff, plan.N3, plan.N1, plan.Npad, plan.Nsq, yp, y_coff,
                                           plan.cfg_id, nat.stream_handle(x.device))
        nat.check(rc, 'sqd_fire_bridge_fwd')
    if br is not None:
        br.done()
    return y


def fire_pool_bridge(x, x_coff, plan, y, y_coff, nseg=4, save=None, codes=None, save_coff1=0, save_coff3=None):
    """y[..., y_coff:+Nsq] = relu(squeeze'(maxpool3x3s2_ceil(cat(relu(expand1x1(x)), relu(expand3x3(x)))))) in ONE launch; y is
    [B, Hp, Wp, .] with (Hp, Wp) = pool_out_size(H, W).  ``plan``: FireBridgePlan(..., pooled=True).  Inference: neither the expand
    output nor the pooled tensor is written.  Training (``save`` fp32 [B,Hp,Wp,>=N1+N3] and ``codes`` uint8 of the same shape): the
    pooled tensor and the pool's arg-max / ReLU codes are stored too (everything the backward reads of this stage)."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    Hp, Wp = pool_out_size(H, W)
    if tuple(y.shape[:3]) != (B, Hp, Wp) or not plan.pooled:
        raise ValueError('fire_pool_bridge: y must be [B, Hp, Wp, .] of the pooled map and the plan a pooled one')
    yp = y.shape[3]
    if x_coff < 0 or x_coff + plan.C > xp or y_coff < 0 or y_coff + plan.Nsq > yp:
        raise ValueError('fire_pool_bridge: channel window out of range')
    if (save is None) != (codes is None):
        raise ValueError('fire_pool_bridge: save and codes go together')
    if save is not None:
        _check_nhwc(save, 'save')
        if save_coff3 is None:
            save_coff3 = save_coff1 + plan.N1
        sp = save.shape[3]
        if tuple(save.shape[:3]) != (B, Hp, Wp) or min(save_coff1, save_coff3) < 0 or save_coff1 + plan.N1 > sp or save_coff3 + plan.N3 > sp:
            raise ValueError('fire_pool_bridge: save must be [B,Hp,Wp,.] with both expand windows inside')
        if not (save_coff1 + plan.N1 <= save_coff3 or save_coff3 + plan.N3 <= save_coff1):
            raise ValueError('fire_pool_bridge: the two windows of save overlap')
        if tuple(codes.shape) != tuple(save.shape) or codes.dtype != torch.uint8 or not codes.is_contiguous() or codes.device != save.device:
            raise ValueError('fire_pool_bridge: codes must be a contiguous uint8 tensor of save\'s shape')
    br = None
    if timing._timer is not None:
        npix = B * H * W
        br = _Bracket('fire_pool_bridge_save' if save is not None else 'fire_pool_bridge',
                      f'fire C{plan.C} E{plan.N1}+{plan.N3} -> pool -> S{plan.Nsq} {H}x{W}',
                      2.0 * (npix * plan.C * (4 * plan.N3 + plan.N1) + B * Hp * Wp * (plan.N1 + plan.N3) * plan.Nsq),
                      4.0 * (npix * plan.C + B * Hp * Wp * (plan.Nsq + (1.25 * (plan.N1 + plan.N3) if save is not None else 0))
                             + plan.C * (16 * plan.N3 + plan.N1) + (plan.N1 + plan.N3) * plan.Nsq))
    if save is not None:
        rc = nat.lib().sqd_fire_pool_bridge_save_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias_tab), nat.ptr(plan.sq_ops), nat.ptr(plan.sq_bias),
                                                     nat.ptr(y), nat.ptr(save), nat.ptr(codes), B, H, W, plan.C, xp, x_coff, plan.N3, plan.N1,
                                                     plan.Npad, plan.Nsq, Hp, Wp, yp, y_coff, sp, save_coff3, save_coff1, int(nseg),
                                                     nat.stream_handle(x.device))
        nat.check(rc, 'sqd_fire_pool_bridge_save_fwd')
    else:
        rc = nat.lib().sqd_fire_pool_bridge_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias_tab), nat.ptr(plan.sq_ops), nat.ptr(plan.sq_bias),
                                                nat.ptr(y), B, H, W, plan.C, xp, x_coff, plan.N3, plan.N1, plan.Npad, plan.Nsq, Hp, Wp, yp, y_coff,
                                                int(nseg), nat.stream_handle(x.device))
        nat.check(rc, 'sqd_fire_pool_bridge_fwd')
    if br is not None:
        br.done()
    return y


def pool_squeeze(x, x_coff, C, plan, y, y_coff):
    """y[..., y_coff:y_coff+N] = relu(squeeze1x1(maxpool3x3s2_ceil(x[..., x_coff:x_coff+C]))) without materialising the
    pooled tensor (inference).  ``plan``: ConvPlan of the squeeze packed for POOL_SQUEEZE_CFG."""
    _check_nhwc(x, 'x'); _check_nhwc(y, 'y')
    B, H, W, xp = x.shape
    Ho, Wo = pool_out_size(H, W)
    if tuple(y.shape[:3]) != (B, Ho, Wo) or plan.taps != 1 or plan.C != C or plan.kc != 32 or plan.Npad != -(-plan.N // 16) * 16:
        raise ValueError('pool_squeeze: geometry / plan mismatch')
    if x_coff + C > xp or y_coff + plan.N > y.shape[3] or not pool_squeeze_ok(C, plan.N):
        raise ValueError('pool_squeeze: unsupported channel configuration')
    br = _Bracket('pool_squeeze', f'pool+squeeze C{C} N{plan.N} {H}x{W}', 2.0 * B * Ho * Wo * plan.N * C,
                  4.0 * B * (H * W * C + Ho * Wo * plan.N)) if timing._timer is not None else None
    rc = nat.lib().sqd_pool_squeeze_fwd(nat.ptr(x), nat.ptr(plan.w), nat.ptr(plan.bias), nat.ptr(y), B, H, W, C, xp, x_coff, plan.N, plan.Npad,
                                        y.shape[3], y_coff, nat.stream_handle(x.device))
    nat.check(rc, 'sqd_pool_squeeze_fwd')
    if br is not None:
        br.done()
    return y


_STEMS = ((3, 64), (7, 96))        # (kernel size, output channels) the library has stem kernels for


def _stem_args(name, image, weight, bias, unsupported=None):
    """The checks every stem forward wrapper starts with, under its own name in the messages (``unsupported``: the wrapper's own
    message for a weight no stem kernel takes); -> the contiguous operands (image, weight, bias or None) and the geometry
    B, H, W, N, k, Ho, Wo."""
    if image.dim() != 4 or image.shape[1] != 3 or image.dtype != torch.float32 or not image.is_cuda:
        raise ValueError(f'{name}: image must be fp32 CUDA NCHW with 3 channels, got {tuple(image.shape)}')
    N, ci, k, k2 = weight.shape
    if ci != 3 or k != k2 or (k, N) not in _STEMS:
        raise ValueError(unsupported or f'{name}: unsupported weight {tuple(weight.shape)}')
    B, _, H, W = image.shape
    Ho, Wo = stem_out_size(H, W, k)
    return (image.contiguous(), weight.detach().contiguous(), None if bias is None else bias.detach().contiguous(),
            B, H, W, N, k, Ho, Wo)


def stem_conv_relu(image, weight, bias, out=None, relu=True):
    """image NCHW [B,3,H,W]; weight OIHW [N,3,k,k] (the checkpoint tensor as is); -> NHWC [B,Ho,Wo,N]
    (``relu=False``: the bare convolution)."""
    image, w, b, B, H, W, N, k, Ho, Wo = _stem_args('stem', image, weight, bias)
    if out is None:
        out = torch.empty(B, Ho, Wo, N, device=image.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, Ho, Wo, N):
        raise ValueError('stem: bad out shape')
    br = _Bracket(f'stem_conv<{k}>', f'stem {H}x{W}', 2.0 * B * Ho * Wo * N * 3 * k * k,
                  4.0 * (B * 3 * H * W + B * Ho * Wo * N)) if timing._timer is not None else None
    rc = nat.lib().sqd_stem_conv_fwd(nat.ptr(image), nat.ptr(w), nat.ptr(b), nat.ptr(out), B, H, W, N, k, int(bool(relu)),
                                     nat.stream_handle(image.device))
    nat.check(rc, 'sqd_stem_conv_fwd')
    if br is not None:
        br.done()
    return out


def stem_pool(image, weight, bias, argmax=None):
    """Fused conv(3->N,k,s2)+ReLU+MaxPool(3,2,ceil): NCHW image -> NHWC pooled features [B,Hp,Wp,N]."""
    image, w, b, B, H, W, N, k, Ho, Wo = _stem_args('stem_pool', image, weight, bias)
    if Ho < 3 or Wo < 3:
        raise ValueError('stem_pool: input too small')
    Hp, Wp = pool_out_size(Ho, Wo)
    out = torch.empty(B, Hp, Wp, N, device=image.device, dtype=torch.float32)
    if argmax is not None and (tuple(argmax.shape) != (B, Hp, Wp, N) or argmax.dtype != torch.uint8):
        raise ValueError('stem_pool: bad argmax tensor')
    br = _Bracket(f'stem_pool<{k}>', f'stem+pool {H}x{W}', 2.0 * B * Ho * Wo * N * 3 * k * k,
                  4.0 * (B * 3 * H * W + B * Hp * Wp * N)) if timing._timer is not None else None
    rc = nat.lib().sqd_stem_conv_relu_pool_fwd(nat.ptr(image), nat.ptr(w), nat.ptr(b), nat.ptr(out), nat.ptr(argmax), B, H, W, N, k,
                                               nat.stream_handle(image.device))
    nat.check(rc, 'sqd_stem_conv_relu_pool_fwd')
    if br is not None:
        br.done()
    return out


def stem_pool_squeeze_ok(image_shape, stem_weight_shape, squeeze_width):
    """True where ops.stem_pool_squeeze has a kernel: the 3x3 / 64-channel stem, a 16-channel squeeze, image width a multiple of 4."""
    N, ci, k, k2 = stem_weight_shape
    return (k, N, squeeze_width) == (3, 64, 16) and image_shape[3] % 4 == 0 and image_shape[2] >= 5 and image_shape[3] >= 5


def stem_pool_squeeze(image, weight, bias, sq_weight, sq_bias, argmax=None):
    """conv(3->64,3,s2)+ReLU+MaxPool(3,2,ceil) AND the first Fire's squeeze (1x1, 64->16, +ReLU) in one launch
    (src/model/squeezedet.py:34-37, :17-18).  Inference (``argmax`` None): NCHW image -> NHWC squeeze output [B,Hp,Wp,16]; the pooled
    tensor is never written.  Training (``argmax``: uint8 [B,Hp,Wp,64]): -> (squeeze output, pooled tensor); the pooled tensor and
    its codes are stored for the backward as by ``stem_pool(argmax=)``."""
    unsupported = f'stem_pool_squeeze: unsupported geometry {tuple(image.shape)} / {tuple(weight.shape)} / {tuple(sq_weight.shape)}'
    image, w, b, B, H, W, N, k, Ho, Wo = _stem_args('stem_pool_squeeze', image, weight, bias, unsupported)
    nsq = sq_weight.shape[0]
    if tuple(sq_weight.shape[1:]) != (N, 1, 1) or not stem_pool_squeeze_ok(image.shape, weight.shape, nsq):
        raise ValueError(unsupported)
    Hp, Wp = pool_out_size(Ho, Wo)
    if argmax is not None and (tuple(argmax.shape) != (B, Hp, Wp, N) or argmax.dtype != torch.uint8 or not argmax.is_contiguous()):
        raise ValueError('stem_pool_squeeze: bad argmax tensor')
    out = torch.empty(B, Hp, Wp, nsq, device=image.device, dtype=torch.float32)
    ws = sq_weight.detach().contiguous()
    bs = None if sq_bias is None else sq_bias.detach().contiguous()
    br = _Bracket(f'stem_pool_sq{"_train" if argmax is not None else ""}<{k}>', f'stem+pool+squeeze {H}x{W} S{nsq}',
                  2.0 * B * (Ho * Wo * N * 3 * k * k + Hp * Wp * N * nsq),
                  4.0 * (B * 3 * H * W + B * Hp * Wp * nsq + (B * Hp * Wp * N * 1.25 if argmax is not None else 0))) if timing._timer is not None else None
    if argmax is not None:
        pooled = torch.empty(B, Hp, Wp, N, device=image.device, dtype=torch.float32)
        rc = nat.lib().sqd_stem_pool_squeeze_train_fwd(nat.ptr(image), nat.ptr(w), nat.ptr(b), nat.ptr(ws), nat.ptr(bs), nat.ptr(pooled),
                                                       nat.ptr(argmax), nat.ptr(out), B, H, W, N, k, nsq, nat.stream_handle(image.device))
        nat.check(rc, 'sqd_stem_pool_squeeze_train_fwd')
        if br is not None:
            br.done()
        return out, pooled
    rc = nat.lib().sqd_stem_pool_squeeze_fwd(nat.ptr(image), nat.ptr(w), nat.ptr(b), nat.ptr(ws), nat.ptr(bs), nat.ptr(out), B, H, W, N, k,
                                             nsq, nat.stream_handle(image.device))
    nat.check(rc, 'sqd_stem_pool_squeeze_fwd')
    if br is not None:
        br.done()
    return out


def maxpool(x, out=None, argmax=None, relu_codes=False):
    """MaxPool2d(3, 2, ceil_mode=True) on NHWC; ``argmax`` (uint8, same shape as out) is filled if given.  ``relu_codes=True``
    (x is a ReLU output, a backward follows): the codes also carry x's ReLU mask (15 = pooled value not > 0), so
    ``maxpool_bwd`` runs without ``relu_src``."""
    _check_nhwc(x, 'x')
    B, H, W, C = x.shape
    if H < 3 or W < 3 or C % 4:
        raise ValueError('maxpool: need H,W >= 3 and C % 4 == 0')
    Ho, Wo = pool_out_size(H, W)
    if out is None:
        out = torch.empty(B, Ho, Wo, C, device=x.device, dtype=torch.float32)
    if tuple(out.shape) != (B, Ho, Wo, C):
        raise ValueError('maxpool: bad out shape')
    if argmax is not None and (tuple(argmax.shape) != (B, Ho, Wo, C) or argmax.dtype != torch.uint8):
        raise ValueError('maxpool: bad argmax tensor')
    br = _Bracket('maxpool_fwd', f'pool C{C} {H}x{W}', 0.0, 4.0 * B * C * (H * W + Ho * Wo)) if timing._timer is not None else None
    if relu_codes:
        if argmax is None:
            raise ValueError('maxpool: relu_codes needs an argmax tensor')
        rc = nat.lib().sqd_maxpool3x3s2_ceil_fwd_relu(nat.ptr(x), nat.ptr(out), nat.ptr(argmax), B, H, W, C, nat.stream_handle(x.device))
    else:
        rc = nat.lib().sqd_maxpool3x3s2_ceil_fwd(nat.ptr(x), nat.ptr(out), nat.ptr(argmax), B, H, W, C, nat.stream_handle(x.device))
    nat.check(rc, 'sqd_maxpool3x3s2_ceil_fwd')
    if br is not None:
        br.done()
    return out


def maxpool_bwd(dy, argmax, in_hw, out=None, relu_src=None):
    _check_nhwc(dy, 'dy')
    B, Ho, Wo, C = dy.shape
    H, W = in_hw
    if pool_out_size(H, W) != (Ho, Wo) or tuple(argmax.shape) != (B, Ho, Wo, C) or argmax.dtype != torch.uint8:
        raise ValueError('maxpool_bwd: geometry mismatch')
    if out is None:
        out = torch.empty(B, H, W, C, device=dy.device, dtype=torch.float32)
    if relu_src is not None and (tuple(relu_src.shape) != (B, H, W, C) or not relu_src.is_contiguous()):
        raise ValueError('maxpool_bwd: relu_src must match the pool input')
    if not (dy.is_contiguous() and argmax.is_contiguous() and out.is_contiguous()):
        raise ValueError('maxpool_bwd: dy, argmax and out must be contiguous')
    br = _Bracket('maxpool_bwd', f'poolbwd C{C} {H}x{W}', 0.0, 4.0 * B * C * (H * W * (2 if relu_src is not None else 1) + Ho * Wo * 1.25)) if timing._timer is not None else None
    # the kernel's grid carries (image, row pair) in blockIdx.y (<= 65535): larger batches go in slices of whole images
    per = max(1, 65535 // ((H + 1) // 2))
    if (H + 1) // 2 > 65535:
        raise ValueError(f'maxpool_bwd: {H} input rows exceed the kernel\'s grid (at most {2 * 65535})')
    for b0 in range(0, B, per):
        b1 = min(B, b0 + per)
        rc = nat.lib().sqd_maxpool3x3s2_ceil_bwd(nat.ptr(dy[b0:b1]), nat.ptr(argmax[b0:b1]), nat.ptr(out[b0:b1]),
                                                 nat.ptr(relu_src[b0:b1]) if relu_src is not None else None, b1 - b0, H, W, C,
                                                 nat.stream_handle(dy.device))
        nat.check(rc, 'sqd_maxpool3x3s2_ceil_bwd')
    if br is not None:
        br.done()
    return out


HEAD_NARROW_MAX_CLASSES = 16   # the one-lane-per-row kernels: float l[16] per lane
HEAD_MANY_MAX_CLASSES = 256    # the lane-group kernels: 16 lanes x 16 registers per anchor row


def head_path(num_classes):
    """Which head kernels serve ``num_classes``: 'narrow' (<= 16: ``decode`` / ``resolve`` / ``detect`` / ``detect_wide`` / ``loss_*``,
    the benchmarked kernels) or 'many' (17 .. 256: ``decode_many`` / ``resolve_many`` / ``detect_many`` / ``filter_dense_many`` /
    ``loss_*_many``).  ValueError outside 1 .. 256."""
    C = int(num_classes)
    if C < 1 or C > HEAD_MANY_MAX_CLASSES:
        raise ValueError(f'num_classes must be in 1 .. {HEAD_MANY_MAX_CLASSES} (16 lanes x 16 registers per anchor row), got {C}')
    return 'narrow' if C <= HEAD_NARROW_MAX_CLASSES else 'many'


def convdet_width(anchors_per_grid, num_classes):
    """(N, Npad) of ConvDet: N = anchors_per_grid * (num_classes + 5) output channels; Npad = the width the executors run it at.
    Npad == N (not padded) where the convolution forms take N as it is (N % 4 == 0 -- every width that ran before, 72 and 108
    among them); otherwise the next multiple of 64: the Winograd data gradient reads the padded gradient as its C (a multiple of
    8), and the Winograd weight gradient takes N <= 80 or N % 64 == 0 (``tiles.wgrad_uses_wino``)."""
    N = int(anchors_per_grid) * (int(num_classes) + 5)
    return N, convdet_pad_width(N)


def convdet_pad_width(N):
    """The width a ConvDet of N output channels runs at (``convdet_width``)."""
    N = int(N)
    return N if N % 4 == 0 else -(-N // 64) * 64


def convdet_padded(anchors_per_grid, num_classes):
    """Whether ConvDet runs at a padded width (``convdet_width``)."""
    N, Npad = convdet_width(anchors_per_grid, num_classes)
    return Npad != N


def convdet_pack(y_pad, N, out=None):
    """[B,H,W,Npad] -> contiguous [B,H,W,N] (the first N channels): ConvDet's padded scratch to the reference's pred layout."""
    _check_nhwc(y_pad, 'y_pad')
    B, H, W, Npad = y_pad.shape
    if not 1 <= N <= Npad:
        raise ValueError(f'convdet_pack: N = {N} outside 1 .. {Npad}')
    if out is None:
        out = torch.empty(B, H, W, N, device=y_pad.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, H, W, N) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != y_pad.device:
        raise ValueError('convdet_pack: bad out tensor')
    br = _Bracket('convdet_pack', f'pack N{N} <- {Npad} {H}x{W}', 0.0, 8.0 * B * H * W * N) if timing._timer is not None else None
    nat.check(nat.lib().sqd_channel_pack_fwd(nat.ptr(y_pad), nat.ptr(out), B * H * W, int(N), Npad, nat.stream_handle(y_pad.device)),
              'sqd_channel_pack_fwd')
    if br is not None:
        br.done()
    return out


def convdet_unpack(dy, Npad):
    """Contiguous [B,H,W,N] -> [B,H,W,Npad], zero past N: dpred as the padded ConvDet's gradient launches read it."""
    _check_nhwc(dy, 'dy')
    B, H, W, N = dy.shape
    if Npad < N:
        raise ValueError(f'convdet_unpack: Npad = {Npad} < N = {N}')
    out = torch.empty(B, H, W, Npad, device=dy.device, dtype=torch.float32)
    br = _Bracket('convdet_unpack', f'unpack N{N} -> {Npad} {H}x{W}', 0.0, 4.0 * B * H * W * (N + Npad)) if timing._timer is not None else None
    nat.check(nat.lib().sqd_channel_unpack_fwd(nat.ptr(dy), nat.ptr(out), B * H * W, N, int(Npad), nat.stream_handle(dy.device)),
              'sqd_channel_unpack_fwd')
    if br is not None:
        br.done()
    return out


def wgrad_reduce_rows(slab, S, N, Npad, C, taps, dw, db, scale=1.0):
    """The S slabs of an Npad-wide weight gradient (``conv_wgrad(..., slab=)``) reduced over the first N rows into ``dw``
    [N,C,k,k] / ``db`` [N] (contiguous views of the flat gradient buffer), times ``scale``."""
    k = 3 if taps == 9 else 1
    stride = Npad * taps * C + Npad
    if slab.numel() != S * stride or not slab.is_contiguous() or slab.dtype != torch.float32:
        raise ValueError('wgrad_reduce_rows: slab workspace does not match the layer')
    if tuple(dw.shape) != (N, C, k, k) or tuple(db.shape) != (N,) or not dw.is_contiguous() or not db.is_contiguous() \
            or dw.dtype != torch.float32 or db.dtype != torch.float32 or N > Npad:
        raise ValueError('wgrad_reduce_rows: dw / db must be contiguous fp32 [N,C,k,k] / [N] with N <= Npad')
    br = _Bracket('wgrad_reduce_rows', f'N{N} of {Npad} C{C}', 0.0, 4.0 * (S + 1) * (N * taps * C + N)) if timing._timer is not None else None
    nat.check(nat.lib().sqd_wgrad_reduce_rows(nat.ptr(slab), nat.ptr(dw), nat.ptr(db), int(S), int(N), int(Npad), int(C), int(taps),
                                              float(scale), nat.stream_handle(slab.device)), 'sqd_wgrad_reduce_rows')
    if br is not None:
        br.done()


def decode(pred, anchors, input_size, num_classes):
    """pred [B,A,C+5], anchors [A,4] fp32 -> class_ids int64 [B,A], scores [B,A], boxes [B,A,4]."""
    return _decode('sqd_decode_fwd', pred, anchors, input_size, num_classes)


def _decode(_entry, pred, anchors, input_size, num_classes):
    if pred.dim() != 3 or pred.shape[2] != num_classes + 5 or pred.dtype != torch.float32 or not pred.is_cuda:
        raise ValueError(f'decode: bad pred {tuple(pred.shape)}')
    pred = pred.contiguous()
    B, A, _ = pred.shape
    if tuple(anchors.shape) != (A, 4) or anchors.dtype != torch.float32 or anchors.device != pred.device:
        raise ValueError('decode: anchors must be fp32 [A,4] on the same device')
    ids = torch.empty(B, A, device=pred.device, dtype=torch.int64)
    scores = torch.empty(B, A, device=pred.device, dtype=torch.float32)
    boxes = torch.empty(B, A, 4, device=pred.device, dtype=torch.float32)
    rc = getattr(nat.lib(), _entry)(nat.ptr(pred), nat.ptr(anchors.contiguous()), nat.ptr(ids), nat.ptr(scores), nat.ptr(boxes),
                                    B, A, num_classes, int(input_size[0]), int(input_size[1]), nat.stream_handle(pred.device))
    nat.check(rc, _entry)
    return ids, scores, boxes


def decode_many(pred, anchors, input_size, num_classes):
    """``decode`` for 1 <= num_classes <= 256 (a 16-lane group per anchor row; class = the lowest index attaining the score)."""
    head_path(num_classes)
    return _decode('sqd_decode_many_fwd', pred, anchors, input_size, num_classes)


def resolve(pred, anchors, input_size, num_classes, log_softmax=False):
    """The reference's PredictionResolver outputs: (probs [B,A,C], log_probs [B,A,C] | None, scores [B,A,1],
    deltas [B,A,4], boxes [B,A,4])."""
    return _resolve('sqd_resolve_fwd', pred, anchors, input_size, num_classes, log_softmax)


def _resolve(_entry, pred, anchors, input_size, num_classes, log_softmax=False):
    if pred.dim() != 3 or pred.shape[2] != num_classes + 5 or pred.dtype != torch.float32 or not pred.is_cuda:
        raise ValueError(f'resolve: bad pred {tuple(pred.shape)}')
    pred = pred.contiguous()
    B, A, _ = pred.shape
    if tuple(anchors.shape) != (A, 4) or anchors.dtype != torch.float32 or anchors.device != pred.device:
        raise ValueError('resolve: anchors must be fp32 [A,4] on the same device')
    dev = pred.device
    probs = torch.empty(B, A, num_classes, device=dev, dtype=torch.float32)
    logp = torch.empty(B, A, num_classes, device=dev, dtype=torch.float32) if log_softmax else None
    scores = torch.empty(B, A, 1, device=dev, dtype=torch.float32)
    deltas = torch.empty(B, A, 4, device=dev, dtype=torch.float32)
    boxes = torch.empty(B, A, 4, device=dev, dtype=torch.float32)
    rc = getattr(nat.lib(), _entry)(nat.ptr(pred), nat.ptr(anchors.contiguous()), nat.ptr(probs), nat.ptr(logp), nat.ptr(scores),
                                    nat.ptr(deltas), nat.ptr(boxes), B, A, num_classes, int(input_size[0]), int(input_size[1]),
                                    nat.stream_handle(dev))
    nat.check(rc, _entry)
    return probs, logp, scores, deltas, boxes


def resolve_many(pred, anchors, input_size, num_classes, log_softmax=False):
    """``resolve`` for 1 <= num_classes <= 256."""
    head_path(num_classes)
    return _resolve('sqd_resolve_many_fwd', pred, anchors, input_size, num_classes, log_softmax)


def _det_buffers(B, K, device, A=None, num_classes=None):
    """(count, class_ids, scores, boxes, anchor_idx[, keys workspace]) for the fused detection kernels (``num_classes``: sizes the
    workspace for the many-class detect past 16 classes)."""
    bufs = (torch.zeros(B, device=device, dtype=torch.int32), torch.zeros(B, K, device=device, dtype=torch.int64),
            torch.zeros(B, K, device=device, dtype=torch.float32), torch.zeros(B, K, 4, device=device, dtype=torch.float32),
            torch.zeros(B, K, device=device, dtype=torch.int32))
    if A is not None:
        bufs = bufs + (_det_workspace(B, A, device, K, num_classes),)
    return bufs


def det_packed_layout(B, K):
    """Byte layout of the packed result buffer: [(offset, elements, dtype, shape)] for (count, class_ids, scores, boxes, anchor_idx)
    -- 16-byte aligned sections -- and the total size.  The host reads a copied buffer back through the same table (lanes.py)."""
    sizes = [(B, torch.int32), (B * K, torch.int64), (B * K, torch.float32), (B * K * 4, torch.float32), (B * K, torch.int32)]
    shapes = [(B,), (B, K), (B, K), (B, K, 4), (B, K)]
    secs, off = [], 0
    for (n, dt), shp in zip(sizes, shapes):
        off = -(-off // 16) * 16
        secs.append((off, n, dt, shp))
        off += n * torch.empty(0, dtype=dt).element_size()
    return secs, -(-off // 16) * 16


def det_buffers_packed(B, K, device, A=None, num_classes=None):
    """The same five result tensors as views of ONE allocation (16-byte aligned sections), so that a whole batch's compact
    detections leave the GPU with a single device-to-host copy.  -> (bufs as ``_det_buffers``, flat uint8 tensor)."""
    secs, total = det_packed_layout(B, K)
    flat = torch.zeros(total, device=device, dtype=torch.uint8)
    bufs = tuple(flat[o:o + n * torch.empty(0, dtype=dt).element_size()].view(dt).view(shp) for o, n, dt, shp in secs)
    if A is not None:
        bufs = bufs + (_det_workspace(B, A, device, K, num_classes),)
    return bufs, flat


def det_workspace_words(B, A):
    """int32 words of the detect workspace: B x ceil4(A) keys + B arrival counters (sqd_detect_shift_fwd)."""
    return B * (-(-A // 4) * 4) + B


DET_NARROW_MAX_K = 64          # detect_kernel: one wave holds the 64 x 64 suppression matrix
DET_NARROW_MAX_A = 25596       # ... and an image's keys + uint16 candidate indices fit 150 KB of LDS
DET_WIDE_MAX_K = 1024          # the wide path: one candidate per thread of a 1024-thread workgroup, 128 KB bit matrix in LDS
DET_WIDE_MAX_A = 1 << 20       # gt_encode's own limit


def detect_path(K, A):
    """Which fused detect serves ``keep_top_k = K`` on ``A`` anchors: 'narrow' (``detect`` / ``filter_dense``: one launch, the
    benchmarked kernel) for K <= 64 and A <= 25 596, else 'wide' (``detect_wide`` / ``filter_dense_wide``).  ValueError past the
    wide path's limits."""
    K, A = int(K), int(A)
    if K < 1 or A < 1:
        raise ValueError(f'detect: keep_top_k and the anchor count must be >= 1 (got {K}, {A})')
    if K > DET_WIDE_MAX_K:
        raise ValueError(f'detect: keep_top_k {K} exceeds the limit of {DET_WIDE_MAX_K}')
    if A > DET_WIDE_MAX_A:
        raise ValueError(f'detect: {A} anchors exceed the limit of {DET_WIDE_MAX_A} (2^20)')
    return 'narrow' if K <= DET_NARROW_MAX_K and A <= DET_NARROW_MAX_A else 'wide'


def det_workspace_words_wide(B, A, K):
    """int32 words of the wide detect workspace (``sqd_detect_wide_workspace_words``: B x ceil4(A) keys)."""
    n = int(nat.lib().sqd_detect_wide_workspace_words(int(B), int(A), int(K)))
    if n < 0:
        detect_path(K, A)                                  # names the limit
        raise ValueError(f'detect: no wide workspace for B={B}, A={A}, keep_top_k={K}')
    return n


def _det_workspace(B, A, device, K=DET_NARROW_MAX_K, num_classes=None):
    """Workspace of the fused detect launch (``keys_ws``).  Narrow path: the keys the eight scoring workgroups of an image hand to
    its last arriver + one arrival counter per image; zeroed once, every launch returns the counters to zero.  Parameters only the
    wide path takes (``detect_path``): its key workspace.  (Parameters neither takes get the narrow size: that launch refuses them.)"""
    K, A = int(K), int(A)
    many = num_classes is not None and int(num_classes) > HEAD_NARROW_MAX_CLASSES      # (the many-class detect is always two launches)
    if (many or K > DET_NARROW_MAX_K or A > DET_NARROW_MAX_A) and 1 <= K <= DET_WIDE_MAX_K and 1 <= A <= DET_WIDE_MAX_A:
        return torch.zeros(det_workspace_words_wide(B, A, K), device=device, dtype=torch.int32)
    return torch.zeros(det_workspace_words(B, A), device=device, dtype=torch.int32)


def _check_score_thresh(name, score_thresh):
    # the kernel's candidate key is the fp32 score bits if score > score_thresh, else 0 ("no candidate"): exact for thresholds >= 0
    # only (a negative one would drop scores of exactly 0 and, in the dense filter, rank negative scores first)
    if not float(score_thresh) >= 0.0:
        raise ValueError(f'{name}: score_thresh must be >= 0 (got {score_thresh})')


def _check_det_out(bufs, B, K, device):
    """A caller's result buffers must be exactly what the kernel writes: it stores B x K rows without knowing their sizes."""
    if len(bufs) not in (5, 6):
        raise ValueError(f'detect: out must hold 5 result tensors (+ an optional workspace), got {len(bufs)}')
    want = (((B,), torch.int32), ((B, K), torch.int64), ((B, K), torch.float32), ((B, K, 4), torch.float32), ((B, K), torch.int32))
    for i, (t, (shape, dt)) in enumerate(zip(bufs[:5], want)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or t.device != device or not t.is_contiguous():
            got = (tuple(t.shape), t.dtype, str(t.device)) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f'detect: out[{i}] must be a contiguous {dt} {shape} tensor on {device}, got {got}')
    if bufs[3].data_ptr() % 16:
        raise ValueError('detect: out[3] (boxes) must be 16-byte aligned')


def _pred_side(name, pred, anchors, num_classes, score_thresh, K=None, scales=None, shifts=None, many=False, V=None):
    """The pred-side argument block of every fused detect, in the order all of them check: pred, the class count (``many``: the
    functions that take up to 256), ``score_thresh``, the view count (``V`` given: pred holds V rows per image), the wide limits
    (``K`` given: ValueError naming the limit, before anything is allocated or written), anchors, scales, shifts.
    -> (contiguous pred, B, A)."""
    if pred.dim() != 3 or pred.shape[2] != num_classes + 5 or pred.dtype != torch.float32 or not pred.is_cuda:
        raise ValueError(f'{name}: bad pred {tuple(pred.shape)}')
    if many:
        head_path(num_classes)
    _check_score_thresh(name, score_thresh)
    if V is not None and (isinstance(V, bool) or not hasattr(V, '__index__') or int(V) < 1):
        raise ValueError(f'{name}: V must be an int >= 1, got {V!r}')
    pred = pred.contiguous()
    B, A, _ = pred.shape
    if V is not None:
        if B < int(V) or B % int(V):
            raise ValueError(f'{name}: pred has {B} rows, not a positive multiple of V = {int(V)}')
        B //= int(V)
    if K is not None:
        detect_path(K, A)
    if V is not None and int(V) * (-(-A // 4) * 4) > DET_VIEWS_MAX_ROW:
        raise ValueError(f'{name}: {int(V)} views of {A} anchors exceed the pooled row limit V * ceil4(A) <= {DET_VIEWS_MAX_ROW} (2^20)')
    if tuple(anchors.shape) != (A, 4) or anchors.dtype != torch.float32 or anchors.device != pred.device:
        raise ValueError(f'{name}: anchors must be fp32 [A,4] on the same device')
    if scales is not None and (tuple(scales.shape) != (B, 2) or scales.dtype != torch.float32 or scales.device != pred.device):
        raise ValueError(f'{name}: scales must be fp32 [B,2] (sy, sx)')
    if shifts is not None and (tuple(shifts.shape) != (B, 2) or shifts.dtype != torch.float32 or shifts.device != pred.device or not shifts.is_contiguous()):
        raise ValueError(f'{name}: shifts must be contiguous fp32 [B,2] (dy, dx)')
    return pred, B, A


def _dense_side(name, class_ids, scores, boxes, num_classes, score_thresh, K=None, many=False):
    """The dense-side argument block of every filter (class_ids int64 [B,A], scores [B,A], boxes [B,A,4]), then the class count
    (``many``), ``score_thresh`` and the wide limits (``K`` given).  -> (B, A)."""
    if scores.dim() != 2 or class_ids.shape != scores.shape or tuple(boxes.shape) != tuple(scores.shape) + (4,):
        raise ValueError(f'{name}: shape mismatch')
    if class_ids.dtype != torch.int64 or scores.dtype != torch.float32 or boxes.dtype != torch.float32 or not scores.is_cuda \
            or class_ids.device != scores.device or boxes.device != scores.device:
        raise ValueError(f'{name}: dtype/device mismatch')
    if many:
        head_path(num_classes)
    _check_score_thresh(name, score_thresh)
    B, A = scores.shape
    if K is not None:
        detect_path(K, A)
    return B, A


def _wide_out(name, out, B, A, K, device, rows=None):
    """Result buffers and key workspace of a wide launch: the caller's ``out`` (checked against B and K) or fresh tensors; the
    workspace -- ``rows`` (default B) key rows -- is the caller's sixth ``out`` tensor if it is large enough, else a fresh one.
    -> (bufs, keys)."""
    if out is not None:
        _check_det_out(out, B, K, device)
    bufs = tuple(out) if out is not None else _det_buffers(B, K, device)
    need = det_workspace_words_wide(B if rows is None else rows, A, K)
    keys = bufs[5] if len(bufs) == 6 else None
    if keys is not None and (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32 or keys.device != device):
        raise ValueError(f'{name}: workspace must be an int32 tensor on the same device')
    if keys is None or keys.numel() < need or not keys.is_contiguous() or keys.data_ptr() % 16:
        keys = torch.empty(need, device=device, dtype=torch.int32)
    return bufs, keys


def detect(pred, anchors, input_size, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, scales=None, out=None, shifts=None,
           keys_ready=False):
    """Fused decode + top-k + class-wise NMS + threshold for a batch.  ``keys_ready``: the workspace in ``out`` already holds the keys
    of this ``pred`` for this ``score_thresh`` (ConvDet's launch wrote them: ``DetKeys``) -- one workgroup per image, no scoring pass.
    Returns (count int32 [B], class_ids int64 [B,K], scores [B,K], boxes [B,K,4], anchor_idx int32 [B,K]).  ``scales`` [B,2] =
    (sy, sx): boxes are divided by them; ``shifts`` [B,2] = (dy, dx): added afterwards (the padding / crops terms of
    ``boxes_postprocess``, src/utils/boxes.py:149-155).  ``out``: the five result tensors (checked against B and ``keep_top_k``) and
    optionally the key workspace; a workspace smaller than ``det_workspace_words`` means one workgroup per image.
    ``score_thresh`` must be >= 0."""
    pred, B, A = _pred_side('detect', pred, anchors, num_classes, score_thresh, scales=scales, shifts=shifts)
    if out is not None:
        _check_det_out(out, B, int(keep_top_k), pred.device)
    bufs = out if out is not None else _det_buffers(B, keep_top_k, pred.device, A)
    if len(bufs) == 5:
        bufs = tuple(bufs) + (_det_workspace(B, A, pred.device),)
    cnt, cls, sc, bx, idx, keys = bufs
    if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32 or keys.device != pred.device:
        raise ValueError('detect: workspace must be an int32 tensor on the same device')
    if keys.numel() < det_workspace_words(B, A) or not keys.is_contiguous():
        keys = None                                  # (a caller-made placeholder: one workgroup per image)
    if keys_ready and (keys is None or keys.data_ptr() % 16):
        raise ValueError('detect: keys_ready needs the 16-byte aligned workspace the keys were written to')
    entry = 'sqd_detect_keys_fwd' if keys_ready else 'sqd_detect_shift_fwd'
    br = _Bracket('detect', f'detect A{A}', 0.0, 4.0 * B * A * (num_classes + 5)) if timing._timer is not None else None
    rc = getattr(nat.lib(), entry)(nat.ptr(pred), nat.ptr(anchors.contiguous()), nat.ptr(scales), nat.ptr(shifts), nat.ptr(keys),
                                   nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, A, num_classes,
                                   int(input_size[0]), int(input_size[1]), int(keep_top_k), float(nms_thresh), float(score_thresh),
                                   nat.stream_handle(pred.device))
    nat.check(rc, entry)
    if br is not None:
        br.done()
    return bufs[:5]


def filter_dense(class_ids, scores, boxes, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3):
    """``Detector.filter`` on already decoded dense tensors ([B,A] / [B,A,4]).  ``score_thresh`` must be >= 0."""
    B, A = _dense_side('filter', class_ids, scores, boxes, num_classes, score_thresh)
    bufs = _det_buffers(B, keep_top_k, scores.device, A)
    cnt, cls, sc, bx, idx, keys = bufs
    rc = nat.lib().sqd_filter_fwd(nat.ptr(class_ids.contiguous()), nat.ptr(scores.contiguous()), nat.ptr(boxes.contiguous()),
                                  nat.ptr(keys), nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, A, num_classes,
                                  int(keep_top_k), float(nms_thresh), float(score_thresh), nat.stream_handle(scores.device))
    nat.check(rc, 'sqd_filter_fwd')
    return bufs[:5]


def detect_wide(pred, anchors, input_size, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, scales=None, out=None, shifts=None):
    """``detect`` for any 1 <= ``keep_top_k`` <= 1024 and up to 2^20 anchors (two launches: score into a workspace, then one
    workgroup per image selects, suppresses and compacts); same arguments, same results bit for bit where both run.  ``out``: the
    five result tensors and optionally a workspace of ``det_workspace_words_wide(B, A, keep_top_k)`` int32 (any contents)."""
    return _detect_wide('sqd_detect_wide_fwd', pred, anchors, input_size, num_classes, keep_top_k, nms_thresh, score_thresh, scales, out, shifts)


def _detect_wide(_entry, pred, anchors, input_size, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, scales=None, out=None, shifts=None):
    pred, B, A = _pred_side('detect_wide', pred, anchors, num_classes, score_thresh, keep_top_k, scales, shifts)
    K = int(keep_top_k)
    bufs, keys = _wide_out('detect_wide', out, B, A, K, pred.device)
    cnt, cls, sc, bx, idx = bufs[:5]
    br = _Bracket('detect', f'{_entry[4:-4]} A{A} K{K}', 0.0, 4.0 * B * A * (num_classes + 5)) if timing._timer is not None else None
    rc = getattr(nat.lib(), _entry)(nat.ptr(pred), nat.ptr(anchors.contiguous()), nat.ptr(scales), nat.ptr(shifts), nat.ptr(keys),
                                    nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, A, num_classes,
                                    int(input_size[0]), int(input_size[1]), K, float(nms_thresh), float(score_thresh),
                                    keys.numel(), nat.stream_handle(pred.device))
    nat.check(rc, _entry)
    if br is not None:
        br.done()
    return bufs[:5]


def detect_many(pred, anchors, input_size, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, scales=None, out=None, shifts=None):
    """``detect_wide`` for 1 <= num_classes <= 256: every 1 <= ``keep_top_k`` <= 1024 and up to 2^20 anchors, same arguments, same
    workspace size.  Equals ``Detector.filter`` on ``decode_many``'s output bit for bit."""
    head_path(num_classes)
    return _detect_wide('sqd_detect_many_fwd', pred, anchors, input_size, num_classes, keep_top_k, nms_thresh, score_thresh, scales, out, shifts)


def filter_dense_wide(class_ids, scores, boxes, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3):
    """``filter_dense`` for any 1 <= ``keep_top_k`` <= 1024 and up to 2^20 anchors."""
    return _filter_dense_wide('sqd_filter_wide_fwd', class_ids, scores, boxes, num_classes, keep_top_k, nms_thresh, score_thresh)


def _filter_dense_wide(_entry, class_ids, scores, boxes, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3):
    B, A = _dense_side('filter_wide', class_ids, scores, boxes, num_classes, score_thresh, keep_top_k)
    K = int(keep_top_k)
    bufs, keys = _wide_out('filter_wide', None, B, A, K, scores.device)
    cnt, cls, sc, bx, idx = bufs
    rc = getattr(nat.lib(), _entry)(nat.ptr(class_ids.contiguous()), nat.ptr(scores.contiguous()), nat.ptr(boxes.contiguous()),
                                    nat.ptr(keys), nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, A, num_classes,
                                    K, float(nms_thresh), float(score_thresh), keys.numel(), nat.stream_handle(scores.device))
    nat.check(rc, _entry)
    return bufs


def filter_dense_many(class_ids, scores, boxes, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3):
    """``filter_dense_wide`` for class ids up to 255 (1 <= num_classes <= 256)."""
    head_path(num_classes)
    return _filter_dense_wide('sqd_filter_many_fwd', class_ids, scores, boxes, num_classes, keep_top_k, nms_thresh, score_thresh)


NMS_MODES = ('hard', 'linear', 'gaussian')               # cfg.nms_mode; the index is the C ABI's nms_mode


def nms_mode_index(name, nms_mode, nms_sigma=0.5, nms_agnostic=False):
    """(C ABI mode, sigma, agnostic as int) of a suppression rule; ValueError for an unknown mode, a sigma that is not a finite number
    > 0 (checked in every mode, read by 'gaussian' only) or an agnostic flag that is not a bool."""
    if not isinstance(nms_mode, str) or nms_mode not in NMS_MODES:
        raise ValueError(f'{name}: nms_mode must be one of {NMS_MODES}, got {nms_mode!r}')
    try:
        sigma = float(nms_sigma)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: nms_sigma must be a finite number > 0, got {nms_sigma!r}') from None
    if isinstance(nms_sigma, bool) or not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f'{name}: nms_sigma must be a finite number > 0, got {nms_sigma!r}')
    if not isinstance(nms_agnostic, bool) and type(nms_agnostic).__name__ != 'bool_':
        raise ValueError(f'{name}: nms_agnostic must be a bool, got {nms_agnostic!r}')
    return NMS_MODES.index(nms_mode), sigma, int(bool(nms_agnostic))


def check_vote_iou(name, vote_iou):
    """``vote_iou`` of box voting: None (off) or a finite number in (0, 1], not a bool -> None or the float; ValueError otherwise."""
    if vote_iou is None:
        return None
    try:
        v = float(vote_iou)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: vote_iou must be None or a finite number in (0, 1], got {vote_iou!r}') from None
    if type(vote_iou).__name__ in ('bool', 'bool_') or not (math.isfinite(v) and 0.0 < v <= 1.0):
        raise ValueError(f'{name}: vote_iou must be None or a finite number in (0, 1], got {vote_iou!r}')
    return v


def _votes_out(vote, return_votes, B, K, device):
    """The int32 [B, K] voter counts of a launch, where asked for: zeros for the voting launch to fill (rows past count stay 0), ones
    without voting (every row is its own only voter)."""
    if not return_votes:
        return None
    return (torch.zeros if vote is not None else torch.ones)(B, K, device=device, dtype=torch.int32)


def detect_nms(pred, anchors, input_size, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, scales=None, out=None, shifts=None,
               nms_mode='hard', nms_sigma=0.5, nms_agnostic=False, keys_ready=False, vote_iou=None, return_votes=False):
    """``detect_wide`` / ``detect_many`` (any 1 <= ``keep_top_k`` <= 1024, up to 2^20 anchors, 1 <= ``num_classes`` <= 256) with the
    suppression rule as an argument: ``nms_mode`` 'hard' | 'linear' | 'gaussian' (Soft-NMS: an overlapped box keeps a decayed score
    -- times 1 - IoU where IoU > ``nms_thresh``, or times exp(-IoU^2 / ``nms_sigma``) -- instead of being deleted), ``nms_agnostic``:
    one suppression group for all classes.  Rows come out in class order (agnostic: one group), each group in pick order, ``scores``
    holding the decayed score; rows whose score fell to ``score_thresh`` or below are gone.  ('hard', False) equals ``detect_wide`` /
    ``detect_many`` bit for bit.  ``keys_ready`` (<= 16 classes): the workspace in ``out`` already holds the keys of this ``pred`` for
    this ``score_thresh`` (``DetKeys``) -- no scoring launch.
    ``vote_iou`` (None: off; else in (0, 1]): box voting (DESIGN.md section 3 "Box voting") -- the rows, their order, classes, scores and
    ``anchor_idx`` stay those of the same call without it; every emitted box becomes the mean, weighted by the original scores, of the
    same-class candidates that overlap it by IoU >= ``vote_iou`` (itself included; suppressed candidates vote too).
    ``return_votes``: an int32 [B,K] tensor with each row's number of voters is appended to the returned tuple."""
    mode, sigma, agnostic = nms_mode_index('detect_nms', nms_mode, nms_sigma, nms_agnostic)
    vote = check_vote_iou('detect_nms', vote_iou)
    pred, B, A = _pred_side('detect_nms', pred, anchors, num_classes, score_thresh, keep_top_k, scales, shifts, many=True)
    K = int(keep_top_k)
    bufs, keys = _wide_out('detect_nms', out, B, A, K, pred.device)
    if keys_ready and (len(bufs) != 6 or keys is not bufs[5] or head_path(num_classes) != 'narrow'):
        raise ValueError('detect_nms: keys_ready needs the 16-byte aligned workspace the keys were written to (<= 16 classes)')
    cnt, cls, sc, bx, idx = bufs[:5]
    votes = _votes_out(vote, return_votes, B, K, pred.device)
    br = _Bracket('detect', f'detect_nms A{A} K{K}', 0.0, 4.0 * B * A * (num_classes + 5)) if timing._timer is not None else None
    entry = 'sqd_detect_nms_fwd' if vote is None else 'sqd_detect_vote_fwd'
    rc = getattr(nat.lib(), entry)(nat.ptr(pred), nat.ptr(anchors.contiguous()), nat.ptr(scales), nat.ptr(shifts), nat.ptr(keys),
                                   nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, A, num_classes,
                                   int(input_size[0]), int(input_size[1]), K, float(nms_thresh), float(score_thresh),
                                   keys.numel(), mode, sigma, agnostic, int(bool(keys_ready)),
                                   *(() if vote is None else (vote, nat.ptr(votes))), nat.stream_handle(pred.device))
    nat.check(rc, entry)
    if br is not None:
        br.done()
    return tuple(bufs[:5]) + ((votes,) if return_votes else ())


DET_VIEWS_MAX_ROW = 1 << 20    # key words of one pooled row, V * ceil4(A): the wide select's row limit


def detect_views(pred, anchors, input_size, num_classes, V, view_xf, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, out=None,
                 nms_mode='hard', nms_sigma=0.5, nms_agnostic=False, vote_iou=None, return_votes=False):
    """Pooled-view fused detect (DESIGN.md section 3 "Pooled views"): ``pred`` [B*V, A, C+5] holds ``V`` network views of each of B
    images (view v of image b = row b*V + v), ``view_xf`` fp32 [B*V, 6] = (sy, sx, dy, dx, flip, mirror) maps a row's canvas boxes
    into its image -- ``x / sx + dx``, ``y / sy + dy``, then, where ``flip`` != 0, ``(x1, x2) <- (mirror - x2, mirror - x1)`` -- and the
    candidates of an image's views meet in ONE top-``keep_top_k`` (score descending, ties to the lower view, then the lower anchor)
    and ONE suppression (the rule of ``detect_nms``) on the image-coordinate boxes.  Returns (count int32 [B], class_ids int64 [B,K],
    scores [B,K], boxes [B,K,4] in image coordinates, pooled_idx int32 [B,K] = v * A + anchor).  ``out``: the five result tensors
    (checked against B and ``keep_top_k``) and optionally a workspace of ``det_workspace_words_wide(B*V, A, keep_top_k)`` int32.
    ``V`` = 1 with ``view_xf`` = (1, 1, 0, 0, 0, 0) equals ``detect_nms`` bit for bit.  Limits: ``V * ceil4(A) <= 2^20``, K <= 1024,
    1 <= ``num_classes`` <= 256.  ``vote_iou`` / ``return_votes``: box voting as in ``detect_nms``, on the image-coordinate boxes -- the
    near-duplicate boxes the views give of one object are merged instead of dropped; a row seen by one view only has few voters."""
    mode, sigma, agnostic = nms_mode_index('detect_views', nms_mode, nms_sigma, nms_agnostic)
    vote = check_vote_iou('detect_views', vote_iou)
    pred, B, A = _pred_side('detect_views', pred, anchors, num_classes, score_thresh, keep_top_k, many=True, V=V)
    V, K, rows = int(V), int(keep_top_k), pred.shape[0]
    if not isinstance(view_xf, torch.Tensor) or tuple(view_xf.shape) != (rows, 6) or view_xf.dtype != torch.float32 \
            or view_xf.device != pred.device or not view_xf.is_contiguous():
        raise ValueError('detect_views: view_xf must be contiguous fp32 [B*V,6] (sy, sx, dy, dx, flip, mirror) on the same device')
    bufs, keys = _wide_out('detect_views', out, B, A, K, pred.device, rows=rows)
    cnt, cls, sc, bx, idx = bufs[:5]
    votes = _votes_out(vote, return_votes, B, K, pred.device)
    br = _Bracket('detect', f'detect_views V{V} A{A} K{K}', 0.0, 4.0 * rows * A * (num_classes + 5)) if timing._timer is not None else None
    entry = 'sqd_detect_views_fwd' if vote is None else 'sqd_detect_views_vote_fwd'
    rc = getattr(nat.lib(), entry)(nat.ptr(pred), nat.ptr(anchors.contiguous()), nat.ptr(view_xf), nat.ptr(keys), nat.ptr(cnt),
                                   nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, V, A, num_classes,
                                   int(input_size[0]), int(input_size[1]), K, float(nms_thresh), float(score_thresh),
                                   keys.numel(), mode, sigma, agnostic, *(() if vote is None else (vote, nat.ptr(votes))),
                                   nat.stream_handle(pred.device))
    nat.check(rc, entry)
    if br is not None:
        br.done()
    return tuple(bufs[:5]) + ((votes,) if return_votes else ())


def filter_dense_nms(class_ids, scores, boxes, num_classes, keep_top_k=64, nms_thresh=0.4, score_thresh=0.3, out=None,
                     nms_mode='hard', nms_sigma=0.5, nms_agnostic=False, vote_iou=None, return_votes=False):
    """``filter_dense_wide`` / ``filter_dense_many`` with the suppression rule of ``detect_nms``.  ``out``: the five result tensors
    (checked against B and ``keep_top_k``) and optionally a workspace of ``det_workspace_words_wide`` int32.  ``vote_iou`` /
    ``return_votes``: box voting as in ``detect_nms``."""
    mode, sigma, agnostic = nms_mode_index('filter_nms', nms_mode, nms_sigma, nms_agnostic)
    vote = check_vote_iou('filter_nms', vote_iou)
    B, A = _dense_side('filter_nms', class_ids, scores, boxes, num_classes, score_thresh, keep_top_k, many=True)
    K = int(keep_top_k)
    bufs, keys = _wide_out('filter_nms', out, B, A, K, scores.device)
    cnt, cls, sc, bx, idx = bufs[:5]
    votes = _votes_out(vote, return_votes, B, K, scores.device)
    entry = 'sqd_filter_nms_fwd' if vote is None else 'sqd_filter_vote_fwd'
    rc = getattr(nat.lib(), entry)(nat.ptr(class_ids.contiguous()), nat.ptr(scores.contiguous()), nat.ptr(boxes.contiguous()),
                                   nat.ptr(keys), nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(idx), B, A, num_classes,
                                   K, float(nms_thresh), float(score_thresh), keys.numel(), mode, sigma, agnostic, 0,
                                   *(() if vote is None else (vote, nat.ptr(votes))), nat.stream_handle(scores.device))
    nat.check(rc, entry)
    return tuple(bufs[:5]) + ((votes,) if return_votes else ())


def detect_fn(num_classes, keep_top_k, A, nms_mode='hard', nms_agnostic=False, nms_sigma=0.5, vote_iou=None):
    """The fused detect that serves (num_classes, keep_top_k, A): ``detect`` / ``detect_wide`` up to 16 classes (``detect_path``),
    ``detect_many`` past them.  Any rule but ('hard', class-wise): ``detect_nms`` with the rule bound, for every K, A and class count.
    ``vote_iou`` set (box voting): ``detect_nms`` with the rule and ``vote_iou`` bound, under every rule."""
    nms_mode_index('detect_fn', nms_mode, nms_sigma, nms_agnostic)
    vote = check_vote_iou('detect_fn', vote_iou)
    if vote is not None:
        head_path(num_classes)
        detect_path(keep_top_k, A)
        return functools.partial(detect_nms, nms_mode=nms_mode, nms_sigma=float(nms_sigma), nms_agnostic=bool(nms_agnostic), vote_iou=vote)
    if nms_mode != 'hard' or nms_agnostic:
        head_path(num_classes)
        detect_path(keep_top_k, A)
        return functools.partial(detect_nms, nms_mode=nms_mode, nms_sigma=float(nms_sigma), nms_agnostic=bool(nms_agnostic))
    if head_path(num_classes) == 'many':
        detect_path(keep_top_k, A)
        return detect_many
    return detect if detect_path(keep_top_k, A) == 'narrow' else detect_wide


def filter_fn(num_classes, keep_top_k, A, nms_mode='hard', nms_agnostic=False, nms_sigma=0.5, vote_iou=None):
    """The dense filter that serves (num_classes, keep_top_k, A), the rule and ``vote_iou``, as ``detect_fn``."""
    nms_mode_index('filter_fn', nms_mode, nms_sigma, nms_agnostic)
    vote = check_vote_iou('filter_fn', vote_iou)
    if vote is not None:
        head_path(num_classes)
        detect_path(keep_top_k, A)
        return functools.partial(filter_dense_nms, nms_mode=nms_mode, nms_sigma=float(nms_sigma), nms_agnostic=bool(nms_agnostic),
                                 vote_iou=vote)
    if nms_mode != 'hard' or nms_agnostic:
        head_path(num_classes)
        detect_path(keep_top_k, A)
        return functools.partial(filter_dense_nms, nms_mode=nms_mode, nms_sigma=float(nms_sigma), nms_agnostic=bool(nms_agnostic))
    if head_path(num_classes) == 'many':
        detect_path(keep_top_k, A)
        return filter_dense_many
    return filter_dense if detect_path(keep_top_k, A) == 'narrow' else filter_dense_wide


def conv_wgrad(dy, dy_coff, N, x, x_coff, C, taps, slab=None, wino=None):
    """(dW OIHW [N,C,k,k], db [N]) from dy[..., dy_coff:dy_coff+N] (already ReLU-masked) and
    x[..., x_coff:x_coff+C].  With ``slab`` (a workspace view of S * stride floats, see ``WgradBatch``) only the partial
    slabs are written and None is returned: the caller reduces all layers with one launch."""
    _check_nhwc(dy, 'dy'); _check_nhwc(x, 'x')
    B, H, W, dyp = dy.shape
    if tuple(x.shape[:3]) != (B, H, W):
        raise ValueError('wgrad: dy and x disagree on B,H,W')
    xp = x.shape[3]
    if dy_coff + N > dyp or x_coff + C > xp or N % 4 or C % 4 or taps not in (1, 9):
        raise ValueError('wgrad: channel window out of range')
    k = 3 if taps == 9 else 1
    use_wino = wgrad_uses_wino(N, C, taps, B, H, W, wino)
    S, stride = wgrad_split(N, C, taps, B, H, W, wino)
    deferred = slab is not None
    if deferred:
        if slab.numel() != S * stride or not slab.is_contiguous() or slab.dtype != torch.float32:
            raise ValueError('wgrad: slab workspace does not match this layer')
        dw = db = None
    else:
        slab = torch.empty(S * stride, device=dy.device, dtype=torch.float32)
        dw = torch.empty(N, C, k, k, device=dy.device, dtype=torch.float32)
        db = torch.empty(N, device=dy.device, dtype=torch.float32)
    if use_wino:
        # executed multiply-adds = direct form / 2.25 (16 position GEMMs per 2x2 tile)
        br = _Bracket('conv_wgrad_wino', f'wgrad 9tap C{C} N{N} {H}x{W}', 2.0 * B * H * W * N * C * 4,
                      4.0 * (B * H * W * (C + N) + 2 * S * stride)) if timing._timer is not None else None
        rc = nat.lib().sqd_conv_wgrad_wino(nat.ptr(dy), nat.ptr(x), nat.ptr(slab), nat.ptr(dw), nat.ptr(db), B, H, W, N, dyp, dy_coff,
                                           C, xp, x_coff, S, _wino_wgrad_tc(N, C), nat.stream_handle(dy.device))
        nat.check(rc, 'sqd_conv_wgrad_wino')
    else:
        br = _Bracket(f'conv_wgrad<{taps}>', f'wgrad {taps}tap C{C} N{N} {H}x{W}', 2.0 * B * H * W * N * C * taps,
                      4.0 * (B * H * W * (C + N) + 2 * S * stride)) if timing._timer is not None else None
        rc = nat.lib().sqd_conv_wgrad(nat.ptr(dy), nat.ptr(x), nat.ptr(slab), nat.ptr(dw), nat.ptr(db), B, H, W, N, dyp, dy_coff,
                                      C, xp, x_coff, taps, S, nat.stream_handle(dy.device))
        nat.check(rc, 'sqd_conv_wgrad')
    if br is not None:
        br.done()
    return None if deferred else (dw, db)


def conv_wgrad_wino_group(items, S, tc):
    """The Winograd weight-gradient slabs of several 3x3 layers of one backward stage in ONE launch (``tiles.wino_wgrad_groups``
    decides which).  ``items``: [(dy, dy_coff, N, x, x_coff, C, slab)] with dy / x NHWC on the same [B,H,W] grid; ``slab`` = the layer's
    ``WgradBatch`` view of S * (N*9*C + N) floats.  Every layer is cut into the same ``S`` splits; slabs only (the batched reduction
    follows)."""
    if not 1 <= len(items) <= WINO_WGRAD_GROUP_MAX:
        raise ValueError('grouped weight gradient: 1..%d layers' % WINO_WGRAD_GROUP_MAX)
    B, H, W = items[0][0].shape[:3]
    rows, flops, byts, tag = [], 0.0, 0.0, []
    for dy, dy_coff, N, x, x_coff, C, slab in items:
        _check_nhwc(dy, 'dy'); _check_nhwc(x, 'x')
        if tuple(dy.shape[:3]) != (B, H, W) or tuple(x.shape[:3]) != (B, H, W):
            raise ValueError('grouped weight gradient: the layers of a group share B,H,W')
        if dy_coff + N > dy.shape[3] or x_coff + C > x.shape[3] or N % 64 or C % 4 or _wino_wgrad_tc(N, C) != tc:
            raise ValueError('grouped weight gradient: channel window out of range / wrong tile form')
        if slab.numel() != S * (N * 9 * C + N) or not slab.is_contiguous() or slab.dtype != torch.float32:
            raise ValueError('grouped weight gradient: slab workspace does not match the layer')
        rows += [dy.data_ptr(), x.data_ptr(), slab.data_ptr(), N, dy.shape[3], dy_coff, C, x.shape[3], x_coff]
        flops += 2.0 * B * H * W * N * C * 4
        byts += 4.0 * (B * H * W * (C + N) + 2 * S * (N * 9 * C + N))
        tag.append(f'C{C} N{N}')
    table = (ctypes.c_longlong * len(rows))(*rows)
    br = _Bracket('conv_wgrad_wino_group', f'wgrad 9tap {" + ".join(tag)} {H}x{W}', flops, byts) if timing._timer is not None else None
    rc = nat.lib().sqd_conv_wgrad_wino_group(ctypes.cast(table, ctypes.c_void_p), len(items), B, H, W, int(S), int(tc),
                                             nat.stream_handle(items[0][0].device))
    nat.check(rc, 'sqd_conv_wgrad_wino_group')
    if br is not None:
        br.done()


def conv_wgrad_group(items, S):
    """The direct 1x1 weight-gradient slabs of several layers of one pixel grid in ONE launch (``tiles.wgrad1x1_groups`` decides which).
    ``items`` as ``conv_wgrad_wino_group``; ``slab`` = the layer's ``WgradBatch`` view of S * (N*C + N) floats."""
    if not 1 <= len(items) <= WINO_WGRAD_GROUP_MAX:
        raise ValueError('grouped weight gradient: 1..%d layers' % WINO_WGRAD_GROUP_MAX)
    B, H, W = items[0][0].shape[:3]
    rows, flops, byts, tag = [], 0.0, 0.0, []
    for dy, dy_coff, N, x, x_coff, C, slab in items:
        _check_nhwc(dy, 'dy'); _check_nhwc(x, 'x')
        if tuple(dy.shape[:3]) != (B, H, W) or tuple(x.shape[:3]) != (B, H, W):
            raise ValueError('grouped weight gradient: the layers of a group share B,H,W')
        if dy_coff + N > dy.shape[3] or x_coff + C > x.shape[3] or N % 4 or C % 4:
            raise ValueError('grouped weight gradient: channel window out of range')
        if slab.numel() != S * (N * C + N) or not slab.is_contiguous() or slab.dtype != torch.float32:
            raise ValueError('grouped weight gradient: slab workspace does not match the layer')
        rows += [dy.data_ptr(), x.data_ptr(), slab.data_ptr(), N, dy.shape[3], dy_coff, C, x.shape[3], x_coff]
        flops += 2.0 * B * H * W * N * C
        byts += 4.0 * (B * H * W * (C + N) + 2 * S * (N * C + N))
        tag.append(f'C{C} N{N}')
    table = (ctypes.c_longlong * len(rows))(*rows)
    br = _Bracket('conv_wgrad_group<1>', f'wgrad 1tap {" + ".join(tag)} {H}x{W}', flops, byts) if timing._timer is not None else None
    rc = nat.lib().sqd_conv_wgrad_group(ctypes.cast(table, ctypes.c_void_p), len(items), B, H, W, int(S), nat.stream_handle(items[0][0].device))
    nat.check(rc, 'sqd_conv_wgrad_group')
    if br is not None:
        br.done()


def squeeze_bwd_ok(N, C):
    """Whether ``squeeze_bwd`` can run a (C -> N) 1x1 layer: all N out-channels in one group."""
    return N % 4 == 0 and C % 4 == 0 and N <= 128


def squeeze_bwd(dy, x, weight, slab, dx, relu_mask, dy_coff=0, N=None):
    """A 1x1 layer's backward in ONE launch: the weight / bias gradient slabs (as ``conv_wgrad(..., slab=...)`` writes them; ``slab``
    from a ``WgradBatch`` entry flagged fused) and the data gradient dx = dy . W, zeroed where ``relu_mask`` and x <= 0.  dy [B,H,W,.]
    (already masked; channel window ``[dy_coff, dy_coff + N)``, default all of it), x / dx [B,H,W,C], weight: the layer's OIHW
    [N,C,1,1] parameter.  Fire.squeeze (relu_mask = the previous layer is a Fire) and, where N <= 128, Fire.expand1x1 (dy = the
    expand1x1 window of the Fire output's gradient, x = the squeeze output, relu_mask False)."""
    _check_nhwc(dy, 'dy'); _check_nhwc(x, 'x'); _check_nhwc(dx, 'dx')
    B, H, W, dyp = dy.shape
    N = dyp - dy_coff if N is None else int(N)
    if dy_coff < 0 or dy_coff % 4 or dy_coff + N > dyp:
        raise ValueError('squeeze_bwd: dy channel window out of range')
    C = x.shape[3]
    if tuple(x.shape[:3]) != (B, H, W) or tuple(dx.shape) != tuple(x.shape):
        raise ValueError('squeeze_bwd: dy, x and dx disagree on B,H,W / C')
    if tuple(weight.shape) != (N, C, 1, 1) or weight.dtype != torch.float32 or not weight.is_cuda or not weight.is_contiguous():
        raise ValueError(f'squeeze_bwd: weight must be a contiguous fp32 CUDA [N,C,1,1] tensor, got {tuple(weight.shape)}')
    if not squeeze_bwd_ok(N, C):
        raise ValueError(f'squeeze_bwd: unsupported layer C={C} N={N}')
    S, stride = wgrad_split(N, C, 1, B, H, W, fused_dgrad=True)
    if slab.numel() != S * stride or not slab.is_contiguous() or slab.dtype != torch.float32:
        raise ValueError('squeeze_bwd: slab workspace does not match this layer')
    npix = B * H * W
    br = _Bracket('squeeze_bwd', f'sqbwd C{C} N{N} {H}x{W}', 4.0 * npix * N * C,
                  4.0 * (npix * (2 * C + N) + N * C + 2 * S * stride)) if timing._timer is not None else None
    rc = nat.lib().sqd_squeeze_bwd(nat.ptr(dy), nat.ptr(x), nat.ptr(weight.detach()), nat.ptr(slab), nat.ptr(dx), B, H, W, N, dyp, dy_coff, C, C, 0,
                                   C, 0, int(bool(relu_mask)), S, nat.stream_handle(dy.device))
    nat.check(rc, 'sqd_squeeze_bwd')
    if br is not None:
        br.done()
    return dx


def _check_stem_out(dw, db, N, ksize):
    if tuple(dw.shape) != (N, 3, ksize, ksize) or tuple(db.shape) != (N,) or not dw.is_contiguous() or not db.is_contiguous() \
            or dw.dtype != torch.float32 or db.dtype != torch.float32:
        raise ValueError('stem wgrad: out=(dw, db) must be contiguous fp32 [N,3,k,k] / [N]')


def _stem_wgrad_buffers(B, Ho, Wo, N, ksize, device, out):
    """-> (S, slab, dw, db): the split-K workspace of a stem weight gradient (one slab per conv tile of 8 x 16 pixels, at most 1024)
    and its checked outputs."""
    S = max(1, min(B * -(-Ho // 8) * -(-Wo // 16), 1024))
    slab = torch.empty(S * (N * 3 * ksize * ksize + N), device=device, dtype=torch.float32)
    dw, db = out if out is not None else (torch.empty(N, 3, ksize, ksize, device=device, dtype=torch.float32),
                                          torch.empty(N, device=device, dtype=torch.float32))
    _check_stem_out(dw, db, N, ksize)
    return S, slab, dw, db


def stem_wgrad(dy, image, N, ksize, out=None):
    """(dW [N,3,k,k], db [N]) of the stem from dy NHWC [B,Ho,Wo,N] (ReLU-masked) and the NCHW image."""
    _check_nhwc(dy, 'dy')
    B, Ho, Wo, n = dy.shape
    if n != N or image.dim() != 4 or image.shape[0] != B or image.shape[1] != 3 or not image.is_contiguous():
        raise ValueError('stem_wgrad: geometry mismatch')
    H, W = image.shape[2], image.shape[3]
    if stem_out_size(H, W, ksize) != (Ho, Wo) or (ksize, N) not in _STEMS:
        raise ValueError('stem_wgrad: unsupported geometry')
    K = 3 * ksize * ksize
    S, slab, dw, db = _stem_wgrad_buffers(B, Ho, Wo, N, ksize, dy.device, out)
    br = _Bracket(f'stem_wgrad<{ksize}>', f'stem wgrad {H}x{W}', 2.0 * B * Ho * Wo * N * K,
                  4.0 * (B * Ho * Wo * N + B * 3 * H * W)) if timing._timer is not None else None
    rc = nat.lib().sqd_stem_wgrad(nat.ptr(dy), nat.ptr(image), nat.ptr(slab), nat.ptr(dw), nat.ptr(db), B, H, W, N, ksize, S,
                                  nat.stream_handle(dy.device))
    nat.check(rc, 'sqd_stem_wgrad')
    if br is not None:
        br.done()
    return dw, db


def stem_wgrad_pooled(dpool, pooled, argmax, image, N, ksize, out=None):
    """Stem (dW, db) when the forward ran fused (stem_pool with argmax): ReLU + max-pool backward folded in.  ``pooled`` may be
    None: the forward's arg-max codes carry the ReLU mask (15 = pooled value 0)."""
    _check_nhwc(dpool, 'dpool')
    if pooled is not None:
        _check_nhwc(pooled, 'pooled')
    B, Hp, Wp, n = dpool.shape
    if n != N or (pooled is not None and tuple(pooled.shape) != (B, Hp, Wp, N)) or tuple(argmax.shape) != (B, Hp, Wp, N) \
            or argmax.dtype != torch.uint8 or not argmax.is_contiguous():
        raise ValueError('stem_wgrad_pooled: dpool / pooled / argmax geometry mismatch')
    if image.dim() != 4 or image.shape[0] != B or image.shape[1] != 3 or not image.is_contiguous():
        raise ValueError('stem_wgrad_pooled: bad image')
    H, W = image.shape[2], image.shape[3]
    Ho, Wo = stem_out_size(H, W, ksize)
    if pool_out_size(Ho, Wo) != (Hp, Wp) or (ksize, N) not in _STEMS:
        raise ValueError('stem_wgrad_pooled: unsupported geometry')
    K = 3 * ksize * ksize
    S, slab, dw, db = _stem_wgrad_buffers(B, Ho, Wo, N, ksize, dpool.device, out)
    br = _Bracket(f'stem_wgrad_pooled<{ksize}>', f'stem wgrad (pooled) {H}x{W}', 2.0 * B * Ho * Wo * N * K,
                  4.0 * (B * Hp * Wp * N * (2.25 if pooled is not None else 1.25) + B * 3 * H * W)) if timing._timer is not None else None
    rc = nat.lib().sqd_stem_wgrad_pooled(nat.ptr(dpool), nat.ptr(pooled), nat.ptr(argmax), nat.ptr(image), nat.ptr(slab), nat.ptr(dw),
                                         nat.ptr(db), B, H, W, N, ksize, S, nat.stream_handle(dpool.device))
    nat.check(rc, 'sqd_stem_wgrad_pooled')
    if br is not None:
        br.done()
    return dw, db


def _check_loss_args(pred, gt, anchors, num_classes):
    if pred.dim() != 3 or pred.shape[2] != num_classes + 5 or pred.dtype != torch.float32 or not pred.is_cuda:
        raise ValueError(f'loss: bad pred {tuple(pred.shape)}')
    B, A, _ = pred.shape
    if tuple(gt.shape) != (B, A, num_classes + 9) or gt.dtype != torch.float32 or gt.device != pred.device:
        raise ValueError(f'loss: gt must be fp32 [B,A,C+9] on the same device, got {tuple(gt.shape)}')
    if tuple(anchors.shape) != (A, 4) or anchors.dtype != torch.float32 or anchors.device != pred.device:
        raise ValueError('loss: anchors must be fp32 [A,4] on the same device')
    return B, A


BOX_LOSSES = ('l2', 'iou', 'giou', 'diou', 'ciou')      # cfg.bbox_loss; the index is the C ABI's SQD_BOX_*


def box_loss_kind(name, box_loss):
    """``box_loss`` (one of ``BOX_LOSSES``) -> SQD_BOX_*; checked before anything is launched."""
    if not isinstance(box_loss, str) or box_loss not in BOX_LOSSES:
        raise ValueError(f'{name}: box_loss must be one of {BOX_LOSSES}, got {box_loss!r}')
    return BOX_LOSSES.index(box_loss)


def split_loss_weights(name, weights):
    """The ``weights`` argument of every ``loss_*`` wrapper: (w_class, w_pos, w_neg, w_bbox), optionally followed by the box-loss
    kind (one of ``BOX_LOSSES``; absent: 'l2', the squared error on the deltas).  -> (the four weights, SQD_BOX_*)."""
    weights = tuple(weights)
    if len(weights) == 5:
        return weights[:4], box_loss_kind(name, weights[4])
    if len(weights) != 4:
        raise ValueError(f'{name}: weights must be (w_class, w_pos, w_neg, w_bbox[, box_loss]), got {len(weights)} values')
    return weights, 0


def _box_entry(kind):
    """The sqd_loss_box_* entry of a launch-record kind ('loss_fwd', 'loss_sparse_bwd', ...): one per family and pass."""
    return 'sqd_' + kind.replace('loss_', 'loss_box_', 1)


def _run_loss_fwd(entry, pred, mid, anchors, lead, B, A, num_classes, input_size, weights, ws_width, count_rows, mean, kind, nbytes):
    """What the eight forward wrappers do once their operands are checked.  ``mid``: the contiguous tensors between pred and anchors
    in the entry's argument list (gt, or the five list members, then the bitmap); ``lead``: the integers in front of B (``total`` of
    the sparse entries); ``ws_width``: partial sums per block (5, masked 6); ``count_rows``: () for nobj [B], (2,) for counts [2,B];
    ``mean``: the entry also takes mean4 [4]; ``nbytes(B, A, *lead, num_classes)``: the bracket's bytes, asked only when a timer
    runs; ``weights`` with a box-loss kind other than 'l2' (``split_loss_weights``): the family's sqd_loss_box_* entry (same
    operands, records and bytes).  -> (losses, nobj or counts[, mean4])."""
    weights, box = split_loss_weights(entry, weights)
    pred, anchors = pred.contiguous(), anchors.contiguous()
    ws = torch.empty(B * 16 * ws_width, device=pred.device, dtype=torch.float32)
    out = [torch.empty(4, B, device=pred.device, dtype=torch.float32), torch.empty(*count_rows, B, device=pred.device, dtype=torch.float32)]
    if mean:
        out.append(torch.empty(4, device=pred.device, dtype=torch.float32))
    br = _Bracket(kind, f'loss A{A}', 0.0, nbytes(B, A, *lead, num_classes)) if timing._timer is not None else None
    entry = _box_entry(kind) if box else entry
    fn = getattr(nat.lib(), entry)
    tail = (*lead, B, A, num_classes, int(input_size[0]), int(input_size[1]), *[float(w) for w in weights], nat.stream_handle(pred.device))
    if box:
        rc = fn(nat.ptr(pred), *[nat.ptr(t) for t in mid], nat.ptr(anchors), nat.ptr(ws), nat.ptr(out[0]), nat.ptr(out[1]),
                nat.ptr(out[2] if mean else None), box, *tail)
    else:
        rc = fn(nat.ptr(pred), *[nat.ptr(t) for t in mid], nat.ptr(anchors), nat.ptr(ws), *[nat.ptr(t) for t in out], *tail)
    nat.check(rc, entry)
    if br is not None:
        br.done()
    return tuple(out)


def _run_loss_bwd(entry, pred, mid, anchors, counts, upstream, out, lead, B, A, num_classes, input_size, weights, kind, nbytes):
    """What the eight backward wrappers do once their operands are checked: ``mid`` / ``lead`` / ``nbytes`` as for ``_run_loss_fwd``; ``counts``:
    the forward's nobj or counts; ``upstream``: coef or gmean, whichever the entry takes; ``out``: a checked tensor to write, or None
    for a new one; ``weights`` with a box-loss kind other than 'l2': the family's sqd_loss_box_* entry, which takes coef and gmean
    side by side (the one ``entry`` does not take is null).  -> dpred."""
    weights, box = split_loss_weights(entry, weights)
    pred, anchors = pred.contiguous(), anchors.contiguous()
    dpred = torch.empty_like(pred) if out is None else out
    br = _Bracket(kind, f'lossbwd A{A}', 0.0, nbytes(B, A, *lead, num_classes)) if timing._timer is not None else None
    gmean = 'mean' in entry
    entry = _box_entry(kind) if box else entry
    fn = getattr(nat.lib(), entry)
    tail = (*lead, B, A, num_classes, int(input_size[0]), int(input_size[1]), *[float(w) for w in weights], nat.stream_handle(pred.device))
    if box:
        rc = fn(nat.ptr(pred), *[nat.ptr(t) for t in mid], nat.ptr(anchors), nat.ptr(counts), nat.ptr(None if gmean else upstream),
                nat.ptr(upstream if gmean else None), nat.ptr(dpred), box, *tail)
    else:
        rc = fn(nat.ptr(pred), *[nat.ptr(t) for t in mid], nat.ptr(anchors), nat.ptr(counts), nat.ptr(upstream), nat.ptr(dpred), *tail)
    nat.check(rc, entry)
    if br is not None:
        br.done()
    return dpred


# The upstream operands of the backward wrappers.  The three families grew their checks apart; each keeps what it accepts and the
# words it raises (``name``: the wrapper, ``msg``: its text): the dense wrappers look at shapes only and take any object that has
# one, the sparse ones add dtype and device, the masked ones also refuse what is no tensor.
def _check_coef(name, coef, B, pred, msg, tensor=False, device=True):
    """coef [3,B] -> contiguous fp32."""
    if (tensor and not isinstance(coef, torch.Tensor)) or tuple(coef.shape) != (3, B) or (device and coef.device != pred.device):
        raise ValueError(f'{name}: {msg}')
    return coef.contiguous().float()


def _check_gmean(name, gmean, pred, tensor=False):
    """gmean: one fp32 value on the device of pred -> contiguous."""
    if (tensor and not isinstance(gmean, torch.Tensor)) or gmean.numel() != 1 or gmean.dtype != torch.float32 or gmean.device != pred.device:
        raise ValueError(f'{name}: gmean must be one fp32 value on the same device')
    return gmean.contiguous()


def _check_nobj(name, nobj, shape, pred, msg, tensor=False, kind=True):
    """The forward's nobj [B] or counts [2,B] (``shape``); ``kind``: fp32 on the device of pred -> contiguous."""
    if (tensor and not isinstance(nobj, torch.Tensor)) or tuple(nobj.shape) != shape \
            or (kind and (nobj.dtype != torch.float32 or nobj.device != pred.device)):
        raise ValueError(f'{name}: {msg}')
    return nobj.contiguous() if kind else nobj


def _dense_fwd_bytes(B, A, num_classes):
    return 4.0 * B * A * (2 * num_classes + 14)


def _dense_bwd_bytes(B, A, num_classes):
    return 4.0 * B * A * (3 * num_classes + 19)


def _loss_fwd(_entry, mean, pred, gt, anchors, input_size, num_classes, weights):
    B, A = _check_loss_args(pred, gt, anchors, num_classes)
    return _run_loss_fwd(_entry, pred, [gt.contiguous()], anchors, (), B, A, num_classes, input_size, weights, 5, (), mean,
                         'loss_fwd', _dense_fwd_bytes)


def _loss_bwd(_entry, pred, gt, anchors, nobj, coef, input_size, num_classes, weights):
    B, A = _check_loss_args(pred, gt, anchors, num_classes)
    msg = 'coef must be [3,B], nobj [B]'
    coef = _check_coef('loss_bwd', coef, B, pred, msg, device=False)
    nobj = _check_nobj('loss_bwd', nobj, (B,), pred, msg, kind=False)
    return _run_loss_bwd(_entry, pred, [gt.contiguous()], anchors, nobj, coef, None, (), B, A, num_classes, input_size, weights,
                         'loss_bwd', _dense_bwd_bytes)


def _loss_mean_bwd(_entry, pred, gt, anchors, nobj, gmean, input_size, num_classes, weights):
    B, A = _check_loss_args(pred, gt, anchors, num_classes)
    gmean = _check_gmean('loss_mean_bwd', gmean, pred)                 # (nobj goes to the entry as it came)
    return _run_loss_bwd(_entry, pred, [gt.contiguous()], anchors, nobj, gmean, None, (), B, A, num_classes, input_size, weights,
                         'loss_bwd', _dense_bwd_bytes)


def loss_fwd(pred, gt, anchors, input_size, num_classes, weights):
    """-> (losses [4,B] = class, score, bbox, total; nobj [B])."""
    return _loss_fwd('sqd_loss_fwd', False, pred, gt, anchors, input_size, num_classes, weights)


def loss_mean_fwd(pred, gt, anchors, input_size, num_classes, weights):
    """-> (losses [4,B], nobj [B], mean4 [4] = batch means of class / score / bbox / total): ``loss.mean()`` inside the loss launches."""
    return _loss_fwd('sqd_loss_mean_fwd', True, pred, gt, anchors, input_size, num_classes, weights)


def loss_mean_bwd(pred, gt, anchors, nobj, gmean, input_size, num_classes, weights):
    """gmean: device scalar (gradient arriving at mean(total)) -> dpred [B,A,C+5]."""
    return _loss_mean_bwd('sqd_loss_mean_bwd', pred, gt, anchors, nobj, gmean, input_size, num_classes, weights)


def loss_bwd(pred, gt, anchors, nobj, coef, input_size, num_classes, weights):
    """coef [3,B] -> dpred [B,A,C+5]."""
    return _loss_bwd('sqd_loss_bwd', pred, gt, anchors, nobj, coef, input_size, num_classes, weights)


def loss_fwd_many(pred, gt, anchors, input_size, num_classes, weights):
    """``loss_fwd`` for 1 <= num_classes <= 256 (a 16-lane group per anchor row)."""
    head_path(num_classes)
    return _loss_fwd('sqd_loss_many_fwd', False, pred, gt, anchors, input_size, num_classes, weights)


def loss_mean_fwd_many(pred, gt, anchors, input_size, num_classes, weights):
    """``loss_mean_fwd`` for 1 <= num_classes <= 256; the per-image values equal ``loss_fwd_many``'s bit for bit."""
    head_path(num_classes)
    return _loss_fwd('sqd_loss_many_mean_fwd', True, pred, gt, anchors, input_size, num_classes, weights)


def loss_mean_bwd_many(pred, gt, anchors, nobj, gmean, input_size, num_classes, weights):
    """``loss_mean_bwd`` for 1 <= num_classes <= 256."""
    head_path(num_classes)
    return _loss_mean_bwd('sqd_loss_many_mean_bwd', pred, gt, anchors, nobj, gmean, input_size, num_classes, weights)


def loss_bwd_many(pred, gt, anchors, nobj, coef, input_size, num_classes, weights):
    """``loss_bwd`` for 1 <= num_classes <= 256."""
    head_path(num_classes)
    return _loss_bwd('sqd_loss_many_bwd', pred, gt, anchors, nobj, coef, input_size, num_classes, weights)


def loss_fns(num_classes):
    """(loss_fwd, loss_mean_fwd, loss_bwd, loss_mean_bwd) that serve ``num_classes`` (``head_path``)."""
    if head_path(num_classes) == 'many':
        return loss_fwd_many, loss_mean_fwd_many, loss_bwd_many, loss_mean_bwd_many
    return loss_fwd, loss_mean_fwd, loss_bwd, loss_mean_bwd


class SparseGT(NamedTuple):
    """The ground truth of a batch of B images as the list of its positives (device tensors): what the dense ``gt [B,A,C+9]``
    holds outside its all-zero rows.  ``anchor_idx`` int32 [total]: the anchor each box was assigned; ``boxes`` fp32 [total,4]: xyxy in
    network-input coordinates (dense columns 1..4); ``deltas`` fp32 [total,4] (dense columns 5..8); ``class_ids`` int32 [total];
    ``offsets`` int32 [B+1]: image b owns the entries ``offsets[b] .. offsets[b+1]``.  Meaning: the dense gt with mask = 1, these boxes
    and deltas and a one-hot class at ``anchor_idx``, zeros elsewhere.

    Contract (include/sqd_hip.h): within one image the anchor indices are distinct (the encoder's greedy assignment guarantees it, and
    ``anchor_match`` keeps it: an extra positive is never a primary and appears once); the order within an image is free; an entry with ``anchor_idx`` outside [0, A) -- the encoder's "unassigned" value A -- is ignored
    and does not count toward n_obj; a class id outside [0, C) gives a row with no class term, as the dense encoder does; ``total = 0``
    and images without entries are legal and give the NaNs that n_obj = 0 gives with a dense gt."""
    anchor_idx: torch.Tensor
    boxes: torch.Tensor
    deltas: torch.Tensor
    class_ids: torch.Tensor
    offsets: torch.Tensor

    def to(self, device, non_blocking=False):
        return SparseGT(*(t.to(device=device, non_blocking=non_blocking) for t in self))


def sparse_gt_from_dense(gt):
    """Dense gt [B,A,C+9] -> SparseGT (torch only; tests and conversions): the rows with ``gt[..., 0] > 0`` in ascending anchor
    order, class = arg-max of the one-hot."""
    if gt.dim() != 3 or gt.shape[2] < 10:
        raise ValueError(f'sparse_gt_from_dense: gt must be [B,A,C+9], got {tuple(gt.shape)}')
    B = gt.shape[0]
    pos = gt[..., 0] > 0
    b_idx, a_idx = torch.nonzero(pos, as_tuple=True)          # row-major: ascending image, then ascending anchor
    rows = gt[b_idx, a_idx]
    offsets = torch.zeros(B + 1, dtype=torch.int32, device=gt.device)
    offsets[1:] = torch.cumsum(pos.sum(1), 0).to(torch.int32)
    cls = rows[:, 9:].argmax(1).to(torch.int32) if rows.shape[0] else torch.zeros(0, dtype=torch.int32, device=gt.device)
    return SparseGT(a_idx.to(torch.int32), rows[:, 1:5].float().contiguous(), rows[:, 5:9].float().contiguous(), cls, offsets)


def sparse_gt_to_dense(sgt, A, C):
    """SparseGT -> the dense gt fp32 [B,A,C+9] it stands for (torch only): entries with ``anchor_idx`` outside [0, A) are dropped, a
    class id outside [0, C) leaves the row's one-hot empty."""
    B = sgt.offsets.shape[0] - 1
    dev = sgt.offsets.device
    gt = torch.zeros(B, A, C + 9, dtype=torch.float32, device=dev)
    counts = (sgt.offsets[1:] - sgt.offsets[:-1]).long()
    img = torch.repeat_interleave(torch.arange(B, device=dev), counts)
    idx = sgt.anchor_idx.long()
    keep = (idx >= 0) & (idx < A)
    img, idx = img[keep], idx[keep]
    gt[img, idx, 0] = 1.0
    gt[img, idx, 1:5] = sgt.boxes[keep]
    gt[img, idx, 5:9] = sgt.deltas[keep]
    cls = sgt.class_ids.long()[keep]
    ok = (cls >= 0) & (cls < C)
    gt[img[ok], idx[ok], 9 + cls[ok]] = 1.0
    return gt


def _check_sparse_loss_args(name, pred, sgt, anchors, num_classes):
    """Everything the sparse launches assume about their operands, before the library is touched: kinds and shapes first, devices
    last.  -> (B, A, total, sgt with contiguous members)."""
    head_path(num_classes)
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3 or pred.shape[2] != num_classes + 5 or pred.dtype != torch.float32:
        raise ValueError(f'{name}: pred must be fp32 [B,A,C+5]')
    B, A, _ = pred.shape
    if A > 2 ** 20:
        raise ValueError(f'{name}: at most 2^20 anchors, got {A}')
    if not isinstance(sgt, SparseGT):
        raise ValueError(f'{name}: sgt must be an ops.SparseGT')
    fields = ((sgt.anchor_idx, 'anchor_idx', torch.int32), (sgt.boxes, 'boxes', torch.float32), (sgt.deltas, 'deltas', torch.float32),
              (sgt.class_ids, 'class_ids', torch.int32), (sgt.offsets, 'offsets', torch.int32))
    for t, nm, dt in fields:
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f'{name}: sgt.{nm} must be a {dt} tensor')
    if tuple(sgt.offsets.shape) != (B + 1,):
        raise ValueError(f'{name}: sgt.offsets must be [B+1] = [{B + 1}], got {tuple(sgt.offsets.shape)}')
    total = sgt.anchor_idx.shape[0] if sgt.anchor_idx.dim() == 1 else -1
    if total < 0 or tuple(sgt.boxes.shape) != (total, 4) or tuple(sgt.deltas.shape) != (total, 4) or tuple(sgt.class_ids.shape) != (total,):
        raise ValueError(f'{name}: anchor_idx [total], boxes [total,4], deltas [total,4], class_ids [total] must agree on total, got '
                         f'{tuple(sgt.anchor_idx.shape)} {tuple(sgt.boxes.shape)} {tuple(sgt.deltas.shape)} {tuple(sgt.class_ids.shape)}')
    if not isinstance(anchors, torch.Tensor) or tuple(anchors.shape) != (A, 4) or anchors.dtype != torch.float32:
        raise ValueError(f'{name}: anchors must be fp32 [A,4]')
    if not pred.is_cuda:
        raise ValueError(f'{name}: pred must be on the GPU, got {pred.device}')
    for t, nm in [(t, 'sgt.' + nm) for t, nm, _ in fields] + [(anchors, 'anchors')]:
        if t.device != pred.device:
            raise ValueError(f'{name}: {nm} is on {t.device}, pred on {pred.device}')
    return B, A, total, SparseGT(*(t.contiguous() for t in sgt))


def _sparse_fwd_bytes(B, A, total, num_classes):
    """Bytes the sparse forward reads: one confidence logit per row, the list once per slice of an image, a positive's pred row,
    box, deltas and anchor."""
    return 4.0 * (B * A + 16 * total + total * (num_classes + 5 + 13))


def loss_sparse_fwd(pred, sgt, anchors, input_size, num_classes, weights):
    """``loss_fwd`` on a sparse ground truth (``SparseGT``), 1 <= num_classes <= 256: -> (losses [4,B], nobj [B]).  A negative row
    costs one float of ``pred``; the dense gt is never read or built."""
    B, A, total, sgt = _check_sparse_loss_args('loss_sparse_fwd', pred, sgt, anchors, num_classes)
    return _run_loss_fwd('sqd_loss_sparse_fwd', pred, sgt, anchors, (total,), B, A, num_classes, input_size, weights, 5, (), False,
                         'loss_sparse_fwd', _sparse_fwd_bytes)


def loss_sparse_mean_fwd(pred, sgt, anchors, input_size, num_classes, weights):
    """``loss_mean_fwd`` on a sparse ground truth: -> (losses [4,B], nobj [B], mean4 [4]); the per-image values equal
    ``loss_sparse_fwd``'s bit for bit."""
    B, A, total, sgt = _check_sparse_loss_args('loss_sparse_mean_fwd', pred, sgt, anchors, num_classes)
    return _run_loss_fwd('sqd_loss_sparse_mean_fwd', pred, sgt, anchors, (total,), B, A, num_classes, input_size, weights, 5, (), True,
                         'loss_sparse_fwd', _sparse_fwd_bytes)


def _sparse_bwd_bytes(B, A, total, num_classes):
    """Bytes the sparse backward moves: all of dpred written, one confidence logit per row and a positive's operands read, the
    list once per workgroup of an image."""
    return 4.0 * (B * A * (num_classes + 5) + B * A + -(-A // 256) * total + total * (num_classes + 5 + 13))


def loss_sparse_bwd(pred, sgt, anchors, nobj, coef, input_size, num_classes, weights):
    """``loss_bwd`` on a sparse ground truth: coef [3,B] -> dpred [B,A,C+5] (dense: ConvDet's backward reads it whole)."""
    B, A, total, sgt = _check_sparse_loss_args('loss_sparse_bwd', pred, sgt, anchors, num_classes)
    msg = 'coef must be [3,B], nobj fp32 [B], both on the device of pred'
    coef = _check_coef('loss_sparse_bwd', coef, B, pred, msg)
    nobj = _check_nobj('loss_sparse_bwd', nobj, (B,), pred, msg)
    return _run_loss_bwd('sqd_loss_sparse_bwd', pred, sgt, anchors, nobj, coef, None, (total,), B, A, num_classes, input_size, weights,
                         'loss_sparse_bwd', _sparse_bwd_bytes)


def loss_sparse_mean_bwd(pred, sgt, anchors, nobj, gmean, input_size, num_classes, weights):
    """``loss_mean_bwd`` on a sparse ground truth: gmean, a device scalar (the gradient arriving at mean(total)) -> dpred [B,A,C+5]."""
    B, A, total, sgt = _check_sparse_loss_args('loss_sparse_mean_bwd', pred, sgt, anchors, num_classes)
    gmean = _check_gmean('loss_sparse_mean_bwd', gmean, pred)
    nobj = _check_nobj('loss_sparse_mean_bwd', nobj, (B,), pred, 'nobj must be fp32 [B] on the device of pred')
    return _run_loss_bwd('sqd_loss_sparse_mean_bwd', pred, sgt, anchors, nobj, gmean, None, (total,), B, A, num_classes, input_size,
                         weights, 'loss_sparse_bwd', _sparse_bwd_bytes)


def ignore_words(A):
    """Words per image of an anchor ignore bitmap: anchor a is bit ``a & 31`` of word ``a >> 5``."""
    return (int(A) + 31) // 32


def check_ignore_overlap(name, overlap):
    """``overlap`` as a float in (0, 1] (``cfg.ignore_overlap`` when it is set)."""
    try:
        v = float(overlap)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: ignore overlap must be a number in (0, 1], got {overlap!r}') from None
    if not (v > 0.0 and v <= 1.0):              # (NaN fails both)
        raise ValueError(f'{name}: ignore overlap must be in (0, 1], got {overlap!r}')
    return v


def anchor_ignore_mask(ign_boxes, ign_offsets, anchors64, overlap, out=None):
    """The anchors that lie on an ignore region (KITTI ``DontCare``, VOC ``difficult``, COCO ``crowd``): ign_boxes fp32 [total,4] xyxy in
    network-input coordinates, ign_offsets int32 [B+1], anchors64 float64 [A,4] (cx,cy,w,h), all on the GPU -> int32 [B, ceil(A/32)],
    bit ``a & 31`` of word ``a >> 5`` set iff ``inter >= overlap * area(anchor) > 0`` for some box of the image (float64, the rule of
    ``boxes.anchor_ignore_mask``, bit for bit).  ``total = 0`` and images without boxes give zero words.  One launch, every word
    written (``out``: a contiguous int32 [B, ceil(A/32)] device tensor to write instead; it needs no clearing), nothing waits."""
    overlap = check_ignore_overlap('anchor_ignore_mask', overlap)
    if not isinstance(ign_boxes, torch.Tensor) or ign_boxes.dtype != torch.float32 or ign_boxes.dim() != 2 or ign_boxes.shape[1] != 4:
        raise ValueError('anchor_ignore_mask: ign_boxes must be fp32 [total,4]')
    if not isinstance(ign_offsets, torch.Tensor) or ign_offsets.dtype != torch.int32 or ign_offsets.dim() != 1 or ign_offsets.shape[0] < 2:
        raise ValueError('anchor_ignore_mask: ign_offsets must be int32 [B+1], B >= 1')
    if not isinstance(anchors64, torch.Tensor) or anchors64.dtype != torch.float64 or anchors64.dim() != 2 or anchors64.shape[1] != 4 \
            or anchors64.shape[0] < 1:
        raise ValueError('anchor_ignore_mask: anchors must be float64 [A,4]')
    B, A, total = ign_offsets.shape[0] - 1, anchors64.shape[0], ign_boxes.shape[0]
    if A > 2 ** 20 or B > 65535 or total > 65535 * B:
        raise ValueError(f'anchor_ignore_mask: at most 2^20 anchors, 65535 images and 65535 ignore boxes per image, got A={A} B={B} total={total}')
    if not anchors64.is_cuda:
        raise ValueError(f'anchor_ignore_mask: anchors must be on the GPU, got {anchors64.device}')
    for t, nm in ((ign_boxes, 'ign_boxes'), (ign_offsets, 'ign_offsets')):
        if t.device != anchors64.device:
            raise ValueError(f'anchor_ignore_mask: {nm} is on {t.device}, anchors on {anchors64.device}')
    ign_boxes, ign_offsets, anchors64 = ign_boxes.contiguous(), ign_offsets.contiguous(), anchors64.contiguous()
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or tuple(out.shape) != (B, ignore_words(A))
                            or out.device != anchors64.device or not out.is_contiguous()):
        raise ValueError(f'anchor_ignore_mask: out must be a contiguous int32 [{B}, {ignore_words(A)}] tensor on the device of the anchors')
    mask = torch.empty(B, ignore_words(A), device=anchors64.device, dtype=torch.int32) if out is None else out
    br = _Bracket('anchor_ignore', f'ignore A{A}', 0.0, 32.0 * A + 16.0 * total + 4.0 * mask.numel()) if timing._timer is not None else None
    rc = nat.lib().sqd_anchor_ignore_fwd(nat.ptr(ign_boxes) if total else None, nat.ptr(ign_offsets), nat.ptr(anchors64), nat.ptr(mask),
                                         ctypes.byref(ctypes.c_double(overlap)), int(total), B, A, nat.stream_handle(anchors64.device))
    nat.check(rc, 'sqd_anchor_ignore_fwd')
    if br is not None:
        br.done()
    return mask


def anchor_match(sgt, anchors64, pos_iou, ign_iou, max_extra, ignore=None, out=None):
    """IoU-threshold anchor matching on top of the encoder's greedy assignment (csrc/gt_encode.hip; rule: DESIGN.md section 3,
    "IoU-threshold matching", and ``boxes.anchor_match``, its host twin): ``sgt``, the ``SparseGT`` of the encoder (one entry per box:
    the primaries), anchors64 float64 [A,4] (cx,cy,w,h), ``0 < ign_iou <= pos_iou <= 1`` (``ign_iou`` None: no band), ``max_extra``
    >= 0, ``ignore``: the int32 [B, ceil(A/32)] bitmap of ``anchor_ignore_mask`` or None -- all on the GPU.

    -> (SparseGT of ``total + B * max_extra`` entries, ignore int32 [B, ceil(A/32)], overflow int32 [B]).  Image b's segment starts at
    ``sgt.offsets[b] + b * max_extra``: its primaries, then the anchors that are no primaries and overlap some box by ``pos_iou`` or more
    (the first ``max_extra`` by ascending anchor index; box and class of the lowest best-overlapping box), then padding entries
    (``anchor_idx`` A, which the loss skips).  ``ignore`` out = the given bits | the band (best overlap in [ign_iou, pos_iou)) | the
    overflow (extras past ``max_extra``, counted per image in ``overflow``).  Two launches, every element written, nothing waits.
    ``out``: (SparseGT, ignore, overflow) of contiguous device tensors of those shapes to write instead (they need no clearing)."""
    from .boxes import check_match_thresholds
    pos_iou, ign_iou, max_extra = check_match_thresholds('anchor_match', pos_iou, ign_iou, max_extra)
    if not isinstance(sgt, SparseGT):
        raise ValueError('anchor_match: sgt must be an ops.SparseGT (the encoder\'s list)')
    fields = ((sgt.anchor_idx, 'anchor_idx', torch.int32), (sgt.boxes, 'boxes', torch.float32), (sgt.deltas, 'deltas', torch.float32),
              (sgt.class_ids, 'class_ids', torch.int32), (sgt.offsets, 'offsets', torch.int32))
    for t, nm, dt in fields:
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f'anchor_match: sgt.{nm} must be a {dt} tensor')
    if sgt.offsets.dim() != 1 or sgt.offsets.shape[0] < 2:
        raise ValueError('anchor_match: sgt.offsets must be int32 [B+1], B >= 1')
    total = sgt.anchor_idx.shape[0] if sgt.anchor_idx.dim() == 1 else -1
    if total < 0 or tuple(sgt.boxes.shape) != (total, 4) or tuple(sgt.deltas.shape) != (total, 4) or tuple(sgt.class_ids.shape) != (total,):
        raise ValueError('anchor_match: anchor_idx [total], boxes [total,4], deltas [total,4], class_ids [total] must agree on total')
    if not isinstance(anchors64, torch.Tensor) or anchors64.dtype != torch.float64 or anchors64.dim() != 2 or anchors64.shape[1] != 4 \
            or anchors64.shape[0] < 1:
        raise ValueError('anchor_match: anchors must be float64 [A,4]')
    B, A = sgt.offsets.shape[0] - 1, anchors64.shape[0]
    out_total = total + B * max_extra
    if A > 2 ** 20 or B > 65535 or out_total >= 2 ** 31:
        raise ValueError(f'anchor_match: at most 2^20 anchors, 65535 images and 2^31 - 1 output entries, got A={A} B={B} '
                         f'total + B * max_extra = {out_total}')
    if ignore is not None and (not isinstance(ignore, torch.Tensor) or ignore.dtype != torch.int32 or tuple(ignore.shape) != (B, ignore_words(A))):
        raise ValueError(f'anchor_match: ignore must be int32 [B, ceil(A/32)] = [{B}, {ignore_words(A)}] (ops.anchor_ignore_mask) or None')
    if not anchors64.is_cuda:
        raise ValueError(f'anchor_match: anchors must be on the GPU, got {anchors64.device}')
    dev = anchors64.device
    for t, nm in [(t, 'sgt.' + nm) for t, nm, _ in fields] + ([(ignore, 'ignore')] if ignore is not None else []):
        if t.device != dev:
            raise ValueError(f'anchor_match: {nm} is on {t.device}, anchors on {dev}')
    sgt = SparseGT(*(t.contiguous() for t in sgt))
    anchors64 = anchors64.contiguous()
    ignore = None if ignore is None else ignore.contiguous()
    shapes = (((out_total,), torch.int32), ((out_total, 4), torch.float32), ((out_total, 4), torch.float32), ((out_total,), torch.int32),
              ((B + 1,), torch.int32), ((B, ignore_words(A)), torch.int32), ((B,), torch.int32))
    if out is None:
        flat = [torch.empty(*s, device=dev, dtype=dt) for s, dt in shapes]
    else:
        flat = [*out[0], out[1], out[2]] if isinstance(out, (tuple, list)) and len(out) == 3 and isinstance(out[0], SparseGT) else []
        if len(flat) != 7 or any(not isinstance(t, torch.Tensor) or tuple(t.shape) != s or t.dtype != dt or t.device != dev or not t.is_contiguous()
                                 for t, (s, dt) in zip(flat, shapes)):
            raise ValueError(f'anchor_match: out must be (SparseGT of {out_total} entries and offsets [{B + 1}], int32 [{B}, {ignore_words(A)}], '
                             f'int32 [{B}]), contiguous, on the device of the anchors')
    out, mask, overflow = SparseGT(*flat[:5]), flat[5], flat[6]
    ws = torch.empty(B * (A + -(-A // 256)), device=dev, dtype=torch.int32)      # best box per anchor, extras per 256-anchor block
    br = _Bracket('anchor_match', f'match A{A}', 0.0, 32.0 * A + B * (16.0 * A + 8.0 * ignore_words(A)) + 80.0 * out_total) \
        if timing._timer is not None else None
    rc = nat.lib().sqd_anchor_match_fwd(
        nat.ptr(sgt.boxes) if total else None, nat.ptr(sgt.class_ids) if total else None, nat.ptr(sgt.offsets),
        nat.ptr(sgt.anchor_idx) if total else None, nat.ptr(sgt.deltas) if total else None, nat.ptr(anchors64), nat.ptr(ignore),
        (ctypes.c_double * 2)(pos_iou, ign_iou), nat.ptr(ws), nat.ptr(out.anchor_idx) if out_total else None,
        nat.ptr(out.boxes) if out_total else None, nat.ptr(out.deltas) if out_total else None,
        nat.ptr(out.class_ids) if out_total else None, nat.ptr(out.offsets), nat.ptr(mask), nat.ptr(overflow), int(total), B, A, max_extra,
        nat.stream_handle(dev))
    nat.check(rc, 'sqd_anchor_match_fwd')
    if br is not None:
        br.done()
    return out, mask, overflow


def _check_masked_loss_args(name, pred, sgt, ignore, anchors, num_classes):
    """``_check_sparse_loss_args`` + the bitmap: int32 [B, ceil(A/32)] on the device of pred.  -> (B, A, total, sgt, ignore)."""
    if not isinstance(pred, torch.Tensor) or pred.dim() != 3:
        raise ValueError(f'{name}: pred must be fp32 [B,A,C+5]')
    B, A = pred.shape[:2]                               # (kinds and shapes first, devices last: the bitmap before the list's devices)
    if not isinstance(ignore, torch.Tensor) or ignore.dtype != torch.int32 or tuple(ignore.shape) != (B, ignore_words(A)):
        raise ValueError(f'{name}: ignore must be int32 [B, ceil(A/32)] = [{B}, {ignore_words(A)}] (ops.anchor_ignore_mask), got '
                         f'{getattr(ignore, "dtype", type(ignore))} {tuple(getattr(ignore, "shape", ()))}')
    B, A, total, sgt = _check_sparse_loss_args(name, pred, sgt, anchors, num_classes)
    if ignore.device != pred.device:
        raise ValueError(f'{name}: ignore is on {ignore.device}, pred on {pred.device}')
    return B, A, total, sgt, ignore.contiguous()


_COUNTS_MSG = 'counts must be fp32 [2,B] = (n_obj, n_neg) on the device of pred'


def _masked_fwd_bytes(B, A, total, num_classes):
    return _sparse_fwd_bytes(B, A, total, num_classes) + B * A / 8.0          # (+ the bitmap)


def _masked_bwd_bytes(B, A, total, num_classes):
    return _sparse_bwd_bytes(B, A, total, num_classes) + B * A / 8.0


def loss_masked_fwd(pred, sgt, ignore, anchors, input_size, num_classes, weights):
    """``loss_sparse_fwd`` with an anchor ignore bitmap (``anchor_ignore_mask``): -> (losses [4,B], counts [2,B] = (n_obj, n_neg)).
    An anchor whose bit is set and that is no positive is neither a positive nor a negative; class / pos / bbox are 0 where
    n_obj = 0 and neg is 0 where n_neg = 0, so an object-free image gives finite values."""
    B, A, total, sgt, ignore = _check_masked_loss_args('loss_masked_fwd', pred, sgt, ignore, anchors, num_classes)
    return _run_loss_fwd('sqd_loss_masked_fwd', pred, [*sgt, ignore], anchors, (total,), B, A, num_classes, input_size, weights, 6, (2,),
                         False, 'loss_masked_fwd', _masked_fwd_bytes)


def loss_masked_mean_fwd(pred, sgt, ignore, anchors, input_size, num_classes, weights):
    """``loss_masked_fwd`` + the batch means: -> (losses [4,B], counts [2,B], mean4 [4]); the per-image values equal
    ``loss_masked_fwd``'s bit for bit."""
    B, A, total, sgt, ignore = _check_masked_loss_args('loss_masked_mean_fwd', pred, sgt, ignore, anchors, num_classes)
    return _run_loss_fwd('sqd_loss_masked_mean_fwd', pred, [*sgt, ignore], anchors, (total,), B, A, num_classes, input_size, weights, 6,
                         (2,), True, 'loss_masked_fwd', _masked_fwd_bytes)


def loss_masked_bwd(pred, sgt, ignore, anchors, counts, coef, input_size, num_classes, weights, out=None):
    """``loss_sparse_bwd`` with the bitmap: coef [3,B], counts [2,B] of the masked forward -> dpred [B,A,C+5], every element written
    (an ignored row that is no positive: zeros).  ``out``: a fp32 [B,A,C+5] device tensor with contiguous strides to write instead
    (any storage offset)."""
    B, A, total, sgt, ignore = _check_masked_loss_args('loss_masked_bwd', pred, sgt, ignore, anchors, num_classes)
    counts = _check_nobj('loss_masked_bwd', counts, (2, B), pred, _COUNTS_MSG, tensor=True)
    coef = _check_coef('loss_masked_bwd', coef, B, pred, 'coef must be [3,B] on the device of pred', tensor=True)
    out = _check_dpred_out('loss_masked_bwd', pred, out)
    return _run_loss_bwd('sqd_loss_masked_bwd', pred, [*sgt, ignore], anchors, counts, coef, out, (total,), B, A, num_classes, input_size,
                         weights, 'loss_masked_bwd', _masked_bwd_bytes)


def loss_masked_mean_bwd(pred, sgt, ignore, anchors, counts, gmean, input_size, num_classes, weights, out=None):
    """``loss_sparse_mean_bwd`` with the bitmap: gmean, a device scalar (the gradient arriving at mean(total)) -> dpred [B,A,C+5]."""
    B, A, total, sgt, ignore = _check_masked_loss_args('loss_masked_mean_bwd', pred, sgt, ignore, anchors, num_classes)
    counts = _check_nobj('loss_masked_mean_bwd', counts, (2, B), pred, _COUNTS_MSG, tensor=True)
    gmean = _check_gmean('loss_masked_mean_bwd', gmean, pred, tensor=True)
    out = _check_dpred_out('loss_masked_mean_bwd', pred, out)
    return _run_loss_bwd('sqd_loss_masked_mean_bwd', pred, [*sgt, ignore], anchors, counts, gmean, out, (total,), B, A, num_classes,
                         input_size, weights, 'loss_masked_bwd', _masked_bwd_bytes)


def _check_dpred_out(name, pred, out):
    """``out`` of the masked backward wrappers: None (a new tensor), or what the launch may write in its place."""
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.shape != pred.shape
                            or out.device != pred.device or not out.is_contiguous()):
        raise ValueError(f'{name}: out must be a contiguous fp32 {tuple(pred.shape)} tensor on the device of pred')
    return out


def encode_gt(boxes, class_ids, box_offsets, anchors64, num_classes, dense=True, parallel=True):
    """On-device GT encoding (compute_deltas + prepare_annotations, src/utils/boxes.py:84-135,
    src/datasets/base.py:61-76).  boxes [total,4] fp32 xyxy, class_ids [total] i32, box_offsets [B+1] i32,
    anchors64 [A,4] float64 -- all on the GPU.  -> (gt [B,A,C+9] or None, anchor_idx [total] i32, deltas [total,4])."""
    if boxes.dtype != torch.float32 or class_ids.dtype != torch.int32 or box_offsets.dtype != torch.int32:
        raise ValueError('encode_gt: boxes must be float32, class_ids / box_offsets int32')
    if anchors64.dtype != torch.float64 or anchors64.dim() != 2 or anchors64.shape[1] != 4:
        raise ValueError('encode_gt: anchors must be float64 [A,4] (the reference matches anchors in float64)')
    if boxes.dim() != 2 or boxes.shape[1] != 4 or class_ids.shape[0] != boxes.shape[0] or box_offsets.dim() != 1:
        raise ValueError('encode_gt: boxes [total,4], class_ids [total], box_offsets [B+1]')
    B, A, total = box_offsets.shape[0] - 1, anchors64.shape[0], boxes.shape[0]
    if B < 1:
        raise ValueError('encode_gt: empty batch')
    boxes, class_ids, box_offsets, anchors64 = boxes.contiguous(), class_ids.contiguous(), box_offsets.contiguous(), anchors64.contiguous()
    dev = boxes.device
    gt = torch.empty(B, A, num_classes + 9, device=dev, dtype=torch.float32) if dense else None
    if total == 0 and not dense:                   # nothing to assign and nothing to zero: no launch
        return None, torch.empty(0, device=dev, dtype=torch.int32), torch.empty(0, 4, device=dev, dtype=torch.float32)
    idx = torch.empty(max(total, 1), device=dev, dtype=torch.int32)
    deltas = torch.empty(max(total, 1), 4, device=dev, dtype=torch.float32)
    br = _Bracket('encode_gt', f'gt A{A}', 0.0, 4.0 * B * A * (num_classes + 9)) if timing._timer is not None else None
    ws = torch.empty(max(total, 1) * 2, device=dev, dtype=torch.float64)       # 16 bytes per box: first-choice candidates
    rc = nat.lib().sqd_encode_gt_fwd(nat.ptr(boxes) if total else None, nat.ptr(class_ids) if total else nat.ptr(idx),
                                     nat.ptr(box_offsets), nat.ptr(anchors64), nat.ptr(gt) if dense else None, nat.ptr(idx),
                                     nat.ptr(deltas), nat.ptr(ws) if (total and parallel) else None, int(total), B, A,
                                     int(num_classes), nat.stream_handle(dev))
    nat.check(rc, 'sqd_encode_gt_fwd')
    if br is not None:
        br.done()
    return gt, idx[:total], deltas[:total]


def image_stats_u8(dev_buf, B, hdr, out=None):
    """Exact per-image, per-channel pixel sums of a packed uint8 upload (``augment.pack_layout`` / ``write_header``: int64 offsets [B],
    int32 sizes [B, 2], then at ``hdr`` the HWC RGB pixels) that lives on the device as ``dev_buf``.  -> int64 [B, 3, 2] on the device
    = (sum x, sum x*x) per image and channel (the kernel's uint64 bit pattern: below 2^63 for any image under 1.4e14 pixels).
    ``out``: a contiguous int64 [B, 3, 2] device tensor to write instead (a slice of a table, say).  One launch, nothing waits."""
    B, hdr = int(B), int(hdr)
    if dev_buf.dtype != torch.uint8 or dev_buf.dim() != 1 or not dev_buf.is_contiguous() or not dev_buf.is_cuda:
        raise ValueError('image_stats_u8: dev_buf must be a contiguous 1-D uint8 tensor on the device')
    if B < 1 or hdr < 16 * B or hdr > dev_buf.numel():
        raise ValueError(f'image_stats_u8: B = {B}, header {hdr} bytes do not fit a buffer of {dev_buf.numel()} bytes')
    dev = dev_buf.device
    if out is None:
        out = torch.empty(B, 3, 2, device=dev, dtype=torch.int64)
    elif tuple(out.shape) != (B, 3, 2) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev:
        raise ValueError('image_stats_u8: out must be a contiguous int64 [B, 3, 2] tensor on the device of dev_buf')
    br = _Bracket('image_stats_u8', f'stats B{B}', 0.0, float(dev_buf.numel() - hdr) + 48.0 * B) if timing._timer is not None else None
    base = dev_buf.data_ptr()
    rc = nat.lib().sqd_image_stats_u8(ctypes.c_void_p(base + hdr), ctypes.c_void_p(base), ctypes.c_void_p(base + 8 * B), nat.ptr(out), B,
                                      nat.stream_handle(dev))
    nat.check(rc, 'sqd_image_stats_u8')
    if br is not None:
        br.done()
    return out


DET_EVAL_MAX_T = 16            # det_match / det_ap: one lane per IoU threshold, a uint16 claim per (detection, threshold)
DET_EVAL_MAX_CLASSES = 256
DET_EVAL_MAX_K = 1024
DET_EVAL_MAX_GT = 65535        # per image: claims are uint16 indices within the image
AP_MODES = {'area': 0, '11point': 1, '101point': 2}


def _check_det_eval_sizes(name, T, num_classes):
    if not 1 <= int(T) <= DET_EVAL_MAX_T:
        raise ValueError(f'{name}: {T} IoU thresholds, the limit is 1..{DET_EVAL_MAX_T}')
    if not 1 <= int(num_classes) <= DET_EVAL_MAX_CLASSES:
        raise ValueError(f'{name}: num_classes {num_classes} outside 1..{DET_EVAL_MAX_CLASSES}')


def det_thresholds(iou_thresholds, device):
    """The IoU thresholds as the float64 [T] device tensor ``det_match`` reads (a tensor of that kind passes through)."""
    if isinstance(iou_thresholds, torch.Tensor):
        thr = iou_thresholds
    else:
        thr = torch.tensor([float(t) for t in iou_thresholds], dtype=torch.float64)
        if torch.device(device).type == 'cuda':
            thr = thr.pin_memory()                         # (an upload nothing waits for)
    if thr.dim() != 1 or thr.dtype != torch.float64:
        raise ValueError('det_match: iou_thresholds must be a sequence of floats or a float64 [T] tensor')
    return thr.to(device, non_blocking=True).contiguous()


def det_match(det, gt_boxes, gt_class_ids, gt_offsets, iou_thresholds, num_classes, gt_ignore=None, npos=None):
    """Label the packed detect output of a batch against its ground truth (csrc/det_eval.hip; rule: DESIGN.md "Detection AP on the
    device").  ``det``: the tuple of ``detect`` / ``Detector.detect_device`` (count int32 [B], class_ids int64 [B,K], scores [B,K],
    boxes [B,K,4]; further members are not read), K <= 1024.  gt_boxes fp32 [total,4] xyxy, gt_class_ids int32 [total], gt_offsets
    int32 [B+1] (at most 65 535 GT per image), gt_ignore uint8 / bool [total] or None, iou_thresholds: 1..16 floats (or a float64
    device tensor), num_classes 1..256.  -> (flags uint8 [B,K,T]: 0 FP, 1 TP, 2 ignored, 3 empty slot; matched_gt int32 [B,K,T];
    npos int32 [num_classes]).  ``npos``: an int32 [num_classes] device tensor the counts are ADDED to (default: fresh zeros).
    One launch, nothing waits."""
    if len(det) < 4:
        raise ValueError('det_match: det must be (count, class_ids, scores, boxes, ...)')
    cnt, cls, sc, bx = det[:4]
    for t, nm, dt in ((cnt, 'count', torch.int32), (cls, 'class_ids', torch.int64), (sc, 'scores', torch.float32), (bx, 'boxes', torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f'det_match: det {nm} must be a {dt} tensor')
    if sc.dim() != 2 or tuple(cls.shape) != tuple(sc.shape) or tuple(bx.shape) != tuple(sc.shape) + (4,) or tuple(cnt.shape) != (sc.shape[0],):
        raise ValueError(f'det_match: det must be count [B], class_ids [B,K], scores [B,K], boxes [B,K,4], got {tuple(cnt.shape)} '
                         f'{tuple(cls.shape)} {tuple(sc.shape)} {tuple(bx.shape)}')
    B, K = sc.shape
    if B < 1 or not 1 <= K <= DET_EVAL_MAX_K:
        raise ValueError(f'det_match: B = {B}, K = {K}: need B >= 1 and 1 <= K <= {DET_EVAL_MAX_K}')
    for t, nm, dt in ((gt_boxes, 'gt_boxes', torch.float32), (gt_class_ids, 'gt_class_ids', torch.int32), (gt_offsets, 'gt_offsets', torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f'det_match: {nm} must be a {dt} tensor')
    total = gt_class_ids.shape[0] if gt_class_ids.dim() == 1 else -1
    if total < 0 or tuple(gt_boxes.shape) != (total, 4) or tuple(gt_offsets.shape) != (B + 1,):
        raise ValueError(f'det_match: gt_boxes [total,4], gt_class_ids [total], gt_offsets [B+1] = [{B + 1}], got {tuple(gt_boxes.shape)} '
                         f'{tuple(gt_class_ids.shape)} {tuple(gt_offsets.shape)}')
    if gt_ignore is not None:
        if not isinstance(gt_ignore, torch.Tensor) or gt_ignore.dtype not in (torch.uint8, torch.bool) or tuple(gt_ignore.shape) != (total,):
            raise ValueError('det_match: gt_ignore must be a uint8 or bool [total] tensor')
        gt_ignore = gt_ignore.view(torch.uint8) if gt_ignore.dtype == torch.bool else gt_ignore
    if not sc.is_cuda:
        raise ValueError(f'det_match: det must be on the GPU, got {sc.device}')
    dev = sc.device
    thr = det_thresholds(iou_thresholds, dev)
    T = thr.shape[0]
    _check_det_eval_sizes('det_match', T, num_classes)
    num_classes = int(num_classes)
    if npos is None:
        npos = torch.zeros(num_classes, device=dev, dtype=torch.int32)
    elif not isinstance(npos, torch.Tensor) or npos.dtype != torch.int32 or tuple(npos.shape) != (num_classes,) or not npos.is_contiguous():
        raise ValueError('det_match: npos must be a contiguous int32 [num_classes] tensor')
    for t, nm in ((cnt, 'count'), (cls, 'class_ids'), (bx, 'boxes'), (gt_boxes, 'gt_boxes'), (gt_class_ids, 'gt_class_ids'),
                  (gt_offsets, 'gt_offsets'), (gt_ignore, 'gt_ignore'), (npos, 'npos')):
        if t is not None and t.device != dev:
            raise ValueError(f'det_match: {nm} is on {t.device}, the detections on {dev}')
    cnt, cls, sc, bx, gt_boxes, gt_class_ids, gt_offsets = (t.contiguous() for t in (cnt, cls, sc, bx, gt_boxes, gt_class_ids, gt_offsets))
    if bx.data_ptr() % 16:
        bx = bx.clone()
    if gt_boxes.data_ptr() % 16:
        gt_boxes = gt_boxes.clone()
    if gt_ignore is not None:
        gt_ignore = gt_ignore.contiguous()
    flags = torch.empty(B, K, T, device=dev, dtype=torch.uint8)
    matched = torch.empty(B, K, T, device=dev, dtype=torch.int32)
    br = _Bracket('det_match', f'match K{K} T{T}', 0.0, 24.0 * B * K + 21.0 * total + 5.0 * B * K * T) if timing._timer is not None else None
    rc = nat.lib().sqd_det_match_fwd(nat.ptr(cnt), nat.ptr(cls), nat.ptr(sc), nat.ptr(bx), nat.ptr(gt_boxes) if total else None,
                                     nat.ptr(gt_class_ids) if total else None, nat.ptr(gt_offsets),
                                     nat.ptr(gt_ignore) if total else None, nat.ptr(thr), nat.ptr(flags), nat.ptr(matched), nat.ptr(npos),
                                     B, K, int(total), T, num_classes, nat.stream_handle(dev))
    nat.check(rc, 'sqd_det_match_fwd')
    if br is not None:
        br.done()
    return flags, matched, npos


def det_ap(class_ids, flags, seg_offsets, npos, mode, want_prec101=False):
    """Average precision per class and threshold from the accumulated, ORDERED labels (csrc/det_eval.hip): class_ids int32 [N]
    (``num_classes`` = empty slot), flags uint8 [N,T], ordered by (class ascending, score descending, insertion order); seg_offsets
    int32 [num_classes+1]; npos int32 [num_classes]; mode 'area' / 0 (area under the monotone precision envelope), '11point' / 1,
    '101point' / 2.  -> (ap float64 [num_classes,T], NaN where npos == 0; tp_cum, fp_cum int32 [N,T], zero outside the segments;
    prec101 float64 [num_classes,T,101] in mode 2 with ``want_prec101``, else None).  1 <= T <= 16, num_classes <= 256.  One launch."""
    mode = AP_MODES.get(mode, mode)
    if mode not in (0, 1, 2):
        raise ValueError(f"det_ap: mode must be one of {sorted(AP_MODES)} or 0 / 1 / 2, got {mode!r}")
    for t, nm, dt in ((class_ids, 'class_ids', torch.int32), (flags, 'flags', torch.uint8), (seg_offsets, 'seg_offsets', torch.int32),
                      (npos, 'npos', torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError(f'det_ap: {nm} must be a {dt} tensor')
    if class_ids.dim() != 1 or flags.dim() != 2 or flags.shape[0] != class_ids.shape[0] or npos.dim() != 1:
        raise ValueError(f'det_ap: class_ids [N], flags [N,T], npos [num_classes], got {tuple(class_ids.shape)} {tuple(flags.shape)} {tuple(npos.shape)}')
    N, T = flags.shape
    C = npos.shape[0]
    _check_det_eval_sizes('det_ap', T, C)
    if tuple(seg_offsets.shape) != (C + 1,):
        raise ValueError(f'det_ap: seg_offsets must be [num_classes+1] = [{C + 1}], got {tuple(seg_offsets.shape)}')
    if N * T >= 2 ** 31:
        raise ValueError(f'det_ap: N * T = {N * T} exceeds 2^31 - 1')
    if not flags.is_cuda:
        raise ValueError(f'det_ap: flags must be on the GPU, got {flags.device}')
    dev = flags.device
    for t, nm in ((class_ids, 'class_ids'), (seg_offsets, 'seg_offsets'), (npos, 'npos')):
        if t.device != dev:
            raise ValueError(f'det_ap: {nm} is on {t.device}, flags on {dev}')
    class_ids, flags, seg_offsets, npos = class_ids.contiguous(), flags.contiguous(), seg_offsets.contiguous(), npos.contiguous()
    ap = torch.empty(C, T, device=dev, dtype=torch.float64)
    tp_cum = torch.zeros(N, T, device=dev, dtype=torch.int32)
    fp_cum = torch.zeros(N, T, device=dev, dtype=torch.int32)
    prec = torch.empty(C, T, 101, device=dev, dtype=torch.float64) if (want_prec101 and mode == 2) else None
    br = _Bracket('det_ap', f'ap N{N} T{T}', 0.0, 4.0 * N + 21.0 * N * T) if timing._timer is not None else None
    rc = nat.lib().sqd_det_ap_fwd(nat.ptr(class_ids) if N else None, nat.ptr(flags) if N else None, nat.ptr(seg_offsets), nat.ptr(npos),
                                  nat.ptr(ap), nat.ptr(tp_cum) if N else None, nat.ptr(fp_cum) if N else None, nat.ptr(prec),
                                  N, T, C, mode, nat.stream_handle(dev))
    nat.check(rc, 'sqd_det_ap_fwd')
    if br is not None:
        br.done()
    return ap, tp_cum, fp_cum, prec
