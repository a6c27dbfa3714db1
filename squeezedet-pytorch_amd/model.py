"""``nn.Module`` surface of the reference's ``src/model/squeezedet.py`` -- same class names,
constructor arguments, ``forward`` signatures, sub-module attribute names and ``state_dict`` keys /
shapes (OIHW fp32) -- with every forward/backward running on the hand-written gfx950 kernels.

Reference map:
  Fire                 src/model/squeezedet.py:9-23
  SqueezeDetBase       :26-97   (features Sequential, dropout, convdet, init_weights)
  PredictionResolver   :100-120
  Loss                 :123-174
  SqueezeDetWithLoss   :177-187
  SqueezeDet           :190-206

Internally activations are NHWC fp32; the two expand convolutions of a Fire write disjoint channel
ranges of one buffer (no ``torch.cat``), ConvDet's NHWC output *is* the permuted tensor of :85.
Canonical parameters stay OIHW ``nn.Parameter``s (optimizer / clip_grad_norm_ / state_dict touch
them directly); the packed copies the kernels read are a private cache keyed on ``param._version``.
There is no CPU path: modules raise if the input is not on a GPU or the HIP library is missing.
"""
from __future__ import annotations


import numpy as np
import torch
import torch.nn as nn

from . import ops
from .config import check_bbox_loss
from .plan import conv3x3_cfg
from .plans import PlanCache, version
from .synthetic import layer_table, convdet_in_channels


def _nhwc_input(x, channels, who):
    """Stand-alone sub-module calls take the reference's NCHW tensors: checked, detached, viewed NHWC (no copy when the
    tensor came out of another sub-module, whose NCHW result is a permuted view of an NHWC buffer)."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == channels):
        raise RuntimeError(f'{who}: expected an fp32 CUDA/HIP tensor [B,{channels},H,W] (the layers run on the MI355X kernels only)')
    return x.detach().permute(0, 2, 3, 1).contiguous()


class _ConvParams(nn.Module):
    """Parameter holder with nn.Conv2d's state_dict layout (``weight`` OIHW, ``bias``).  Inside ``SqueezeDetBase.forward``
    the layer runs as part of the fused HIP plan; called on its own (``model.base.features[0](x)``, ``fire.squeeze(s)``,
    as the reference's ``nn.Conv2d`` allows) it launches its kernel stand-alone: NCHW in, NCHW out, no activation,
    inference only (not differentiable -- training differentiates through the parent module)."""

    def __init__(self, cin, cout, ksize, stride=1, padding=0):
        super().__init__()
        self.in_channels, self.out_channels = cin, cout
        self.kernel_size, self.stride, self.padding = (ksize, ksize), (stride, stride), (padding, padding)
        self.weight = nn.Parameter(torch.empty(cout, cin, ksize, ksize))
        self.bias = nn.Parameter(torch.empty(cout))
        self._own_plan = None
        self._own_pad = None               # run_nhwc's zero-padded stand-in (a 3x3 layer of a width that is no multiple of 4)

    def extra_repr(self):
        return f'{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}, padding={self.padding}'

    def _plan(self, npix):
        k = self.kernel_size[0]
        wc = ops.choose_wino_cfg(self.in_channels, self.out_channels, npix) if k == 3 else None
        cfg_id = ('w', wc) if wc is not None else ('d', ops.choose_cfg(k * k, self.in_channels, self.out_channels, npix))
        ver = (cfg_id,) + version((self,))
        if self._own_plan is None or self._own_plan[0] != ver:
            plan = ops.WinoPlan(self.weight, self.bias, wc) if wc is not None else ops.ConvPlan(self.weight, self.bias, cfg_id[1])
            self._own_plan = (ver, plan)
        return self._own_plan[1]

    def run_nhwc(self, x, relu=False, out=None, out_coff=0):
        """NHWC in -> NHWC out (channel window ``out_coff`` of ``out`` when given)."""
        Bq, H, W, _ = x.shape
        if self.kernel_size[0] == 3 and ops.convdet_pad_width(self.out_channels) != self.out_channels and out is None:
            # a ConvDet of a width the convolution forms do not take, called on its own: zero-padded stand-in, then the pack launch
            if self._own_pad is None or self._own_pad.weight.device != self.weight.device:
                self._own_pad = _PaddedConvDet(self, ops.convdet_pad_width(self.out_channels))
            return ops.convdet_pack(self._own_pad.sync().run_nhwc(x, relu=relu), self.out_channels)
        y = out if out is not None else torch.empty(Bq, H, W, self.out_channels, device=x.device, dtype=torch.float32)
        plan = self._plan(Bq * H * W)
        if isinstance(plan, ops.WinoPlan):
            return ops.conv_wino(x, 0, plan, y, out_coff, relu=relu)
        return ops.conv(x, 0, plan, y, out_coff, relu=relu)

    def forward(self, x):
        if self.stride[0] == 2:                           # the stem: reads the NCHW image directly
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32):
                raise RuntimeError('stem conv: expected an fp32 CUDA/HIP NCHW image')
            return ops.stem_conv_relu(x.detach(), self.weight, self.bias, relu=False).permute(0, 3, 1, 2)
        return self.run_nhwc(_nhwc_input(x, self.in_channels, 'conv')).permute(0, 3, 1, 2)


class _PaddedConvDet:
    """ConvDet as the executors launch it when its width N = anchors_per_grid * (num_classes + 5) is one the convolution forms do not
    take (``ops.convdet_width``): zero-padded copies [Npad, Cin, 3, 3] / [Npad] of the canonical parameters, which keep the
    reference's shapes.  ``sync`` copies the parameters into the first N rows when they changed (a contiguous prefix: two
    device-to-device copies); the rows past N stay zero, so the padded output channels are zero and the padded gradient rows are never
    read.  Not a module: nothing of it reaches ``state_dict`` / ``parameters``."""

    def __init__(self, mod, Npad):
        self.src, self.true_channels = mod, mod.out_channels
        self.in_channels, self.out_channels = mod.in_channels, int(Npad)
        self.kernel_size, self.stride, self.padding = mod.kernel_size, mod.stride, mod.padding
        dev = mod.weight.device
        self.weight = torch.zeros(self.out_channels, mod.in_channels, 3, 3, device=dev, dtype=torch.float32)
        self.bias = torch.zeros(self.out_channels, device=dev, dtype=torch.float32)
        self._ver = None
        self._own_plan = None                 # (_ConvParams.run_nhwc / _plan run on this object for a stand-alone call)

    _plan, run_nhwc = _ConvParams._plan, _ConvParams.run_nhwc      # (a stand-alone call launches it like any 3x3 layer)

    def sync(self):
        m, N = self.src, self.true_channels
        ver = version((m,))
        if ver != self._ver:
            self.weight[:N].copy_(m.weight.detach())
            self.bias[:N].copy_(m.bias.detach())
            self._ver = ver
        return self


class _Marker(nn.Module):
    """Keeps the reference's nn.Sequential indices for the ReLU / MaxPool2d slots (fused away inside
    ``SqueezeDetBase.forward``).  Called on its own it applies that layer: the pool through the HIP kernel, the ReLU as a
    plain elementwise op."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what

    def forward(self, x):
        if self.what.startswith('ReLU'):
            return torch.relu(x.detach())
        return ops.maxpool(_nhwc_input(x, x.shape[1], 'max pool')).permute(0, 3, 1, 2)


class Fire(nn.Module):
    def __init__(self, inplanes, squeeze_planes, expand1x1_planes, expand3x3_planes):
        super().__init__()
        self.squeeze = _ConvParams(inplanes, squeeze_planes, 1)
        self.expand1x1 = _ConvParams(squeeze_planes, expand1x1_planes, 1)
        self.expand3x3 = _ConvParams(squeeze_planes, expand3x3_planes, 3, padding=1)

    def forward(self, x):
        """Stand-alone Fire (src/model/squeezedet.py:17-23): NCHW in, NCHW out; three kernel launches, the two expands
        write the two halves of one buffer (no ``torch.cat``).  Inference only."""
        xh = _nhwc_input(x, self.squeeze.in_channels, 'Fire')
        s = self.squeeze.run_nhwc(xh, relu=True)
        e1, e3 = self.expand1x1.out_channels, self.expand3x3.out_channels
        out = torch.empty(*s.shape[:3], e1 + e3, device=s.device, dtype=torch.float32)
        self.expand1x1.run_nhwc(s, relu=True, out=out, out_coff=0)
        self.expand3x3.run_nhwc(s, relu=True, out=out, out_coff=e1)
        return out.permute(0, 3, 1, 2)


class SqueezeDetBase(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_classes = cfg.num_classes
        self.num_anchors = cfg.num_anchors
        self.arch = cfg.arch
        mods = []
        for l in layer_table(cfg.arch):                   # raises ValueError('Invalid architecture.')
            if l[0] == 'conv':
                mods.append(_ConvParams(l[1], l[2], l[3], stride=l[4], padding=l[5]))
            elif l[0] == 'relu':
                mods.append(_Marker('ReLU (fused into the stem kernel)'))
            elif l[0] == 'pool':
                mods.append(_Marker('MaxPool2d(kernel_size=3, stride=2, ceil_mode=True)'))
            else:
                mods.append(Fire(*l[1:]))
        self.features = nn.Sequential(*mods)
        self.dropout_prob = float(cfg.dropout_prob)
        self.dropout = nn.Dropout(cfg.dropout_prob, inplace=True) if cfg.dropout_prob > 0 else None
        self.convdet = _ConvParams(convdet_in_channels(cfg.arch), cfg.anchors_per_grid * (cfg.num_classes + 5), 3, padding=1)
        self._convdet_pad = None                  # _PaddedConvDet when the width is padded (convdet_exec)
        self._convdet_slab = None                 # its weight-gradient slab workspace
        self.plan_cache = PlanCache()             # every packed / transformed weight copy the executors launch with
        self._wgrad_batches = {}
        self.last_grad_flat = None                # flat gradient buffer of the latest backward (every .grad is a view of it)
        self.grad_sync = None                     # trainer.GradientExchange when data parallel (attach_data_parallel)
        self.use_winograd = True                  # 3x3 forward convs: Winograd F(2x2,3x3) kernel where tuning.json says it is faster
        self.fuse_expand = True                   # inference forward: expand1x1 + expand3x3 in one launch
        self.fuse_expand_wino = True              # ... in Winograd form (ops.fire_wino) where the table has an X: row
        self.fuse_fire_bridge = True              # ... together with the NEXT Fire's squeeze (ops.fire_bridge) where it has a Y: row
        self.fuse_train_forward = True    # training forward: the bridges in their storing forms
        # inference forward: pool 2 / 3 folded into the following squeeze (ops.pool_squeeze).  Off by default: measured equal
        # to the two separate kernels (0.174 vs 0.18 ms) -- both are bound by the 9x L2 read amplification of the window gather
        self.fuse_pool_squeeze = False
        self.fuse_stem_squeeze = True             # inference forward: the first Fire's squeeze inside the stem launch (ops.stem_pool_squeeze)
        # detection (Detector.detect_device / lanes.DetectStream): ConvDet's epilogue stores the score keys, the fused detect skips its
        # scoring pass (three classes, ConvDet on the V-shared Winograd kernel, narrow detect; same launches, same bits)
        self.fuse_detect_keys = True
        self._forced_drop_mask = None       # tests: NCHW mask (already scaled by 1/(1-p)) instead of RNG
        # counter-based dropout (ops.DropState): applied in the last Fire's expand epilogues, its step advanced by ConvDet's launch,
        # no mask tensor and no torch RNG kernel in the step.  fused_dropout = False draws the mask as a tensor (stand-alone kernel)
        self.fused_dropout = True
        self._drop = None                   # (torch.initial_seed() it was derived from, ops.DropState)
        self._drop_restored = False         # the stream came from set_dropout_rng (a checkpoint), not from torch's seed
        self.fuse_squeeze_bwd = True     # backward: squeeze wgrad + dgrad in one launch
        self.group_wgrad = ops.WINO_WGRAD_GROUP   # backward: the expand3x3 weight gradients of a stage share one launch (ops.conv_wgrad_wino_group)
        self.init_weights()

    # ---- reference: init_weights, src/model/squeezedet.py:89-97 ----
    def init_weights(self):
        for m in self.modules():
            if isinstance(m, _ConvParams):
                nn.init.normal_(m.weight, mean=0.0, std=0.002 if m is self.convdet else 0.005)
                nn.init.constant_(m.bias, 0)

    def convdet_exec(self):
        """The ConvDet the executors launch: the module itself where the convolution forms take its width (every width that ran
        before: exactly the launches of before), else its zero-padded stand-in, brought up to date with the parameters."""
        cd = self.convdet
        N, Npad = cd.out_channels, ops.convdet_pad_width(cd.out_channels)
        if Npad == N:
            return cd
        pad = self._convdet_pad
        if pad is None or pad.weight.device != cd.weight.device or pad.out_channels != Npad:
            pad = self._convdet_pad = _PaddedConvDet(cd, Npad)
            self._convdet_slab = None
        return pad.sync()

    def convdet_slab(self, numel):
        """Slab workspace of the padded ConvDet's weight gradient (allocated once per size: pointer-stable)."""
        ws = self._convdet_slab
        if ws is None or ws.numel() != numel or ws.device != self.convdet.weight.device:
            ws = self._convdet_slab = torch.empty(numel, device=self.convdet.weight.device, dtype=torch.float32)
        return ws

    # ---- packed-weight cache (plans.PlanCache: the entry keeps the modules, staleness and refresh are decided there) ----
    def plan(self, name, mod, cfg_id, direction='fwd'):
        return self.plan_cache.get('conv', (name, cfg_id), (mod,),
                                   lambda: ops.ConvPlan(mod.weight, mod.bias, cfg_id, dgrad=(direction != 'fwd')), direction)

    def wino_plan(self, name, mod, cfg_id, direction='fwd'):
        """Transformed-weight cache of the Winograd 3x3 kernel (ops.WinoPlan), re-transformed in place when the parameter
        changed."""
        return self.plan_cache.get('wino', (name, cfg_id), (mod,),
                                   lambda: ops.WinoPlan(mod.weight, mod.bias, cfg_id, dgrad=(direction != 'fwd')), direction)

    def fused_expand_plan(self, idx, fire, cfg_id):
        """Packed weights of ``fire``'s expand pair for the one-launch fused expand (inference forward).  Rebuilt when
        either module's parameters change; not part of ``refresh_plans`` (training keeps the two separate kernels, whose
        per-layer activations and packed weights the backward needs anyway)."""
        e1, e3 = fire.expand1x1, fire.expand3x3
        return self.plan_cache.get('fused_expand', (idx, cfg_id), (e1, e3),
                                   lambda: ops.FusedExpandPlan(e1.weight, e1.bias, e3.weight, e3.bias, cfg_id))

    def fire_wino_plan(self, idx, fire, cfg_id):
        """Packed weights of ``fire``'s expand pair for the one-launch Winograd form (inference forward); rebuilt when either
        module's parameters change."""
        e1, e3 = fire.expand1x1, fire.expand3x3
        return self.plan_cache.get('fire_wino', (idx, cfg_id), (e1, e3),
                                   lambda: ops.FireWinoPlan(e1.weight, e1.bias, e3.weight, e3.bias, cfg_id))

    def fire_bridge_plan(self, idx, fire, nxt, cfg_id, pooled=False):
        """Operands of the one-launch form of ``fire``'s expand pair + ``nxt``'s squeeze (ops.fire_bridge / ops.fire_pool_bridge);
        refreshed in place when any of the three modules' parameters change (``refresh_plans`` does all bridges with two launches)."""
        e1, e3, sq = fire.expand1x1, fire.expand3x3, nxt.squeeze
        return self.plan_cache.get('bridge', (idx, cfg_id, pooled), (e1, e3, sq),
                                   lambda: ops.FireBridgePlan(e1.weight, e1.bias, e3.weight, e3.bias, sq.weight, sq.bias, cfg_id, pooled=pooled))

    # Read-only views of ``plan_cache`` in the shapes of the three dictionaries it replaced, for harnesses and tools written against
    # those.  Derived on every read: they hold no state, and nothing in the package reads them.
    @property
    def _plans(self):                              # (name, cfg, direction) -> (version, plan)
        return {e.key + (e.direction,): (e.version, e.plan) for e in self.plan_cache.entries() if e.kind == 'conv'}

    @property
    def _wino_plans(self):                         # the same, of the Winograd plans
        return {e.key + (e.direction,): (e.version, e.plan) for e in self.plan_cache.entries() if e.kind == 'wino'}

    @property
    def _fused_plans(self):     # ('fused' | 'firewino', idx, cfg) -> (version, plan);  ('firebridge', idx, cfg, pooled) -> (version, plan, mods)
        tag = {'fused_expand': 'fused', 'fire_wino': 'firewino', 'bridge': 'firebridge'}
        return {(tag[e.kind],) + e.key: (e.version, e.plan) + ((e.mods,) if e.kind == 'bridge' else ())
                for e in self.plan_cache.entries() if e.kind in tag}

    def conv3x3(self, name, mod, x, x_coff, y, y_coff, relu, ymul=None):
        """Forward 3x3 convolution of ``mod``: the Winograd kernel where the measured table prefers it, else the direct
        implicit-GEMM kernel."""
        Bq, H, W, _ = x.shape
        C, N = mod.in_channels, mod.out_channels
        # (the Winograd kernel reads ymul with y's geometry)
        wino, cfg = conv3x3_cfg(C, N, Bq * H * W, self.use_winograd and (ymul is None or tuple(ymul.shape) == tuple(y.shape)))
        if wino:
            return ops.conv_wino(x, x_coff, self.wino_plan(name, mod, cfg), y, y_coff, relu=relu, ymul=ymul)
        return ops.conv(x, x_coff, self.plan(name, mod, cfg), y, y_coff, relu=relu, ymul=ymul, ymul_coff=y_coff)

    def dgrad3x3(self, name, mod, dy, dy_coff, dx, accumulate=False, ymask=None, ymul=None):
        """dx (=|+=) data gradient of ``mod``'s 3x3 convolution (transposed, tap-flipped weights), ymul / ymask fused into the
        epilogue; Winograd kernel where the measured table prefers it."""
        Bq, H, W, _ = dy.shape
        C, N = mod.out_channels, mod.in_channels                  # the dgrad convolves dY (out channels) into dX (in channels)
        same_geom = all(t is None or tuple(t.shape) == tuple(dx.shape) for t in (ymask, ymul))
        wino, cfg = conv3x3_cfg(C, N, Bq * H * W, self.use_winograd and same_geom)
        if wino:
            return ops.conv_wino(dy, dy_coff, self.wino_plan(name, mod, cfg, 'dgrad'), dx, 0, accumulate=accumulate, ymask=ymask, ymul=ymul)
        return ops.conv(dy, dy_coff, self.plan(name, mod, cfg, 'dgrad'), dx, 0, accumulate=accumulate, ymask=ymask, ymul=ymul)

    # ---- dropout state ----
    def drop_state(self, device):
        """The device-side {seed, step} of this module's dropout (created on first use from ``torch.initial_seed()``; re-derived,
        step 0, when the process was re-seeded with ANOTHER seed since -- ``torch.manual_seed`` keeps working as the one seed of a run,
        and the per-rank seed offsets of ``trainer.attach_data_parallel`` give every rank its own masks; re-seeding with the same
        value is not observable here and continues the stream: ``set_dropout_rng(seed, 0, device)`` restarts it explicitly)."""
        seed = torch.initial_seed()
        stale = self._drop is not None and (self._drop[1].state.device != torch.device(device) or self._drop[1].p != self.dropout_prob)
        # a RESTORED stream (set_dropout_rng: checkpoint resume) is not tied to torch's seed any more: the per-rank re-seeding of a later
        # attach_data_parallel, or a torch.manual_seed of the training script, must not silently restart it at step 0
        reseeded = self._drop is not None and not self._drop_restored and self._drop[0] != seed
        if self._drop is None or stale or reseeded:
            self._drop = (seed, ops.DropState(self.dropout_prob, seed ^ 0x5851f42d4c957f2d, device))
            self._drop_restored = False
        return self._drop[1]

    def get_dropout_rng(self):
        """(seed, step) of the dropout stream or None (checkpoints)."""
        return None if self._drop is None else self._drop[1].get()

    def set_dropout_rng(self, seed, step, device):
        """Restore a saved dropout stream (checkpoint resume); it stays in force -- also across a later ``torch.manual_seed`` / the
        per-rank seed offsets of ``attach_data_parallel`` -- until ``set_dropout_rng`` is called again."""
        d = ops.DropState(self.dropout_prob, 0, device)
        d.set(seed, step)
        self._drop = (torch.initial_seed(), d)
        self._drop_restored = True          # (drop_state() keeps it whatever happens to torch's seed; set_dropout_rng again replaces it)

    def invalidate_plans(self):
        """Drop every packed / transformed weight copy.  The caches notice optimizer steps, ``load_state_dict``, ``.to()``
        and any other in-place op on the parameters (version counter / data pointer); a write through ``param.data``
        (a hand-made EMA, manual ``p.data.copy_``) moves neither -- call this after one.  The EMA the fused optimizers keep
        (``trainer.FusedClipSGD`` / ``FusedClipAdamW`` with ``ema_decay > 0``) needs no such call: ``optimizer.averaged_weights()``
        advances the version counters when it swaps the averaged values in and out."""
        self.plan_cache.clear()
        for m in self.modules():
            if isinstance(m, _ConvParams):
                m._own_plan = m._own_pad = None

    def refresh_plans(self):
        """Re-pack every cached plan whose parameter changed since it was packed (after an optimizer step that
        is all of them) with ONE batched kernel launch per kind instead of one launch per plan."""
        self.convdet_exec()                        # (a padded ConvDet's stand-in is brought up to date before versions are compared)
        self.plan_cache.refresh()

    def wgrad_batch(self, entries_fn, key):
        """Cached ops.WgradBatch for one set of layer shapes (``entries_fn()`` builds the entry list on a miss)."""
        hit = self._wgrad_batches.get(key)
        if hit is None:
            if len(self._wgrad_batches) > 4:
                self._wgrad_batches.clear()
            entries, slots, total = entries_fn()
            hit = (ops.WgradBatch(entries, self.convdet.weight.device), slots, total)
            self._wgrad_batches[key] = hit
        return hit

    def forward(self, x):
        from .autograd import backbone_apply
        return backbone_apply(self, x)


class PredictionResolver(nn.Module):
    def __init__(self, cfg, log_softmax=False):
        super().__init__()
        self.log_softmax = log_softmax
        self.input_size = cfg.input_size
        self.num_classes = cfg.num_classes
        self.anchors = torch.from_numpy(np.asarray(cfg.anchors)).unsqueeze(0).float()
        self.anchors_per_grid = cfg.anchors_per_grid
        self._dev_anchors = {}

    def anchors_on(self, device):
        a = self._dev_anchors.get(device)
        if a is None:
            a = self.anchors[0].to(device).contiguous()
            self._dev_anchors[device] = a
        return a

    def forward(self, pred):
        """Same five outputs as the reference (src/model/squeezedet.py:109-120): (pred_class_probs [B,A,C],
        pred_log_class_probs | None, pred_scores [B,A,1], pred_deltas [B,A,4], pred_boxes [B,A,4]) -- inference only
        (not differentiable; the training path differentiates through ``Loss``, whose kernel has the analytic backward)."""
        resolve = ops.resolve if ops.head_path(self.num_classes) == 'narrow' else ops.resolve_many
        return resolve(pred.detach(), self.anchors_on(pred.device), self.input_size, self.num_classes, self.log_softmax)

    def decode(self, pred):
        """Fused resolver + ``probs *= score; argmax; max`` of ``SqueezeDet.forward`` (:199-202):
        (class_ids int64 [B,A], scores [B,A], boxes [B,A,4])."""
        decode = ops.decode if ops.head_path(self.num_classes) == 'narrow' else ops.decode_many
        return decode(pred, self.anchors_on(pred.device), self.input_size, self.num_classes)


class SqueezeDet(nn.Module):
    """ Model for inference """

    def __init__(self, cfg):
        super().__init__()
        self.base = SqueezeDetBase(cfg)
        self.resolver = PredictionResolver(cfg, log_softmax=False)

    def forward(self, batch):
        pred = self.base(batch['image'])
        class_ids, scores, boxes = self.resolver.decode(pred)
        return {'class_ids': class_ids, 'scores': scores, 'boxes': boxes}


class Loss(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.resolver = PredictionResolver(cfg, log_softmax=True)
        self.num_anchors = cfg.num_anchors
        self.class_loss_weight = cfg.class_loss_weight
        self.positive_score_loss_weight = cfg.positive_score_loss_weight
        self.negative_score_loss_weight = cfg.negative_score_loss_weight
        self.bbox_loss_weight = cfg.bbox_loss_weight
        # 'l2' (the reference's squared error on the deltas) | 'iou' | 'giou' | 'diou' | 'ciou': the regression term of the loss launches
        self.bbox_loss = check_bbox_loss(getattr(cfg, 'bbox_loss', 'l2'), 'Loss')

    def forward(self, pred, gt, ignore=None):
        """``gt``: the dense tensor [B,A,C+9] or an ``ops.SparseGT`` (the positives as a list: the sparse loss launches).  ``ignore``:
        an anchor ignore bitmap int32 [B, ceil(A/32)] (``ops.anchor_ignore_mask``; sparse ``gt`` only): the masked launches, which
        leave ignored anchors out of the loss and give finite values on an object-free image."""
        from .autograd import loss_apply
        return loss_apply(self, pred, gt, ignore)

    def mean_loss(self, pred, gt, ignore=None):
        """``forward(pred, gt, ignore)[0].mean()`` and the (detached) statistics as one autograd node whose forward and backward are the
        loss kernels alone (backward.LossMeanFn; LossSparseMeanFn for an ``ops.SparseGT``; LossMaskedMeanFn with ``ignore``): -> (mean
        total loss, 0-dim; stats dict of per-image vectors)."""
        from .backward import LossMeanFn, LossMaskedMeanFn, LossSparseMeanFn
        if ignore is not None:
            if not isinstance(gt, ops.SparseGT):
                raise ValueError('Loss: an ignore bitmap needs a sparse ground truth (ops.SparseGT, cfg.sparse_gt); the dense loss has no masked form')
            mean, vec = LossMaskedMeanFn.apply(pred, self.resolver.anchors_on(pred.device), self, ignore, *gt)
        elif isinstance(gt, ops.SparseGT):
            mean, vec = LossSparseMeanFn.apply(pred, self.resolver.anchors_on(pred.device), self, *gt)
        else:
            mean, vec = LossMeanFn.apply(pred, gt, self.resolver.anchors_on(pred.device), self)
        return mean, {'loss': vec[3], 'class_loss': vec[0], 'score_loss': vec[1], 'bbox_loss': vec[2]}


class SqueezeDetWithLoss(nn.Module):
    """ Model for training """

    def __init__(self, cfg):
        super().__init__()
        self.base = SqueezeDetBase(cfg)
        self.loss = Loss(cfg)

    def forward(self, batch):
        pred = self.base(batch['image'])
        loss, loss_stats = self.loss(pred, batch['gt'] if 'gt' in batch else batch['gt_sparse'], batch.get('gt_ignore'))
        return loss, loss_stats

    def forward_mean(self, batch):
        """``forward(batch)[0].mean()`` (the scalar the reference's trainer differentiates, src/engine/trainer.py:43) + the per-image
        statistics, with the mean and its backward inside the loss kernels (no torch kernel between loss and backbone).
        ``batch['gt_ignore']`` (optional, with ``'gt_sparse'``): the anchor ignore bitmap."""
        pred = self.base(batch['image'])
        return self.loss.mean_loss(pred, batch['gt'] if 'gt' in batch else batch['gt_sparse'], batch.get('gt_ignore'))
