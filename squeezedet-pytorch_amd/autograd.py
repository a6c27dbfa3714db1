"""Forward / backward executors behind ``torch.autograd.Function`` so that ``SqueezeDetBase`` and
``Loss`` keep the reference's ``nn.Module`` surface (src/model/squeezedet.py:79-87, :133-174) while
every FLOP runs in the HIP kernels.

The whole backbone is ONE autograd node: its forward walks the layer table launching
stem -> pool -> (squeeze, expand1x1, expand3x3)* -> ConvDet on the current stream, keeping NHWC
activations; its backward walks the table in reverse (dgrad = the same implicit-GEMM kernel with
transposed/flipped weights and the ReLU mask applied while staging dY; wgrad / bias-grad kernels)
and returns the gradients of the 64 canonical OIHW parameters.
"""
from __future__ import annotations


import torch

from . import ops, plan


def _needs_grad(base):
    return torch.is_grad_enabled() and any(p.requires_grad for p in base.parameters())


def _flags(base):
    """The model switches the forward schedule depends on, read once per forward."""
    return plan.Flags(*(getattr(base, f) for f in plan.Flags._fields))


def run_backbone_forward(base, image, save=False, drop_mask=None, drop=None, det_keys=None):
    """Launch the forward schedule (plan.forward_schedule: every launch decision is taken there).  Returns (pred_nhwc
    [B,H,W,A_per_cell*(C+5)], saved dict | None).  Dropout in front of ConvDet (training): ``drop`` (an ops.DropState) applies it
    inside the last Fire's expand launches, or ``drop_mask`` (a scaled keep mask, NHWC) multiplies it in.  ``det_keys`` (an
    ops.DetKeys, inference): ConvDet's launch also stores the detection keys where it can (``det_keys.written``)."""
    if not image.is_cuda:
        raise RuntimeError('SqueezeDetBase runs on the MI355X HIP kernels only: input must be a CUDA/HIP tensor')
    if image.dtype != torch.float32:
        raise RuntimeError('SqueezeDetBase expects fp32 input')
    feats = base.features
    B, dev = image.shape[0], image.device
    steps = plan.forward_schedule(base.arch, B, image.shape[2:], _flags(base), save,
                                  'mask' if drop_mask is not None else 'stream' if drop is not None else None)

    def empty(*shape, dtype=torch.float32):
        return torch.empty(B, *shape, device=dev, dtype=dtype)
    saved = {} if save else None
    cd = base.convdet_exec()                   # (a padded ConvDet's stand-in is brought up to date before the plans are refreshed)
    base.refresh_plans()                       # one batched re-pack if the optimizer touched the parameters
    stem = feats[0]
    bridged = None                             # the next Fire's squeeze output, produced by the previous launch
    if steps[0].form == 'stem_conv':
        a = ops.stem_conv_relu(image, stem.weight, stem.bias)
        if save:
            saved['stem_out'] = a
    else:
        # conv + ReLU + pool fused: the 30.7 MB/image stem output never reaches HBM.  Training keeps the pool
        # argmax; the backward folds ReLU + pool into the stem weight-gradient kernel (ops.stem_wgrad_pooled)
        am = empty(*ops.pool_out_size(steps[1].H, steps[1].W), steps[1].C, dtype=torch.uint8) if save else None
        if steps[0].form == 'stem_pool':
            a = ops.stem_pool(image, stem.weight, stem.bias, argmax=am)
        else:
            # the first Fire's squeeze rides in the stem launch.  Inference: the pooled 64-channel tensor (its only consumer) is
            # never written; training: it and its codes are stored as well (the backward reads them)
            fsq = feats[3].squeeze
            res = ops.stem_pool_squeeze(image, stem.weight, stem.bias, fsq.weight, fsq.bias, argmax=am)
            bridged, a = res if save else (res, None)
        if save:
            saved['stem_pool'] = (am, a)
    if save:
        saved['image'] = image
    for st in steps[1:-1]:
        if type(st) is plan.PoolStep:
            # ('folded': the next squeeze reads the un-pooled map; 'done': the previous launch already pooled and squeezed)
            if st.how == 'launch':
                am = empty(*ops.pool_out_size(st.H, st.W), st.C, dtype=torch.uint8) if save else None
                # training: the codes carry the ReLU mask of the pool's input (a Fire output), the backward reads no mask tensor
                a = ops.maxpool(a, argmax=am, relu_codes=save)
                if save:
                    saved[f'pool{st.i}'] = (am, (st.H, st.W))
            continue
        i, H, W, s, e1, e3 = st.i, st.H, st.W, st.s, st.e1, st.e3
        fire = feats[i]
        if st.mask_launch:                     # this step's mask drawn as a tensor by the stand-alone kernel, multiplied in like a given mask
            drop_mask = ops.dropout_mask(drop, (B, H, W, e1 + e3))
        if st.squeeze == 'done':
            sq, bridged = bridged, None
        else:
            sq = empty(H, W, s)
            if st.squeeze == 'pool_squeeze':
                ops.pool_squeeze(a, 0, st.C, base.plan(f'{i}.squeeze@pool', fire.squeeze, st.sq_cfg), sq, 0)
            else:
                ops.conv(a, 0, base.plan(f'{i}.squeeze', fire.squeeze, st.sq_cfg), sq, 0, relu=True)
        if st.expand == 'fire_pool_bridge':
            # inference: expand pair + concat + the max pool + the squeeze of the Fire behind it in one launch
            bridged = empty(*ops.pool_out_size(H, W), st.nsq)
            ops.fire_pool_bridge(sq, 0, base.fire_bridge_plan(i, fire, feats[i + 2], 12, pooled=True), bridged, 0, nseg=st.cfg)
            a = None
            continue
        if st.expand == 'fire_bridge':
            # inference: this Fire's expand pair AND the next Fire's squeeze in one launch; the concatenated expand
            # output (the next layer's only consumer is that squeeze) is never written
            bridged = empty(H, W, st.nsq)
            ops.fire_bridge(sq, 0, base.fire_bridge_plan(i, fire, feats[i + 1], st.cfg), bridged, 0)
            a = None
            continue
        if st.expand == 'fire_pool_bridge_save':
            # training: expand pair + concat + max pool + the next squeeze in one launch; what the backward reads of this stage -- the
            # pooled tensor (the next squeeze's input) and the pool's arg-max / ReLU codes -- is stored by it, the unpooled expand
            # output is never written
            Hp, Wp = ops.pool_out_size(H, W)
            pooled = empty(Hp, Wp, e1 + e3)
            am = empty(Hp, Wp, e1 + e3, dtype=torch.uint8)
            bridged = empty(Hp, Wp, st.nsq)
            ops.fire_pool_bridge(sq, 0, base.fire_bridge_plan(i, fire, feats[i + 2], 12, pooled=True), bridged, 0, nseg=st.cfg,
                                 save=pooled, codes=am, save_coff1=0, save_coff3=e1)
            saved[f'fire{i}'] = (a, sq, torch.empty(B, H, W, e1 + e3, device='meta'))       # (only the shape of the expand output is read)
            saved[f'pool{i + 1}'] = (am, (H, W))
            a = pooled
            continue
        out = empty(H, W, e1 + e3)
        if st.expand == 'fire_bridge_save':
            # training: the Fire -> Fire bridge in its storing form (the expand output the backward needs is written by the same launch)
            bridged = empty(H, W, st.nsq)
            ops.fire_bridge(sq, 0, base.fire_bridge_plan(i, fire, feats[i + 1], st.cfg), bridged, 0, save=out, save_coff1=0, save_coff3=e1)
        elif st.expand == 'fire_wino':
            # inference: both expands in ONE Winograd launch (expand1x1 = the four inner transform positions, riding
            # along as extra channel slices on the same staged squeeze tile)
            ops.fire_wino(sq, 0, base.fire_wino_plan(i, fire, st.cfg), out, 0, e1)
        elif st.expand == 'fire_expand':
            # inference: both expands in one launch (they read the same squeeze tile; the 1x1 rides along as extra
            # channel groups that only run the centre tap)
            ops.fire_expand(sq, 0, base.fused_expand_plan(i, fire, st.cfg), out, 0)
        elif st.expand == 'conv_drop':
            # dropout in front of ConvDet (reference: squeezedet.py:81-82) inside the two expand launches: the keep decision of an
            # element is a function of (seed, step, its index in `out`), evaluated in the epilogue -- no mask tensor
            ops.conv(sq, 0, base.plan(f'{i}.expand1x1', fire.expand1x1, st.cfg), out, 0, relu=True, drop=drop)
            ops.conv_wino(sq, 0, base.wino_plan(f'{i}.expand3x3', fire.expand3x3, ops.WINO_SK_CFG), out, e1, relu=True, drop=drop)
        else:
            # ... or as a given mask: relu(x) * m == relu(x * m) for the non-negative scaled keep mask, so it is the `ymul`
            # epilogue of the last Fire's two expand kernels -- no extra pass
            ym = drop_mask if st.ymul else None
            ops.conv(sq, 0, base.plan(f'{i}.expand1x1', fire.expand1x1, st.cfg), out, 0, relu=True, ymul=ym, ymul_coff=0)
            base.conv3x3(f'{i}.expand3x3', fire.expand3x3, sq, 0, out, e1, relu=True, ymul=ym)
        if save:
            saved[f'fire{i}'] = (a, sq, out)
        a = out
    pred = empty(steps[-1].H, steps[-1].W, cd.out_channels)
    # (a padded ConvDet's scratch is not `pred`: no keys from it)
    with ops.det_keys_request(det_keys if cd is base.convdet else None):
        base.conv3x3('convdet', cd, a, 0, pred, 0, relu=False)
    if cd is not base.convdet:
        # a width the convolution forms do not take ran zero-padded into a scratch: pack it into the contiguous reference layout
        pred = ops.convdet_pack(pred, base.convdet.out_channels)
    if drop is not None:
        # this forward's mask is consumed: step += 1 on the device.  (The balanced Winograd kernel can carry the advance inside its
        # launch -- ops.conv_wino(..., drop_advance=) -- but measured inside the step it runs ConvDet's forward slower than the unit
        # kernel of the table, 219-230 against 208-216 us, which costs more than this one-thread launch.)
        ops.dropout_advance(drop)
    if save:
        saved['convdet_in'] = a
        saved['drop_mask'] = drop_mask
        # with the fused form the backward needs no mask: convdet_in > 0 exactly where the element was kept AND its ReLU was active
        saved['drop_scale'] = float(drop.scale) if steps[-1].fused_rng else None
    return pred, saved


def _make_drop_mask(base, device):
    """An injected mask (tests: NCHW, already scaled by 1 / (1 - p)) in the layout the epilogues read."""
    return base._forced_drop_mask.to(device).permute(0, 2, 3, 1).contiguous()


def backbone_apply(base, image, det_keys=None):
    if torch.is_grad_enabled() and isinstance(image, torch.Tensor) and image.requires_grad:
        # (torch would hand back image.grad; the backward stops at the stem's weight gradient, so it would stay None without a word)
        raise RuntimeError('SqueezeDetBase: the input image requires grad, but the HIP backward computes no gradient with respect to '
                           'the image (it ends at the stem\'s weight gradient).  Pass image.detach(), or run under torch.no_grad().')
    train_drop = base.training and base.dropout is not None
    drop_mask = drop = None
    if train_drop:
        if base._forced_drop_mask is not None:
            drop_mask = _make_drop_mask(base, image.device)
        else:
            drop = base.drop_state(image.device)
    if _needs_grad(base):
        from .backward import BackboneFn
        params = [p for _, p in base.named_parameters()]
        pred = BackboneFn.apply(base, image, drop_mask, drop, *params)
    else:
        pred, _ = run_backbone_forward(base, image, save=False, drop_mask=drop_mask, drop=drop,
                                       det_keys=None if train_drop else det_keys)
    B = pred.shape[0]
    out = pred.view(B, -1, base.num_classes + 5)
    if out.shape[1] != base.num_anchors:
        raise RuntimeError(f'input size yields {out.shape[1]} anchors but cfg.num_anchors is {base.num_anchors}')
    return out


def loss_apply(loss_mod, pred, gt, ignore=None):
    from .backward import LossFn, LossMaskedFn, LossSparseFn
    anchors = loss_mod.resolver.anchors_on(pred.device)
    if ignore is not None:
        if not isinstance(gt, ops.SparseGT):
            raise ValueError('Loss: an ignore bitmap needs a sparse ground truth (ops.SparseGT, cfg.sparse_gt); the dense loss has no masked form')
        vec = LossMaskedFn.apply(pred, anchors, loss_mod, ignore, *gt)
    elif isinstance(gt, ops.SparseGT):
        vec = LossSparseFn.apply(pred, anchors, loss_mod, *gt)
    else:
        vec = LossFn.apply(pred, gt, anchors, loss_mod)
    # vec: [4, B] = (class, pos+neg score, bbox, total) -- reference returns (loss, stats dict), :166-174
    class_loss, score_loss, bbox_loss, loss = vec[0], vec[1], vec[2], vec[3]
    return loss, {'loss': loss, 'class_loss': class_loss, 'score_loss': score_loss, 'bbox_loss': bbox_loss}
