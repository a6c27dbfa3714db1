"""Backward executors: ``BackboneFn`` (one autograd node for stem..ConvDet) and ``LossFn``.

Reference behaviour reproduced: autograd through ``SqueezeDetBase.forward`` (src/model/squeezedet.py:79-87)
and ``Loss.forward`` (:133-174) as triggered by ``loss.backward()`` in src/engine/trainer.py:47.

Gradient flow convention: every gradient tensor materialised in HBM already carries the ReLU mask of
the activation it belongs to -- the kernel that *produces* it applies the mask in its epilogue
(``ymask``), so the (up to four) consumers of that gradient read it once each without the mask tensor.
"""
from __future__ import annotations

import torch

from . import ops, plan
from .autograd import run_backbone_forward
from .synthetic import layer_table


def _wgrad_layout(base, wgrad, skip=()):
    """Flat gradient layout (named_parameters order: every gradient is a view of ONE buffer) and the batched-reduction
    entries of all Fire / ConvDet weight gradients (``wgrad``: plan.backward_schedule, in backward order; ``skip``: prefixes
    reduced on their own -- a padded ConvDet, whose slabs are wider than its gradient)."""
    slots, off = {}, 0
    for n, p in base.named_parameters():
        slots[n] = (off, tuple(p.shape)); off += p.numel()
    entries = [(pre, w.N, w.C, w.taps, *w.shape, slots[pre + '.weight'][0], slots[pre + '.bias'][0], w.fused, w.group)
               for pre, w in wgrad.items() if pre not in skip]
    return entries, slots, off


def run_backbone_backward(base, saved, dpred):
    """dpred: NHWC [B,H,W,anchors_per_grid*(C+5)].  Returns {param_name (relative to base): grad}; every gradient is a
    view of one flat fp32 buffer in ``named_parameters`` order (``base.last_grad_flat``)."""
    layers = layer_table(base.arch)
    feats = base.features
    dpred = dpred.contiguous()
    B, H, W, ncd = dpred.shape
    cd = base.convdet_exec()
    padded = cd is not base.convdet
    if padded:
        # ConvDet ran zero-padded (ops.convdet_width): its gradient launches read dpred spread to that width, zero past ncd
        n_true, ncd = ncd, cd.out_channels
        dpred = ops.convdet_unpack(dpred, ncd)
    a_in = saved['convdet_in']
    cin_cd = a_in.shape[3]
    shapes = tuple(tuple(saved[f'fire{i}'][2].shape) for i in range(len(layers)) if layers[i][0] == 'fire')
    wgrad, convdet_sk = plan.backward_schedule(base.arch, [s[:3] for s in shapes], ncd, base.fuse_squeeze_bwd, base.group_wgrad,
                                               saved['drop_scale'] is not None)
    shape_key = (B, H, W, bool(base.fuse_squeeze_bwd), base.group_wgrad) + shapes
    wb, slots, total = base.wgrad_batch(lambda: _wgrad_layout(base, wgrad, ('convdet',) if padded else ()), shape_key)
    # + 1: the data-parallel exchange carries this rank's image count through the same all-reduce (trainer.GradientExchange)
    grad_buf = torch.empty(total + 1, device=dpred.device, dtype=torch.float32)
    grad_flat = grad_buf[:total]
    sync = getattr(base, 'grad_sync', None)
    if sync is not None:
        sync.begin(grad_buf, total, B)
    # Stages of the backward = runs of layers between two pools.  With a gradient exchange attached, each stage's slabs
    # are reduced as soon as the stage is done and its slice of the flat buffer (named_parameters order: a stage is a
    # contiguous range, later stages of the network sit at higher offsets) is handed to the all-reduce; without one, all
    # slabs are reduced by a single launch at the end.
    stage = {'row': 0, 'hi': total}
    pending = {}                                           # group id -> the members seen so far (ops.conv_wgrad_wino_group)

    def close_stage(first_param):
        """Everything from ``first_param`` to the previous stage's start is final once the pending slabs are reduced."""
        if sync is None:
            return
        row_hi = wb.row_of[first_param.rsplit('.', 1)[0]] + 1 if first_param is not None else wb.nrows
        if row_hi > stage['row']:
            wb.reduce(grad_flat, stage['row'], row_hi, scale=sync.scale)     # (weighted by this rank's image count on the way out)
            stage['row'] = row_hi
        lo = slots[first_param][0] if first_param is not None else 0
        sync.ready(lo, stage['hi'])
        stage['hi'] = lo

    def gview(name):
        off, shape = slots[name]
        n = 1
        for d in shape:
            n *= d
        return grad_flat[off:off + n].view(shape)
    if padded:
        # slabs of the padded width in a workspace of their own, reduced over the first n_true rows straight into the parameter-shaped
        # views of the flat buffer (times the data-parallel weight, as wb.reduce would)
        S_cd, stride_cd = ops.wgrad_split(ncd, cin_cd, 9, B, H, W)
        slab_cd = base.convdet_slab(S_cd * stride_cd)
        ops.conv_wgrad(dpred, 0, ncd, a_in, 0, cin_cd, 9, slab=slab_cd)
        ops.wgrad_reduce_rows(slab_cd, S_cd, n_true, ncd, cin_cd, 9, gview('convdet.weight'), gview('convdet.bias'),
                              scale=1.0 if sync is None else sync.scale)
    else:
        ops.conv_wgrad(dpred, 0, ncd, a_in, 0, cin_cd, 9, slab=wb.slab('convdet'))
    last = len(layers) - 1
    assert layers[last][0] == 'fire'
    out_last = saved[f'fire{last}'][2]
    dA = torch.empty_like(out_last)
    if saved['drop_scale'] is not None:
        # fused dropout: out_last IS the dropped ReLU output (> 0 exactly where kept and active), so the gradient is masked by it and
        # scaled by the constant 1 / (1 - p): no mask tensor is read
        if convdet_sk:
            ops.conv_wino(dpred, 0, base.wino_plan('convdet', cd, ops.WINO_SK_CFG, 'dgrad'), dA, 0, ymask=out_last, yscale=saved['drop_scale'])
        else:
            base.dgrad3x3('convdet', cd, dpred, 0, dA, ymask=out_last)
            dA.mul_(saved['drop_scale'])
    else:
        base.dgrad3x3('convdet', cd, dpred, 0, dA, ymul=saved['drop_mask'], ymask=out_last)
    for i in range(last, 1, -1):
        l = layers[i]
        if l[0] == 'pool':
            close_stage(f'features.{i + 1}.squeeze.weight')    # the Fire modules behind this pool are done
            if i == 2 and 'stem_pool' in saved:
                continue                                   # folded into the stem weight gradient below
            am, (Hi, Wi) = saved[f'pool{i}']
            # the forward recorded the ReLU mask of the pool's input inside the arg-max codes (ops.maxpool(relu_codes=True)):
            # the gradient that leaves here already carries it, and no activation tensor is re-read for its sign
            dA = ops.maxpool_bwd(dA, am, (Hi, Wi))
            continue
        _, cin, s, e1, e3 = l
        fire = feats[i]
        x_in, sq, _ = saved[f'fire{i}']
        pre = f'features.{i}.'
        fused_e1 = bool(wb.fused.get(pre + 'expand1x1'))

        def grouped(key, item, run_group):
            # a member of a launch group runs with the other members, as soon as the last of them has its gradient (dA stays alive until
            # then); returns False for a layer that has its own launch
            grp = wb.group_of.get(key)
            if grp is None:
                return False
            lst = pending.setdefault(grp[0], [])
            lst.append(item)
            if len(lst) == len(grp[3]):
                run_group(lst, grp)
                del pending[grp[0]]
            return True
        if not fused_e1 and not grouped(pre + 'expand1x1', (dA, 0, e1, sq, 0, s, wb.slab(pre + 'expand1x1')),
                                        lambda lst, grp: ops.conv_wgrad_group(lst, grp[1])):
            ops.conv_wgrad(dA, 0, e1, sq, 0, s, 1, slab=wb.slab(pre + 'expand1x1'))
        if not grouped(pre + 'expand3x3', (dA, e1, e3, sq, 0, s, wb.slab(pre + 'expand3x3')),
                       lambda lst, grp: ops.conv_wgrad_wino_group(lst, grp[1], grp[2])):
            ops.conv_wgrad(dA, e1, e3, sq, 0, s, 9, slab=wb.slab(pre + 'expand3x3'))
        dSq = torch.empty_like(sq)
        if fused_e1:
            # narrow expand1x1 (N <= 128: the first four Fires): weight-gradient slabs and the data gradient from ONE pass over the
            # expand1x1 half of dA; the expand3x3 data gradient below accumulates onto it and applies the squeeze's ReLU mask
            ops.squeeze_bwd(dA, sq, fire.expand1x1.weight, wb.slab(pre + 'expand1x1'), dSq, relu_mask=False, dy_coff=0, N=e1)
        else:
            ops.conv(dA, 0, base.plan(f'{i}.expand1x1', fire.expand1x1, wgrad[pre + 'expand1x1'].dgrad_cfg, 'dgrad'), dSq, 0)
        base.dgrad3x3(f'{i}.expand3x3', fire.expand3x3, dA, e1, dSq, accumulate=True, ymask=sq)
        dIn = torch.empty_like(x_in)
        prev_is_fire = layers[i - 1][0] == 'fire'
        if wb.fused.get(pre + 'squeeze'):
            # weight gradient slabs AND the data gradient in one launch: x_in is streamed once (it used to be read by the weight
            # gradient, and again -- for its sign only -- by the data-gradient kernel's ReLU-mask epilogue)
            ops.squeeze_bwd(dSq, x_in, fire.squeeze.weight, wb.slab(pre + 'squeeze'), dIn, relu_mask=prev_is_fire)
        else:
            ops.conv_wgrad(dSq, 0, s, x_in, 0, cin, 1, slab=wb.slab(pre + 'squeeze'))
            ops.conv(dSq, 0, base.plan(f'{i}.squeeze', fire.squeeze, wgrad[pre + 'squeeze'].dgrad_cfg, 'dgrad'), dIn, 0,
                     ymask=x_in if prev_is_fire else None)
        dA = dIn
    stem = feats[0]
    stem_out = (gview('features.0.weight'), gview('features.0.bias'))
    if 'stem_pool' in saved:
        am, pooled = saved['stem_pool']
        # (the codes carry the ReLU mask: the pooled tensor is not read again)
        ops.stem_wgrad_pooled(dA, None, am, saved['image'].contiguous(), stem.out_channels, stem.kernel_size[0], out=stem_out)
    else:
        ops.stem_wgrad(dA, saved['image'].contiguous(), stem.out_channels, stem.kernel_size[0], out=stem_out)
    if sync is not None:
        lo0 = slots['features.0.weight'][0]
        sync.scale_slice(lo0, lo0 + stem.weight.numel() + stem.bias.numel())      # the stem's gradient does not pass through the slab reduction
    assert not pending, 'a weight-gradient group was left incomplete'
    if sync is None:
        wb.reduce(grad_flat)                               # all 31 Fire / ConvDet slab reductions: one launch
    else:
        close_stage(None)                                  # whatever is left (first stage + stem)
        sync.finish()
    base.last_grad_flat = grad_flat
    return {n: gview(n) for n in slots}


def _param_state(params):
    """What the backward's operands looked like at the forward: the staleness rule of the plan cache (plans.version), per parameter."""
    return [(p._version, p.data_ptr()) for p in params]


class BackboneFn(torch.autograd.Function):
    """The autograd contract around the node ("autograd contract"): the backward reads the parameters LIVE (the plan
    cache re-packs the data-gradient operands from them, ops.squeeze_bwd takes expand1x1 / squeeze weights as they are), so a parameter
    changed since the forward is refused with torch's own error instead of mixing old activations with new weights; the saved
    activations are freed by the first backward, a second one is refused (``retain_graph`` would keep them alive through the
    optimizer step of every training loop)."""

    @staticmethod
    def forward(ctx, base, image, drop_mask, drop, *params):
        pred, saved = run_backbone_forward(base, image.detach(), save=True, drop_mask=drop_mask, drop=drop)
        ctx.base = base
        ctx.saved = saved
        ctx.names = [n for n, _ in base.named_parameters()]
        ctx.params = params
        ctx.param_state = _param_state(params)
        return pred

    @staticmethod
    def backward(ctx, dpred):
        if ctx.saved is None:
            raise RuntimeError('Trying to backward through the graph a second time: SqueezeDetBase frees its saved activations after '
                               'the first backward, with or without retain_graph=True (keeping them would raise the peak memory of '
                               'every training step).  Run the forward again for another backward.')
        for n, p, was in zip(ctx.names, ctx.params, ctx.param_state):
            now = (p._version, p.data_ptr())
            if now != was:
                raise RuntimeError(f'one of the variables needed for gradient computation has been modified by an inplace operation: '
                                   f'parameter {n} of SqueezeDetBase is at version {now[0]}; expected version {was[0]} instead'
                                   + ('' if now[1] == was[1] else ' (and its storage was replaced)')
                                   + '.  The backward reads the parameters as they are now: run it before the optimizer step / EMA '
                                   'update, or run the forward again.')
        grads = run_backbone_backward(ctx.base, ctx.saved, dpred)
        ctx.saved = None
        ctx.params = None
        return (None, None, None, None) + tuple(grads[n] if need else None for n, need in zip(ctx.names, ctx.needs_input_grad[4:]))


def _loss_meta(ctx, loss_mod):
    """ctx.meta = (input_size, num_classes, weights) of the Loss module: what the six loss Functions hand to ops in both passes.  A
    ``bbox_loss`` other than 'l2' rides behind the four weights (``ops.split_loss_weights``)."""
    res = loss_mod.resolver
    ctx.meta = (res.input_size, res.num_classes, (loss_mod.class_loss_weight, loss_mod.positive_score_loss_weight,
                                                  loss_mod.negative_score_loss_weight, loss_mod.bbox_loss_weight))
    kind = getattr(loss_mod, 'bbox_loss', 'l2')
    if kind != 'l2':
        ctx.meta = ctx.meta[:2] + (ctx.meta[2] + (kind,),)
    return ctx.meta


def _coef(g):
    """g [4,B] arriving at (class, score, bbox, total) -> coef [3,B]: the gradient of `total` reaches all three components."""
    return (g[:3] + g[3:4]).contiguous()


def _mean_outputs(ctx, losses, mean4):
    """What the three mean Functions return: the 0-dim view of the total's mean, and the per-image vectors for the statistics."""
    ctx.mark_non_differentiable(losses)
    ctx.set_materialize_grads(False)   # (no zero-filled gradient tensor for the statistics output: that is a fill launch per step)
    return mean4[3], losses


class LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, anchors, loss_mod):
        meta = _loss_meta(ctx, loss_mod)
        losses, nobj = ops.loss_fns(meta[1])[0](pred.detach(), gt, anchors, *meta)
        ctx.save_for_backward(pred.detach(), gt, anchors, nobj)
        return losses                      # [4,B] = (class, score, bbox, total)

    @staticmethod
    def backward(ctx, g):
        pred, gt, anchors, nobj = ctx.saved_tensors
        return ops.loss_fns(ctx.meta[1])[2](pred, gt, anchors, nobj, _coef(g), *ctx.meta), None, None, None


class LossMeanFn(torch.autograd.Function):
    """``Loss(pred, gt)[0].mean()`` (src/engine/trainer.py:43) as ONE autograd node: the batch mean comes out of the loss launch, its
    backward hands the scalar gradient straight to the loss backward kernel -- no torch reduction / select / elementwise kernels
    between the loss and the backbone's backward."""

    @staticmethod
    def forward(ctx, pred, gt, anchors, loss_mod):
        meta = _loss_meta(ctx, loss_mod)
        losses, nobj, mean4 = ops.loss_fns(meta[1])[1](pred.detach(), gt, anchors, *meta)
        ctx.save_for_backward(pred.detach(), gt, anchors, nobj)
        return _mean_outputs(ctx, losses, mean4)

    @staticmethod
    def backward(ctx, g, _gl):
        pred, gt, anchors, nobj = ctx.saved_tensors
        return ops.loss_fns(ctx.meta[1])[3](pred, gt, anchors, nobj, g.reshape(1), *ctx.meta), None, None, None


class LossSparseFn(torch.autograd.Function):
    """``LossFn`` on a sparse ground truth (ops.SparseGT): the loss launches read the list of positives, no dense gt exists."""

    @staticmethod
    def forward(ctx, pred, anchors, loss_mod, *sgt):
        losses, nobj = ops.loss_sparse_fwd(pred.detach(), ops.SparseGT(*sgt), anchors, *_loss_meta(ctx, loss_mod))
        ctx.save_for_backward(pred.detach(), anchors, nobj, *sgt)
        return losses                      # [4,B] = (class, score, bbox, total)

    @staticmethod
    def backward(ctx, g):
        pred, anchors, nobj, *sgt = ctx.saved_tensors
        dpred = ops.loss_sparse_bwd(pred, ops.SparseGT(*sgt), anchors, nobj, _coef(g), *ctx.meta)
        return (dpred, None, None) + (None,) * len(sgt)


class LossSparseMeanFn(torch.autograd.Function):
    """``LossMeanFn`` on a sparse ground truth: mean(total) and its backward inside the sparse loss launches."""

    @staticmethod
    def forward(ctx, pred, anchors, loss_mod, *sgt):
        losses, nobj, mean4 = ops.loss_sparse_mean_fwd(pred.detach(), ops.SparseGT(*sgt), anchors, *_loss_meta(ctx, loss_mod))
        ctx.save_for_backward(pred.detach(), anchors, nobj, *sgt)
        return _mean_outputs(ctx, losses, mean4)

    @staticmethod
    def backward(ctx, g, _gl):
        pred, anchors, nobj, *sgt = ctx.saved_tensors
        dpred = ops.loss_sparse_mean_bwd(pred, ops.SparseGT(*sgt), anchors, nobj, g.reshape(1), *ctx.meta)
        return (dpred, None, None) + (None,) * len(sgt)


class LossMaskedFn(torch.autograd.Function):
    """``LossSparseFn`` with an anchor ignore bitmap (ops.anchor_ignore_mask): ignored anchors are neither positives nor negatives, and
    an object-free image gives finite losses and gradients (ops.loss_masked_*)."""

    @staticmethod
    def forward(ctx, pred, anchors, loss_mod, ignore, *sgt):
        losses, counts = ops.loss_masked_fwd(pred.detach(), ops.SparseGT(*sgt), ignore, anchors, *_loss_meta(ctx, loss_mod))
        ctx.save_for_backward(pred.detach(), anchors, counts, ignore, *sgt)
        return losses                      # [4,B] = (class, score, bbox, total)

    @staticmethod
    def backward(ctx, g):
        pred, anchors, counts, ignore, *sgt = ctx.saved_tensors
        dpred = ops.loss_masked_bwd(pred, ops.SparseGT(*sgt), ignore, anchors, counts, _coef(g), *ctx.meta)
        return (dpred, None, None, None) + (None,) * len(sgt)


class LossMaskedMeanFn(torch.autograd.Function):
    """``LossSparseMeanFn`` with an anchor ignore bitmap: mean(total) and its backward inside the masked loss launches."""

    @staticmethod
    def forward(ctx, pred, anchors, loss_mod, ignore, *sgt):
        losses, counts, mean4 = ops.loss_masked_mean_fwd(pred.detach(), ops.SparseGT(*sgt), ignore, anchors, *_loss_meta(ctx, loss_mod))
        ctx.save_for_backward(pred.detach(), anchors, counts, ignore, *sgt)
        return _mean_outputs(ctx, losses, mean4)

    @staticmethod
    def backward(ctx, g, _gl):
        pred, anchors, counts, ignore, *sgt = ctx.saved_tensors
        dpred = ops.loss_masked_mean_bwd(pred, ops.SparseGT(*sgt), ignore, anchors, counts, g.reshape(1), *ctx.meta)
        return (dpred, None, None, None) + (None,) * len(sgt)
