"""Every launch decision of one inference or training step, taken on the host WITHOUT a GPU: which kernel instance (tile
configuration from the measured table ``tuning.json``) every layer launches for a given architecture / batch / input size.
``forward_schedule`` decides the forward (stem form, pools, squeeze, which launch takes a Fire's expand pair, dropout),
``backward_schedule`` the backward (fused squeeze backward, grouped weight gradients, ConvDet's data gradient) and
``conv3x3_cfg`` a plain 3x3 launch.  The executors (``autograd.run_backbone_forward``, ``backward.run_backbone_backward``,
``SqueezeDetBase.conv3x3``) walk these schedules; ``inference_launch_plan`` / ``training_launch_plan`` render the same schedules as
(kernel name, shape tag) lists.  GPU tests assert the rendering equals the real launches name for name and shape for shape
(tests/test_surface_gpu.py), for the default and for non-default model flags, so that profiles can be checked against the code
that shipped: ``profiles/traffic.json`` records the launch set it was measured on (inference at top level, training under
``"train"``) and a CPU test recomputes that set here.

Reference for the layer sequence: src/model/squeezedet.py:33-87, src/engine/detector.py:20-50, src/engine/trainer.py:42-50.
"""
from __future__ import annotations

import functools
from collections import Counter, namedtuple

from . import ops
from .synthetic import convdet_in_channels, layer_table

# the model switches (``SqueezeDetBase`` attributes of the same names) the forward schedule depends on
Flags = namedtuple('Flags', 'use_winograd fuse_expand fuse_expand_wino fuse_fire_bridge fuse_pool_squeeze fuse_stem_squeeze '
                            'fuse_train_forward fused_dropout')
# One record per stem / pool / Fire / ConvDet, in layer order; (H, W, C) = the layer's input.
# form: stem_conv | stem_pool | stem_pool_sq | stem_pool_sq_train (the last two also run the first Fire's squeeze, width sq)
StemStep = namedtuple('StemStep', 'form ks sq')
# how: launch | folded (into the next squeeze: pool_squeeze) | done (by the previous launch)
PoolStep = namedtuple('PoolStep', 'i H W C how')
# squeeze: conv (cfg sq_cfg) | pool_squeeze | done.  expand: fire_pool_bridge[_save] (cfg = segments) | fire_bridge[_save] | fire_wino |
# fire_expand | conv_drop (cfg: expand1x1 with the fused dropout, expand3x3 on the balanced Winograd kernel) | plain (cfg: expand1x1);
# nsq: width of the next Fire's squeeze a bridge also runs.  mask_launch: the stand-alone dropout_mask launch precedes this Fire's
# squeeze; ymul: the plain pair multiplies a mask tensor (given or just drawn) in.
FireStep = namedtuple('FireStep', 'i H W C s e1 e3 mask_launch squeeze sq_cfg expand cfg nsq ymul')
ConvDetStep = namedtuple('ConvDetStep', 'H W C fused_rng')      # fused_rng: the dropout ran inside the last Fire's expand launches
# One record per weight gradient, keyed by the parameter prefix.  fused: it comes out of squeeze_bwd; group: its launch group
# (a ``tiles.wino_wgrad_groups`` value) or None; dgrad_cfg: configuration of a 1x1 layer's own data-gradient launch.
WgradStep = namedtuple('WgradStep', 'N C taps shape fused group dgrad_cfg')

_CHOOSERS = ('choose_cfg', 'choose_wino_cfg', 'choose_fire_wino_cfg', 'choose_fused_cfg', 'choose_fire_bridge_cfg', 'choose_fire_pool_bridge',
             'conv_drop_cfg', 'stem_pool_squeeze_ok', 'pool_squeeze_ok', 'squeeze_bwd_ok', 'wino_wgrad_groups', 'wgrad1x1_groups')


def _choosers():
    """The table look-ups as they stand in ``ops`` now.  Part of the memo keys below: a schedule is only answered from the memo while
    the look-ups are the ones it was built with (tests force forms by swapping them).  Whoever edits the loaded tuning table in place
    calls ``forward_schedule.cache_clear()`` / ``backward_schedule.cache_clear()``."""
    return tuple(getattr(ops, n) for n in _CHOOSERS)


def conv3x3_cfg(C, N, npix, use_winograd):
    """A plain 3x3 launch (forward, or data gradient with C / N swapped): (True, Winograd configuration) where the measured table has
    the row, else (False, configuration of the direct kernel)."""
    wc = ops.choose_wino_cfg(C, N, npix) if use_winograd else None
    return (True, wc) if wc is not None else (False, ops.choose_cfg(9, C, N, npix))


def forward_schedule(arch, batch, input_size, flags, save=False, dropout=None):
    """-> tuple of StemStep / PoolStep / FireStep ... ConvDetStep.  ``save``: the forward keeps what the backward reads.  ``dropout``
    (in front of ConvDet): None, 'stream' (the counter-based stream) or 'mask' (a given mask tensor)."""
    return _forward_schedule(arch, int(batch), (int(input_size[0]), int(input_size[1])), flags, bool(save), dropout, _choosers())


@functools.lru_cache(maxsize=256)
def _forward_schedule(arch, batch, input_size, flags, save, dropout, _key):
    layers = layer_table(arch)
    assert layers[-1][0] == 'fire'                     # (ConvDet and the dropout in front of it sit behind a Fire)

    def kind(j):
        return layers[j][0] if j < len(layers) else None
    C, ks = layers[0][2], layers[0][3]
    H, W = ops.stem_out_size(input_size[0], input_size[1], ks)
    first, bridged, folded = 2, False, False           # bridged: the next Fire's squeeze already ran inside the previous launch
    if kind(2) == 'pool':
        # conv + ReLU + pool in one launch; with the first Fire's squeeze riding in it (a saving forward: in its storing form)
        bridged = bool(flags.fuse_stem_squeeze and (flags.fuse_train_forward if save else True) and kind(3) == 'fire'
                       and ops.stem_pool_squeeze_ok((batch, 3) + input_size, (C, 3, ks, ks), layers[3][2]))
        steps = [StemStep(('stem_pool_sq_train' if save else 'stem_pool_sq') if bridged else 'stem_pool', ks, layers[3][2] if bridged else None),
                 PoolStep(2, H, W, C, 'done')]
        H, W = ops.pool_out_size(H, W)
        first = 3
    else:
        steps = [StemStep('stem_conv', ks, None)]
    for i in range(first, len(layers)):
        if kind(i) == 'pool':
            folded = bool(not bridged and not save and flags.fuse_pool_squeeze and kind(i + 1) == 'fire' and ops.pool_squeeze_ok(C, layers[i + 1][2]))
            steps.append(PoolStep(i, H, W, C, 'done' if bridged else 'folded' if folded else 'launch'))
            H, W = ops.pool_out_size(H, W)
            continue
        _, cin, s, e1, e3 = layers[i]
        assert C == cin, f'layer {i}: expected {cin} channels, got {C}'
        npix = batch * H * W
        is_last = i == len(layers) - 1
        drop_here = dropout if is_last else None       # (the last Fire carries the dropout in its expand epilogues: two plain launches)
        if bridged:
            squeeze, sq_cfg = 'done', None
        elif folded:
            squeeze, sq_cfg = 'pool_squeeze', ops.POOL_SQUEEZE_CFG
        else:
            squeeze, sq_cfg = 'conv', ops.choose_cfg(1, cin, s, npix)
        # which launch takes the expand pair, in the order the forms are tried.  The bridges also run the next Fire's squeeze:
        # inference forms (the expand output is never written), or -- a saving forward -- storing forms
        bridge = flags.fuse_fire_bridge and flags.use_winograd and (flags.fuse_train_forward if save else not drop_here)
        expand, cfg, nsq = 'plain', None, None
        if bridge and kind(i + 1) == 'pool' and kind(i + 2) == 'fire':
            cfg = ops.choose_fire_pool_bridge(s, e1, e3, layers[i + 2][2], npix)
            if cfg is not None:
                expand, nsq = 'fire_pool_bridge', layers[i + 2][2]
        if cfg is None and bridge and kind(i + 1) == 'fire' and not (is_last and dropout):
            cfg = ops.choose_fire_bridge_cfg(s, e1, e3, layers[i + 1][2], npix)
            if save and cfg is not None and cfg % 1000 != 12:          # (only the small-C form has a storing variant)
                cfg = None
            if cfg is not None:
                expand, nsq = 'fire_bridge', layers[i + 1][2]
        if cfg is not None and save:
            expand += '_save'
        if cfg is None and not save and not drop_here:
            if flags.fuse_expand_wino and flags.use_winograd:
                cfg = ops.choose_fire_wino_cfg(s, e1, e3, npix)
                expand = 'fire_wino' if cfg is not None else expand
            if cfg is None and flags.fuse_expand and e1 == e3:
                cfg = ops.choose_fused_cfg(s, e1, npix)
                expand = 'fire_expand' if cfg is not None else expand
        mask_launch = False
        if drop_here == 'stream':
            # the fused form needs a weight-stationary 1x1 configuration and the balanced Winograd kernel (8 | squeeze width);
            # otherwise this step's mask is drawn as a tensor by the stand-alone kernel and multiplied in like a given mask
            cfg = ops.conv_drop_cfg(s, e1, npix) if (flags.fused_dropout and s % 8 == 0 and flags.use_winograd) else None
            expand, mask_launch = ('conv_drop', False) if cfg is not None else ('plain', True)
        if expand == 'plain':
            cfg = ops.choose_cfg(1, s, e1, npix)
        steps.append(FireStep(i, H, W, C, s, e1, e3, mask_launch, squeeze, sq_cfg, expand, cfg, nsq, bool(drop_here) and expand == 'plain'))
        bridged, folded = nsq is not None, False
        C = e1 + e3
    steps.append(ConvDetStep(H, W, C, steps[-1].expand == 'conv_drop'))
    return tuple(steps)


forward_schedule.cache_clear = _forward_schedule.cache_clear


def backward_schedule(arch, shapes, ncd, fuse_squeeze_bwd, group_wgrad, fused_rng):
    """-> ({parameter prefix ('convdet', 'features.{i}.expand1x1', ...): WgradStep} in backward order, whether ConvDet's data
    gradient runs on the balanced Winograd kernel).  ``shapes``: (B, H, W) of every Fire, in layer order; ``ncd``: ConvDet's
    output channels; ``fused_rng``: ``ConvDetStep.fused_rng`` of the forward."""
    return _backward_schedule(arch, tuple(tuple(s) for s in shapes), ncd, bool(fuse_squeeze_bwd), group_wgrad, bool(fused_rng), _choosers())


@functools.lru_cache(maxsize=256)
def _backward_schedule(arch, shapes, ncd, fuse_squeeze_bwd, group_wgrad, fused_rng, _key):
    layers = layer_table(arch)
    back = [i for i in range(len(layers) - 1, 1, -1) if layers[i][0] == 'fire']
    shp = dict(zip(back[::-1], shapes))

    def fused(N, C):
        return fuse_squeeze_bwd and ops.squeeze_bwd_ok(N, C)
    # expand3x3 weight gradients that share a launch: the Fire modules between two pools (same grid), same tile form ...
    groups = ops.wino_wgrad_groups([(f'features.{i}.expand3x3', layers[i][4], layers[i][2]) + shp[i] for i in back], enabled=group_wgrad)
    # ... and the expand1x1 weight gradients that are too wide for the fused squeeze backward (their own direct-form launch otherwise)
    groups.update(ops.wgrad1x1_groups([(f'features.{i}.expand1x1', layers[i][3], layers[i][2]) + shp[i] for i in back
                                       if not fused(layers[i][3], layers[i][2])], enabled=group_wgrad))
    out = {'convdet': WgradStep(ncd, convdet_in_channels(arch), 9, shp[back[0]], False, None, None)}
    for i in back:
        _, cin, s, e1, e3 = layers[i]
        npix = shp[i][0] * shp[i][1] * shp[i][2]
        for name, N, C, taps in (('expand1x1', e1, s, 1), ('expand3x3', e3, s, 9), ('squeeze', s, cin, 1)):
            f = taps == 1 and fused(N, C)
            out[f'features.{i}.{name}'] = WgradStep(N, C, taps, shp[i], f, None if f else groups.get(f'features.{i}.{name}'),
                                                   None if (f or taps == 9) else ops.choose_cfg(1, N, C, npix))
    return out, fused_rng and ncd % 8 == 0


backward_schedule.cache_clear = _backward_schedule.cache_clear


def _tap1(cfg, Cin, N, H, W):
    return (ops.cfg_kernel_name(cfg), f'1tap C{Cin} N{N} {H}x{W}')


def _conv3x3(batch, H, W, Cin, N, use_winograd):
    wino, cfg = conv3x3_cfg(Cin, N, batch * H * W, use_winograd)
    return (ops.wino_kernel_name(cfg) if wino else ops.cfg_kernel_name(cfg), f'9tap C{Cin} N{N} {H}x{W}')


def _render_forward(steps, batch, input_size, use_winograd):
    """The forward schedule up to the last Fire as (kernel name, shape tag), as ``ops`` brackets the launches."""
    h, w = input_size
    plan = []
    for prev, st in zip((None,) + steps, steps[:-1]):
        if type(st) is StemStep:
            tag = 'stem' if st.form == 'stem_conv' else 'stem+pool' if st.sq is None else 'stem+pool+squeeze'
            plan.append((f'{st.form}<{st.ks}>', f'{tag} {h}x{w}' + (f' S{st.sq}' if st.sq is not None else '')))
        elif type(st) is PoolStep:
            if st.how == 'launch':
                plan.append(('maxpool_fwd', f'pool C{st.C} {st.H}x{st.W}'))
        else:
            H, W, s, e1, e3 = st.H, st.W, st.s, st.e1, st.e3
            if st.mask_launch:
                plan.append(('dropout_mask', f'{batch * H * W * (e1 + e3)} elements'))
            if st.squeeze == 'pool_squeeze':
                plan.append(('pool_squeeze', f'pool+squeeze C{st.C} N{s} {prev.H}x{prev.W}'))
            elif st.squeeze == 'conv':
                plan.append(_tap1(st.sq_cfg, st.C, s, H, W))
            if st.expand.startswith('fire_pool_bridge'):
                plan.append((st.expand, f'fire C{s} E{e1}+{e3} -> pool -> S{st.nsq} {H}x{W}'))
            elif st.expand.startswith('fire_bridge'):
                plan.append((st.expand, f'fire C{s} E{e1}+{e3} -> S{st.nsq} {H}x{W}'))
            elif st.expand == 'fire_wino':
                plan.append((ops.fire_wino_kernel_name(st.cfg), f'fire C{s} E{e1}+{e3} {H}x{W}'))
            elif st.expand == 'fire_expand':
                plan.append((ops.cfg_kernel_name(st.cfg).replace('conv_dma', 'fire_expand'), f'expand C{s} E{e1} {H}x{W}'))
            else:
                plan.append(_tap1(st.cfg, s, e1, H, W))
                plan.append(('conv_wino_sk', f'9tap C{s} N{e3} {H}x{W}') if st.expand == 'conv_drop' else _conv3x3(batch, H, W, s, e3, use_winograd))
    return plan


def inference_launch_plan(arch='squeezedet', batch=20, input_size=(384, 1248), anchors_per_grid=9, num_classes=3,
                          use_winograd=True, fuse_expand=True, fuse_fire_bridge=True, fuse_expand_wino=True,
                          fuse_pool_squeeze=False, fuse_stem_squeeze=True, keep_top_k=64):
    """-> list of (kernel name as bench.py / KernelTimer prints it, shape tag), in launch order.  The six switches are
    ``SqueezeDetBase``'s attributes of the same names, one to one; ``keep_top_k`` = ``cfg.keep_top_k`` (with the class and anchor
    counts it decides which fused detect runs: ``ops.detect_fn``)."""
    flags = Flags(use_winograd, fuse_expand, fuse_expand_wino, fuse_fire_bridge, fuse_pool_squeeze, fuse_stem_squeeze, True, True)
    steps = forward_schedule(arch, batch, input_size, flags)
    plan = _render_forward(steps, batch, input_size, use_winograd)
    H, W = steps[-1].H, steps[-1].W
    ncd, npad = ops.convdet_width(anchors_per_grid, num_classes)
    # (a width the convolution forms do not take runs zero-padded into a scratch and is packed into the contiguous pred)
    plan.append(_conv3x3(batch, H, W, convdet_in_channels(arch), npad, use_winograd))
    if npad != ncd:
        plan.append(('convdet_pack', f'pack N{ncd} <- {npad} {H}x{W}'))
    A = H * W * anchors_per_grid
    fused = ops.detect_fn(num_classes, keep_top_k, A)
    plan.append(('detect', f'detect A{A}' if fused is ops.detect else f'{fused.__name__} A{A} K{int(keep_top_k)}'))
    return plan


def _wgrad(batch, H, W, N, C, taps):
    if ops.wgrad_uses_wino(N, C, taps, batch, H, W):
        return ('conv_wgrad_wino', f'wgrad 9tap C{C} N{N} {H}x{W}')
    return (f'conv_wgrad<{taps}>', f'wgrad {taps}tap C{C} N{N} {H}x{W}')


def training_launch_plan(arch='squeezedet', batch=20, input_size=(384, 1248), anchors_per_grid=9, num_classes=3,
                         use_winograd=True, data_parallel_stages=False, fuse_squeeze_bwd=True, dropout=True,
                         fused_dropout=True, fuse_train_forward=True, fuse_fire_bridge=True, fuse_stem_squeeze=True, group_wgrad=None,
                         sparse_gt=False, ignore_regions=False):
    """Launches of one training iteration's forward (activations saved; ``fuse_train_forward``: the stem + squeeze launch and the
    two small-C bridges run in their STORING forms -- what the backward reads is written by the fused launch -- where the table has
    their rows; the other inference-only fusions stay off), multi-task loss forward / backward and the backbone backward, as
    (kernel name, shape tag) in launch order.  The optimizer launch and torch's own elementwise kernels (``loss.mean()``) are not
    KernelTimer-bracketed and not listed.  ``data_parallel_stages``: with a gradient exchange
    attached the slab reduction runs once per backward stage instead of once at the end.  ``fuse_squeeze_bwd`` / ``group_wgrad`` =
    ``SqueezeDetBase``'s attributes.  ``dropout`` (``cfg.dropout_prob > 0``): the counter-based dropout in front of ConvDet rides
    in the last Fire's expand launches (a weight-stationary 1x1 configuration + the balanced Winograd kernel) and ConvDet's data
    gradient runs on the balanced Winograd kernel (mask = its own input, constant scale); where that form does not apply
    (``fused_dropout`` off, squeeze width not a multiple of 8) the mask is drawn by the stand-alone ``dropout_mask`` launch.
    ``sparse_gt`` (``cfg.sparse_gt``): the two loss rows are the sparse launches' (``ops.loss_sparse_*``); everything else is the same.
    ``ignore_regions`` (a batch with ``'gt_ignore'``, ``cfg.ignore_overlap``; needs ``sparse_gt``): the two loss rows are the masked
    launches' (``ops.loss_masked_*``)."""
    if ignore_regions and not sparse_gt:
        raise ValueError('training_launch_plan: ignore_regions needs sparse_gt (the dense loss has no masked form)')
    flags = Flags(use_winograd, True, True, fuse_fire_bridge, False, fuse_stem_squeeze, fuse_train_forward, fused_dropout)
    steps = forward_schedule(arch, batch, input_size, flags, True, 'stream' if dropout else None)
    plan = _render_forward(steps, batch, input_size, use_winograd)
    H, W = steps[-1].H, steps[-1].W
    ntrue, ncd = ops.convdet_width(anchors_per_grid, num_classes)      # ncd: the width ConvDet's launches run at
    padded = ncd != ntrue
    ccd = convdet_in_channels(arch)
    plan.append(_conv3x3(batch, H, W, ccd, ncd, use_winograd))
    if padded:
        plan.append(('convdet_pack', f'pack N{ntrue} <- {ncd} {H}x{W}'))
    A = H * W * anchors_per_grid
    kind = 'loss_masked' if ignore_regions else ('loss_sparse' if sparse_gt else 'loss')
    plan.append((kind + '_fwd', f'loss A{A}'))
    plan.append((kind + '_bwd', f'lossbwd A{A}'))
    # ---- backward ----
    wgrad, convdet_sk = backward_schedule(arch, [(batch, st.H, st.W) for st in steps if type(st) is FireStep], ncd, fuse_squeeze_bwd,
                                          group_wgrad, steps[-1].fused_rng)
    if padded:
        plan.append(('convdet_unpack', f'unpack N{ntrue} -> {ncd} {H}x{W}'))
    plan.append(_wgrad(batch, H, W, ncd, ccd, 9))
    if padded:                                         # its slabs are reduced on their own, over the first ntrue rows
        plan.append(('wgrad_reduce_rows', f'N{ntrue} of {ncd} C{ccd}'))
    # ConvDet data gradient (balanced kernel: mask = its own input, constant scale)
    plan.append(('conv_wino_sk', f'9tap C{ncd} N{ccd} {H}x{W}') if convdet_sk else _conv3x3(batch, H, W, ncd, ccd, use_winograd))
    rows_total, rows_done = (0 if padded else 1), 0    # slab-reduction records: ConvDet (unless padded), then 3 per Fire in backward order
    pending = {}                                       # group id -> shape tags of the members seen so far (issued with the last one)
    ks = steps[0].ks
    for st in reversed(steps[1:-1]):
        if type(st) is PoolStep:
            if data_parallel_stages and rows_total > rows_done:         # a stage of the backward is complete: its bucket goes out
                plan.append(('wgrad_reduce_batched', f'{rows_total - rows_done} layers'))
                rows_done = rows_total
            if st.i != 2:                                               # (the stem's pool is folded into the stem weight gradient)
                plan.append(('maxpool_bwd', f'poolbwd C{st.C} {st.H}x{st.W}'))
            continue
        H, W, s, e1, e3 = st.H, st.W, st.s, st.e1, st.e3
        w1, w3, wsq = (wgrad[f'features.{st.i}.{n}'] for n in ('expand1x1', 'expand3x3', 'squeeze'))
        for w, kernel in ((w1, 'conv_wgrad_group<1>'), (w3, 'conv_wgrad_wino_group')):
            if w.group is not None:
                gid, _S, _tc, members = w.group
                pending.setdefault(gid, []).append(f'C{w.C} N{w.N}')
                if len(pending[gid]) == len(members):
                    plan.append((kernel, f'wgrad {w.taps}tap {" + ".join(pending.pop(gid))} {H}x{W}'))
            elif not w.fused:
                plan.append(_wgrad(batch, H, W, w.N, w.C, w.taps))
        if w1.fused:
            plan.append(('squeeze_bwd', f'sqbwd C{s} N{e1} {H}x{W}'))                  # expand1x1 weight + data gradient, one launch
        else:
            plan.append(_tap1(w1.dgrad_cfg, e1, s, H, W))                             # expand1x1 data gradient
        plan.append(_conv3x3(batch, H, W, e3, s, use_winograd))                       # expand3x3 data gradient (accumulates)
        if wsq.fused:
            plan.append(('squeeze_bwd', f'sqbwd C{st.C} N{s} {H}x{W}'))               # squeeze weight + data gradient, one launch
        else:
            plan.append(_wgrad(batch, H, W, s, st.C, 1))
            plan.append(_tap1(wsq.dgrad_cfg, s, st.C, H, W))                          # squeeze data gradient
        rows_total += 3
    Hs, Ws = input_size
    if steps[0].form == 'stem_conv':
        plan.append((f'stem_wgrad<{ks}>', f'stem wgrad {Hs}x{Ws}'))
    else:
        plan.append((f'stem_wgrad_pooled<{ks}>', f'stem wgrad (pooled) {Hs}x{Ws}'))
    if rows_total > rows_done:
        plan.append(('wgrad_reduce_batched', f'{rows_total - rows_done} layers'))
    return plan


def launches_per_kernel(plan):
    """{kernel name: launches per step}."""
    return dict(Counter(name for name, _ in plan))
