"""A float64 twin of ``SqueezeDetWithLoss`` in plain torch, and the usage scenarios of the ``nn.Module`` training surface written once
(helper module of tests/test_autograd_twin_host.py and tests/test_autograd_surface_gpu.py; no project kernels).

The twin's parameters carry the state-dict names, its forward is ``oracle.backbone_forward`` followed by ``oracle.multitask_loss`` and
torch's own autograd differentiates it: whatever torch guarantees around a module (accumulation into ``.grad``, several forwards before
a backward, frozen parameters, any upstream gradient, the errors of a misuse) holds for it by construction.  Every scenario below is a
function of ``(model, batches, H)`` that uses public torch calls only; ``H`` hides the one difference between the two models (how a
batch is handed over and where the dropout mask comes from).  The HIP model and the twin run the same function and their ``p.grad``
are compared.

Ground-truth forms: the twin always reads the dense ``gt [B,A,C+9]`` (for a sparse list: ``ops.sparse_gt_to_dense`` of it).  With an
ignore bitmap (``batch['ign']``, bool [B,A]) the loss of an image is the unmasked loss on the rows that are kept -- the identity
tests/ignore_ref.py is built on -- so the loss itself is not restated here.  Images without positives or without negatives have
conventions of their own (ignore_ref) and are not used by the scenarios.
"""
import types

import numpy as np
import torch
import torch.nn as nn

import oracle

F64, F32 = torch.float64, torch.float32

# the bars of tests/test_training_gpu.py::_check_grads_flip_aware (ConvDet: no mask between it and the loss)
TIGHT_NAMES = ('base.convdet.weight', 'base.convdet.bias')
BAR_TIGHT, BAR_MAX, BAR_L2 = 2e-4, 5e-2, 2e-2
DEFAULT_BARS = (BAR_TIGHT, BAR_MAX, BAR_L2)
LOSS_RTOL = 1e-4
WIDEN = 4.0                      # a bar the float32 twin alone exceeds becomes WIDEN x its measured error


class Twin(nn.Module):
    def __init__(self, state_dict, anchors, input_size, arch='squeezedet', num_classes=3, dtype=F64):
        super().__init__()
        self.arch, self.num_classes, self.input_size, self.dtype = arch, int(num_classes), tuple(input_size), dtype
        self.anchors = np.asarray(anchors)
        for name, v in state_dict.items():
            mod = self
            *path, leaf = name.split('.')
            for part in path:
                if part not in mod._modules:
                    mod.add_module(part, nn.Module())
                mod = mod._modules[part]
            mod.register_parameter(leaf, nn.Parameter(v.detach().clone().to(dtype)))

    def predict(self, batch, drop_mask=None):
        """pred [B,A,C+5].  ``drop_mask`` (NCHW, scaled by 1 / (1 - p)) is applied in train mode only, like the module's dropout."""
        image = batch['image']
        image = image if image.dtype == self.dtype else image.to(self.dtype)
        if drop_mask is not None:
            drop_mask = drop_mask.to(self.dtype) if self.training else None
        return oracle.backbone_forward(image, dict(self.named_parameters()), self.arch, self.num_classes, drop_mask)

    def loss_of(self, pred, batch):
        gt = batch['gt'].to(self.dtype)
        ign = batch.get('ign')
        if ign is None:
            return oracle.multitask_loss(pred, gt, self.anchors, self.input_size, self.num_classes)
        ign = torch.as_tensor(np.asarray(ign)).bool()
        rows = []
        for b in range(pred.shape[0]):
            pos = gt[b, :, 0] > 0
            keep = ~(ign[b] & ~pos)
            assert int(pos.sum()) > 0 and int(keep.sum()) > int(pos.sum()), 'the twin takes images with positives and negatives only'
            _, st = oracle.multitask_loss(pred[b:b + 1, keep], gt[b:b + 1, keep], self.anchors[keep.numpy()], self.input_size,
                                          self.num_classes)
            rows.append(st)
        stats = {k: torch.cat([r[k] for r in rows]) for k in rows[0]}
        return stats['loss'], stats

    def forward(self, batch, drop_mask=None, want_pred=False):
        """-> (loss [B], stats dict) like ``SqueezeDetWithLoss.forward``; with ``want_pred`` also pred."""
        pred = self.predict(batch, drop_mask)
        loss, stats = self.loss_of(pred, batch)
        return (loss, stats, pred) if want_pred else (loss, stats)


class TwinHelpers:
    """How a scenario talks to the twin.  ``masks``: the dropout masks of the forwards to come, in order (NCHW; read back from the
    HIP model's stream on the GPU tier, drawn from a seed on the CPU tier); one is consumed per train-mode forward."""

    def __init__(self, masks=None):
        self.masks = list(masks) if masks is not None else None

    def _mask(self, model):
        if self.masks is None or not model.training:
            return None
        return self.masks.pop(0)

    def forward(self, model, batch):
        return model(batch, drop_mask=self._mask(model))

    def forward_mean(self, model, batch):
        loss, stats = model(batch, drop_mask=self._mask(model))
        return loss.mean(), {k: v.detach() for k, v in stats.items()}

    def pred(self, model, batch):
        return model.predict(batch, self._mask(model))


def snap(model):
    return {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}


def random_masks(shapes, seed, p=0.5):
    """Scaled keep masks (NCHW) of the given shapes from one seeded stream: the CPU tier's stand-in for the device stream."""
    rs = np.random.RandomState(seed)
    return [torch.from_numpy((rs.uniform(size=s) >= p).astype(np.float64) / (1.0 - p)) for s in shapes]


# ---- the scenarios -----------------------------------------------------------------------------------------------------------------------

def sc_single(model, batches, H, which=0):
    """One forward, ``loss.mean().backward()``: the loop every other test enters the library through."""
    loss, _ = H.forward(model, batches[which])
    loss.mean().backward()
    return {'loss': loss.detach(), 'grads': snap(model)}


def sc_accumulate(model, batches, H, mode='plain'):
    """Micro-batch A then B, each forward followed by its backward, no ``zero_grad`` in between.  ``mode``: 'plain'; 'zero_first'
    (gradients exist and are zeroed in place with ``zero_grad(set_to_none=False)`` before the pair); 'mean' (through ``forward_mean``)."""
    A, B = batches
    out = {}
    if mode == 'zero_first':
        loss, _ = H.forward(model, A)
        loss.mean().backward()
        model.zero_grad(set_to_none=False)
    for tag, b in (('A', A), ('B', B)):
        if mode == 'mean':
            mean, stats = H.forward_mean(model, b)
            out['loss_' + tag] = stats['loss'].detach()
            mean.backward()
        else:
            loss, _ = H.forward(model, b)
            out['loss_' + tag] = loss.detach()
            loss.mean().backward()
    out['grads'] = snap(model)
    return out


def sc_forwards_first(model, batches, H):
    """Forward A, forward B, backward B, backward A (dropout on: each backward must use its own forward's mask)."""
    A, B = batches
    la, _ = H.forward(model, A)
    lb, _ = H.forward(model, B)
    lb.mean().backward()
    gb = snap(model)
    model.zero_grad()
    la.mean().backward()
    return {'loss_A': la.detach(), 'loss_B': lb.detach(), 'grads_B': gb, 'grads_A': snap(model)}


def frozen_but_convdet(name):
    return not name.startswith('base.convdet.')


def frozen_middle_fire(name):
    return name.startswith('base.features.6.')


def frozen_all(name):
    return True


def sc_frozen(model, batches, H, frozen):
    """``frozen(name)`` -> the parameter does not require grad.  With every parameter frozen nothing is differentiable."""
    for n, p in model.named_parameters():
        p.requires_grad_(not frozen(n))
    if all(frozen(n) for n, _ in model.named_parameters()):
        pred = H.pred(model, batches[0])
        return {'pred_requires_grad': pred.requires_grad, 'pred_grad_fn': pred.grad_fn, 'grads': snap(model)}
    loss, _ = H.forward(model, batches[0])
    loss.mean().backward()
    return {'loss': loss.detach(), 'grads': snap(model)}


FOREIGN_KINDS = ('sum', 'sq3', 'image0', 'transpose', 'x1024', 'x2^-10')


def sc_foreign(model, batches, H, kind, hook=None):
    """An upstream gradient on ``pred`` that no loss kernel produced.  ``hook``: registered on pred (the CPU tier reads the strides
    of the gradient that reaches the backbone's node with it)."""
    A = batches[0]
    if kind in ('x1024', 'x2^-10'):
        loss, _ = H.forward(model, A)
        (loss.mean() * (1024.0 if kind == 'x1024' else 2.0 ** -10)).backward()
        return {'grads': snap(model)}
    pred = H.pred(model, A)
    if hook is not None:
        pred.register_hook(hook)
    Bn, An, Wn = pred.shape
    rs = np.random.RandomState(77)
    if kind == 'sum':
        s = pred.sum()                                           # an expanded (stride-0) gradient
    elif kind == 'sq3':
        s = (pred[..., :3] ** 2).sum()                           # zero outside the first three columns
    elif kind == 'image0':
        w = torch.from_numpy(rs.standard_normal((An, Wn))).to(pred)
        s = (pred[0] * w).sum()                                  # image 1 gets an all-zero gradient
    elif kind == 'transpose':
        w = torch.from_numpy(rs.standard_normal((Bn, Wn, An))).to(pred)
        s = (pred.transpose(1, 2) * w).sum()                     # a non-contiguous gradient
    else:
        raise ValueError(kind)
    s.backward()
    return {'grads': snap(model)}


def sc_eval_with_grad(model, batches, H):
    """Eval mode, grad enabled: no dropout, the gradients are those of the mask-free forward."""
    model.eval()
    loss, _ = H.forward(model, batches[0])
    loss.mean().backward()
    return {'loss': loss.detach(), 'grads': snap(model)}


def sc_train_no_grad(model, batches, H):
    """Train mode under ``torch.no_grad()``: the dropout applies, nothing is differentiable."""
    with torch.no_grad():
        loss, _ = H.forward(model, batches[0])
    return {'loss': loss.detach(), 'requires_grad': loss.requires_grad, 'grad_fn': loss.grad_fn}


def sc_loss_component(model, batches, H, which):
    """Backward through one statistic, or a mixture of one with ``loss.mean()``."""
    loss, stats = H.forward(model, batches[0])
    if which == 'mixture':
        s = 0.5 * stats['class_loss'].sum() + 2.0 * loss.mean()
    else:
        s = stats[which].sum()
    s.backward()
    return {'loss': loss.detach(), 'grads': snap(model)}


INPLACE_PARAM = 'base.features.6.expand3x3.weight'


def sc_inplace_update(model, batches, H, out, name=INPLACE_PARAM):
    """An in-place parameter update between forward and backward (an optimizer step, an EMA).  torch raises in backward."""
    loss, _ = H.forward(model, batches[0])
    with torch.no_grad():
        dict(model.named_parameters())[name].add_(1e-3)
    try:
        loss.mean().backward()
    finally:
        out['grads'] = snap(model)


def sc_second_backward(model, batches, H, out, retain, via='loss'):
    """backward twice through the same forward.  ``via``: 'loss' (``loss.mean()``: the loss node is passed first) or 'pred'
    (``pred.sum()``: nothing but the backbone holds saved tensors).  ``out`` receives the gradients after the first and after the
    second call (also when the second raises)."""
    if via == 'pred':
        s = H.pred(model, batches[0]).sum()
    else:
        loss, _ = H.forward(model, batches[0])
        s = loss.mean()
    s.backward(retain_graph=retain)
    out['first'] = snap(model)
    try:
        s.backward(retain_graph=retain)
    finally:
        out['second'] = snap(model)


def sc_image_requires_grad(model, batches, H, out):
    """The image is a leaf that requires grad."""
    A = dict(batches[0])
    A['image'] = A['image'].detach().clone().requires_grad_()
    loss, _ = H.forward(model, A)
    loss.mean().backward()
    out['image_grad'] = A['image'].grad


# ---- comparing gradients -----------------------------------------------------------------------------------------------------------------

def _as_params(grads, names=None):
    return [(n, types.SimpleNamespace(grad=g)) for n, g in grads.items() if (names is None or n in names)]


def measure(got, ref, names=None):
    """-> (worst max-abs error over the tensor's scale among the ConvDet tensors, the same among all, worst relative L2): the three
    quantities ``_check_grads_flip_aware`` bounds."""
    tight = mx = l2 = 0.0
    for n, g in got.items():
        if names is not None and n not in names:
            continue
        r = ref[n].float()
        g = g.detach().cpu().float()
        scale = max(float(r.abs().max()), 1e-3)
        err = float((g - r).abs().max()) / scale
        rel2 = float((g - r).norm() / max(float(r.norm()), 1e-12))
        if n in TIGHT_NAMES:
            tight = max(tight, err)
        mx, l2 = max(mx, err), max(l2, rel2)
    return tight, mx, l2


def widened(meas32):
    """The bars of a scenario given what the float32 twin alone measures against the float64 twin: the project's own where the
    float32 chain stays inside them, else WIDEN x the measured figure (headroom for the kernels' other summation order)."""
    return tuple(b if m <= b else WIDEN * m for m, b in zip(meas32, DEFAULT_BARS))


def check_grads(got, ref, bars=DEFAULT_BARS, names=None):
    """``got`` / ``ref``: {name: gradient}.  At the project's own bars this IS ``_check_grads_flip_aware``; with widened bars the same
    three quantities against them."""
    assert all(g is not None for n, g in got.items() if names is None or n in names), 'a trainable parameter has no gradient'
    if tuple(bars) == DEFAULT_BARS:
        from test_training_gpu import _check_grads_flip_aware
        _check_grads_flip_aware(_as_params(got, names), ref)
        return
    tight, mx, l2 = measure(got, ref, names)
    assert tight <= bars[0] and mx <= bars[1] and l2 <= bars[2], ((tight, mx, l2), bars)


def check_frozen(grads, frozen):
    """A frozen parameter's ``.grad`` is None (not a zero tensor), every other parameter has one."""
    for n, g in grads.items():
        if frozen(n):
            assert g is None, f'{n}: frozen, but has a gradient'
        else:
            assert g is not None, f'{n}: trainable, but has no gradient'


def check_loss(got, ref):
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), ref.detach().double().numpy(), rtol=LOSS_RTOL)


def scaled_pair_mask(g_big, g_small):
    """Elements on which ``g_big == g_small * 2**20`` must hold bit for bit: neither is subnormal in float32, and neither is zero
    unless both are (the weight gradients of a channel whose ReLU never fires are exact zeros at any scale -- almost half of all
    elements at 64x96 -- and stay under the assertion; excluding them would make the excluded share a property of the network)."""
    tiny = float(np.finfo(np.float32).tiny)
    return ((g_big.abs() >= tiny) & (g_small.abs() >= tiny)) | ((g_big == 0) & (g_small == 0))


# ---- operands ----------------------------------------------------------------------------------------------------------------------------

SIZE = (64, 96)


def make_cases(cfg, num_classes=3, ignore_density=None):
    """Micro-batch A (2 images: the operands of test_full_backward_vs_oracle) and B (1 image) on the host in float32:
    {'image', 'gt'[, 'ign']}."""
    from squeezedet_pytorch_amd import synthetic
    cases = []
    for n, si, sg in ((2, 3, 2), (1, 4, 5)):
        c = {'image': synthetic.make_images(n, SIZE, seed=si),
             'gt': synthetic.make_gt(n, cfg.anchors, SIZE, num_classes, seed=sg, min_boxes=2, max_boxes=3)}
        if ignore_density is not None:
            rs = np.random.RandomState(100 + si)
            c['ign'] = rs.rand(n, cfg.anchors.shape[0]) < ignore_density
        cases.append(c)
    return cases


def twin_batches(cases, dtype=F64):
    return [{k: (v.to(dtype) if isinstance(v, torch.Tensor) else v) for k, v in c.items()} for c in cases]
