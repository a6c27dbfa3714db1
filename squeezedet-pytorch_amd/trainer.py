"""The training loop: a ``Trainer`` with the reference's interface (src/engine/trainer.py:9-92), the collate helper
``encode_sparse_batch`` and the benchmark's ``make_train_step``.

The pieces it drives live in modules of their own, and every public name of theirs is re-exported here (``trainer`` is the one
import point of the training path, as in the reference):

* ``exchange``: the process-per-GPU gradient exchange (``GradientExchange``, ``attach_data_parallel``) and the rank seeding
* ``optim``: the one-launch optimizers ``FusedClipSGD`` / ``FusedClipAdamW`` (clip + step + weight EMA, csrc/optim.hip)
* ``graph_step``: ``GraphedStep``, the training step replayed as one captured hipGraph
"""
from __future__ import annotations

import time

import torch

from .exchange import (_RANK_STREAMS, GradientExchange, _dist, allreduce_gradients, attach_data_parallel,  # noqa: F401
                       broadcast_parameters, detach_data_parallel, find_base, mark_rank_streams_set, shard_sizes)
from .graph_step import LOG_RING, LOG_ROWS, SPARSE_CAP_MIN, GraphedStep, gt_form, sparse_capacity, step_signature  # noqa: F401
from .optim import FusedClipAdamW, FusedClipBase, FusedClipSGD, HyperTable  # noqa: F401


def encode_sparse_batch(batch, cfg):
    """Collate helper: a batch carrying sparse annotations (``gt_boxes`` / ``gt_class_ids``: per-image lists, network-input
    coordinates) instead of the dense ``gt`` gets the dense tensor built ON THE GPU (``annotations.encode_annotations``;
    the reference does it per image in DataLoader workers, src/datasets/base.py:61-76).  With ``cfg.sparse_gt`` the batch gets
    ``'gt_sparse'`` (an ``ops.SparseGT``: the positives as a list, read by the sparse loss launches) instead and no dense tensor is
    built.  Dense batches pass through, whatever the flag.  ``cfg.ignore_overlap`` (needs ``cfg.sparse_gt``): ``batch['gt_ignore_boxes']``,
    a per-image list of ignore boxes (xyxy, network-input coordinates; absent: none), becomes ``'gt_ignore'``, the anchor ignore
    bitmap the masked loss reads; with the field unset the ignore boxes are dropped.  ``cfg.match_iou`` (needs ``cfg.sparse_gt``;
    ``config.check_match``): the IoU-threshold matcher adds its extra positives to ``'gt_sparse'``, its band and overflow to ``'gt_ignore'``
    (on top of the regions' bits, if any), and the batch gets ``'gt_match_overflow'``, int32 [B] on the device."""
    from .annotations import encode_annotations, ignore_overlap_of
    from .config import check_match
    overlap = ignore_overlap_of(cfg, 'encode_sparse_batch')
    match = check_match(cfg, 'encode_sparse_batch')
    if 'gt' in batch or 'gt_sparse' in batch or 'gt_boxes' not in batch:
        return batch
    out = {k: v for k, v in batch.items() if k not in ('gt_boxes', 'gt_class_ids', 'gt_ignore_boxes')}
    sparse = bool(getattr(cfg, 'sparse_gt', False))
    if match is not None:
        ign = batch.get('gt_ignore_boxes') if overlap is not None else None
        ign = [[] for _ in batch['gt_boxes']] if (ign is None and overlap is not None) else ign
        out['gt_sparse'], out['gt_ignore'], out['gt_match_overflow'] = encode_annotations(
            batch['gt_class_ids'], batch['gt_boxes'], cfg.anchors, cfg.num_classes, device=cfg.device, dense=False, ignore_boxes_list=ign,
            ignore_overlap=overlap, match=match, return_overflow=True)
        return out
    if overlap is not None:
        ign = batch.get('gt_ignore_boxes')
        ign = [[] for _ in batch['gt_boxes']] if ign is None else ign
        out['gt_sparse'], out['gt_ignore'] = encode_annotations(batch['gt_class_ids'], batch['gt_boxes'], cfg.anchors, cfg.num_classes,
                                                                device=cfg.device, dense=False, ignore_boxes_list=ign,
                                                                ignore_overlap=overlap)
        return out
    out['gt_sparse' if sparse else 'gt'] = encode_annotations(batch['gt_class_ids'], batch['gt_boxes'], cfg.anchors, cfg.num_classes,
                                                               device=cfg.device, dense=not sparse)
    return out


class _Mean:
    """Weighted running mean of a logged quantity."""
    __slots__ = ('last', 'total', 'weight')

    def __init__(self):
        self.last, self.total, self.weight = 0.0, 0.0, 0.0

    def add(self, value, weight=1.0):
        self.last = value
        self.total += value * weight
        self.weight += weight

    @property
    def mean(self):
        return self.total / self.weight if self.weight else 0.0


LOSS_KEYS = ('loss', 'class_loss', 'score_loss', 'bbox_loss')


class Trainer(object):
    """Same constructor, ``train_epoch`` / ``val_epoch`` / ``run_epoch`` / ``set_device`` surface and return values as the
    reference's ``Trainer`` (src/engine/trainer.py:9-92).  Differences underneath: process-per-GPU gradient exchange
    (``attach_data_parallel``) instead of the DataParallel wrapper, sparse annotations are encoded on the GPU, and the
    four logged losses cost ONE host sync per iteration (one stacked copy) instead of four ``.item()`` calls."""

    def __init__(self, model, optimizer, lr_scheduler, cfg):
        self.model, self.optimizer, self.lr_scheduler, self.cfg = model, optimizer, lr_scheduler, cfg
        self.metrics = list(LOSS_KEYS)
        self.set_device(cfg.gpus, cfg.chunk_sizes, cfg.device)
        if getattr(cfg, 'graph_step', False):
            self.graphed_step()                    # (what the captured step refuses -- optimizer, process group, model -- is refused here)

    def set_device(self, gpus, chunk_sizes, device):
        """``gpus`` / ``chunk_sizes`` describe the global job as in the reference; this process only owns ``device``.
        Multi-GPU = a process group initialised by the launcher (torchrun)."""
        d = _dist()
        self.world = d.get_world_size() if d is not None else 1
        self.rank = d.get_rank() if d is not None else 0
        self.model = self.model.to(device)
        for st in self.optimizer.state.values():
            for name, v in list(st.items()):
                if isinstance(v, torch.Tensor):
                    st[name] = v.to(device=device, non_blocking=True)
        self.exchange = attach_data_parallel(self.model, self.optimizer)

    def _to_device(self, batch):
        batch = encode_sparse_batch(batch, self.cfg)

        def move(k, v):
            if 'image_meta' in k:
                return v
            if isinstance(v, torch.Tensor):
                return v.to(device=self.cfg.device, non_blocking=True)
            if isinstance(v, tuple) and hasattr(v, '_fields') and all(isinstance(t, torch.Tensor) for t in v):
                return type(v)(*(t.to(device=self.cfg.device, non_blocking=True) for t in v))       # a NamedTuple of tensors (ops.SparseGT)
            return v
        return {k: move(k, v) for k, v in batch.items()}

    def _iteration(self, batch, train):
        fused = train and hasattr(self.model, 'forward_mean')
        if fused:
            # loss.mean() and its backward inside the loss kernels (no torch reduction / elementwise launches in the step)
            mean_loss, parts = self.model.forward_mean(batch)
            per_image_loss = parts['loss']
        else:
            per_image_loss, parts = self.model(batch)
        if train:
            self.optimizer.zero_grad()
            if fused:
                if getattr(self, '_one', None) is None or self._one.device != mean_loss.device:
                    self._one = torch.ones((), device=mean_loss.device)
                mean_loss.backward(self._one)      # local shard mean; the gradient exchange turns it into the global mean
            else:
                per_image_loss.mean().backward()
            if not (isinstance(self.optimizer, FusedClipBase) and self.optimizer.max_norm > 0):     # (it clips inside its one launch)
                torch.nn.utils.clip_grad_norm_([p for p in self.model.parameters() if p.requires_grad], self.cfg.grad_norm)
            self.optimizer.step()
        n = per_image_loss.shape[0]
        logged = torch.stack([parts[k].detach().sum() for k in self.metrics] + [per_image_loss.new_tensor(float(n))])
        if self.world > 1:
            _dist().all_reduce(logged)             # 5 floats: global sums and the global image count
        logged = logged.tolist()                   # the iteration's single host sync
        return [v / logged[-1] for v in logged[:-1]], n

    def graphed_step(self):
        """The ``GraphedStep`` of ``cfg.graph_step`` (made on first use; its refusals surface here)."""
        gs = getattr(self, '_graphed', None)
        if gs is None or gs.model is not self.model or gs.optimizer is not self.optimizer:
            if isinstance(self.optimizer, FusedClipBase) and not self.optimizer.max_norm > 0:
                raise ValueError(f'Trainer: cfg.graph_step clips inside the optimizer launch: construct the {type(self.optimizer).__name__} with '
                                 'max_norm=cfg.grad_norm (with max_norm=0 the eager loop clips with a torch call the captured step lacks)')
            gs = self._graphed = GraphedStep(self.model, self.optimizer, self.cfg)
        return gs

    def _run_epoch_graphed(self, epoch, data_loader):
        """The train phase with ``cfg.graph_step``: every iteration is one ``GraphedStep.step`` and no host sync; the losses come from
        the device log, read at every ``print_interval`` and at the epoch's end.  The printed line has the eager loop's format with the
        latest iteration's losses; ``data`` / ``net`` are averages over the iterations since the last print (a per-iteration host clock
        without a sync would time the enqueue only)."""
        t_epoch = time.time()
        gs = self.graphed_step()
        self.model.train(True)
        gs.reset_log()
        limit = len(data_loader) if self.cfg.num_iters < 0 else self.cfg.num_iters
        t_mark = t_int = time.time()
        t_data, n_int = 0.0, 0
        for it, batch in enumerate(data_loader):
            if it >= limit:
                break
            batch = self._to_device(batch)
            t_data += time.time() - t_mark
            gs.step(batch)
            n_int += 1
            if self.rank == 0 and it % self.cfg.print_interval == 0:
                _, latest, _ = gs.read_log()                 # the interval's one host sync
                t_all = time.time() - t_int
                losses = ' '.join(f'| {k} {latest[k]:.3f}' for k in self.metrics)
                print(f'epoch {epoch}: train [{it}/{limit}] {losses} | data {1e3 * t_data / n_int:.1f}ms | net {1e3 * (t_all - t_data) / n_int:.1f}ms')
                t_int, t_data, n_int = time.time(), 0.0, 0
            t_mark = time.time()
        self.lr_scheduler.step()
        sums, _, _ = gs.read_log()
        out = {k: (sums[k] / sums['images'] if sums['images'] else 0.0) for k in self.metrics}
        out['epoch_time'] = (time.time() - t_epoch) / 60.0
        return out

    def run_epoch(self, phase, epoch, data_loader):
        if phase == 'train' and getattr(self.cfg, 'graph_step', False):
            return self._run_epoch_graphed(epoch, data_loader)
        t_epoch = time.time()
        train = phase == 'train'
        self.model.train(train)
        means = {k: _Mean() for k in self.metrics}
        limit = len(data_loader) if self.cfg.num_iters < 0 else self.cfg.num_iters
        t_mark = time.time()
        for it, batch in enumerate(data_loader):
            if it >= limit:
                break
            batch = self._to_device(batch)
            t_data = time.time() - t_mark
            values, n = self._iteration(batch, train)
            for k, v in zip(self.metrics, values):
                means[k].add(v, n)
            t_net = time.time() - t_mark - t_data
            if self.rank == 0 and it % self.cfg.print_interval == 0:
                losses = ' '.join(f'| {k} {v:.3f}' for k, v in zip(self.metrics, values))
                print(f'epoch {epoch}: {phase:<5s} [{it}/{limit}] {losses} | data {1e3 * t_data:.1f}ms | net {1e3 * t_net:.1f}ms')
            t_mark = time.time()
        if train:
            self.lr_scheduler.step()
        out = {k: m.mean for k, m in means.items()}
        out['epoch_time'] = (time.time() - t_epoch) / 60.0
        return out

    def train_epoch(self, epoch, data_loader):
        return self.run_epoch('train', epoch, data_loader)

    @torch.no_grad()
    def val_epoch(self, epoch, data_loader):
        """With ``cfg.ema_eval`` the epoch runs on the optimizer's averaged weights (``averaged_weights()``: swapped in, swapped back)."""
        if getattr(self.cfg, 'ema_eval', False):
            if not (isinstance(self.optimizer, FusedClipBase) and self.optimizer.ema_on):
                raise ValueError('Trainer: cfg.ema_eval needs a FusedClipSGD or FusedClipAdamW constructed with ema_decay > 0, got '
                                 f'{type(self.optimizer).__name__}')
            with self.optimizer.averaged_weights():
                return self.run_epoch('val', epoch, data_loader)
        return self.run_epoch('val', epoch, data_loader)

def make_train_step(cfg, state_dict, image, rank, world, dist, gt_seed=1, force_exchange=False, fused_optimizer=True, parts=None):
    """Benchmark helper: returns (step_fn, description, probe_fn).  A step = fwd + loss + bwd (with the bucketed RCCL
    gradient exchange when a process group exists) + clip_grad_norm_(5.0) + SGD(lr .01, momentum .9, wd 1e-4) on a
    device-resident batch.  ``probe_fn()`` -> (gt on the CPU, eval-mode per-image loss of the current weights on the CPU):
    what bench.py's CPU leg checks against the oracle before the first optimizer step."""
    from . import synthetic
    from .model import SqueezeDetWithLoss
    model = SqueezeDetWithLoss(cfg)
    model.load_state_dict(state_dict)
    model = model.to(image.device).train()
    params = [p for p in model.parameters() if p.requires_grad]
    kind = str(getattr(cfg, 'optimizer', 'sgd')).lower()
    if kind not in ('sgd', 'adamw'):
        raise ValueError(f"make_train_step: cfg.optimizer must be 'sgd' or 'adamw', got {getattr(cfg, 'optimizer')!r}")
    ema = dict(ema_decay=float(getattr(cfg, 'ema_decay', 0.0)), ema_warmup=bool(getattr(cfg, 'ema_warmup', False)))
    if fused_optimizer:
        base = find_base(model)
        if kind == 'adamw':
            opt = FusedClipAdamW(params, lr=cfg.lr, weight_decay=cfg.weight_decay, max_norm=cfg.grad_norm,
                                 flat_grad=lambda: base.last_grad_flat, **ema)
        else:
            opt = FusedClipSGD(params, lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay, max_norm=cfg.grad_norm,
                               flat_grad=lambda: base.last_grad_flat, **ema)
    elif kind == 'adamw':
        opt = torch.optim.AdamW(params, lr=cfg.lr, weight_decay=cfg.weight_decay)
    else:
        opt = torch.optim.SGD(params, lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
    gt_cpu = synthetic.make_gt(image.shape[0], cfg.anchors, cfg.input_size, cfg.num_classes, seed=gt_seed + rank)
    gt = gt_cpu.to(image.device)
    batch = {'image': image, 'gt': gt}
    ex = attach_data_parallel(model, opt) if dist is not None else None
    if ex is not None:
        ex.force = bool(force_exchange)
    if parts is not None:                            # (bench.py diagnostics: the objects behind the closure)
        parts.update(model=model, optimizer=opt, base=find_base(model), exchange=ex)

    one = torch.ones((), device=image.device)       # the root gradient, allocated once (autograd would fill a new tensor every step)

    def step():
        loss, stats = model.forward_mean(batch)     # = model(batch)[0].mean(), the mean and its backward inside the loss kernels
        opt.zero_grad()
        loss.backward(one)
        if not fused_optimizer:
            torch.nn.utils.clip_grad_norm_(params, cfg.grad_norm)
        opt.step()                                   # (fused: clip + SGD in one launch)
        return loss

    def probe():
        model.eval()
        with torch.no_grad():
            lv, _ = model(batch)
        model.train()
        return gt_cpu, lv.detach().cpu()

    net = 'SqueezeDet' if cfg.arch == 'squeezedet' else 'SqueezeDet+'
    oname = 'SGD' if kind == 'sgd' else 'AdamW'
    if fused_optimizer and ema['ema_decay'] > 0:
        oname += ' + EMA'
    desc = f'{net} KITTI 1248x384 bs={image.shape[0]}/GPU training: fwd + multi-task loss + bwd + clip(5.0) + {oname}' + (
        f' (clip + {oname}: one fused launch)' if fused_optimizer else '')
    if ex is not None:
        desc += f' + RCCL gradient all-reduce over {world} GPU(s) in 3 buckets overlapped with backward'
    return step, desc, probe
