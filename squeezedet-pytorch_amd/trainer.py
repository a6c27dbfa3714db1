"""Training-side plumbing of the hot path: the data-parallel gradient exchange and a ``Trainer`` with the
reference's interface.

What the reference does (src/engine/trainer.py:18-92, src/utils/data_parallel.py:46-156): ONE Python process
replicates the module onto every GPU each step, scatters the batch by ``chunk_sizes``, gathers the per-sample loss
vectors on GPU 0 and back-propagates ``loss.mean()`` of that gathered vector through the replicas.

What runs here: one process per GPU (``torch.distributed`` over RCCL / xGMI), weights replicated once, and the
gradient of that same GLOBAL mean assembled by an all-reduce that the backward itself drives:

* ``attach_data_parallel(model)`` hangs a ``GradientExchange`` on the model's ``SqueezeDetBase``.  From then on
  ``loss.backward()`` leaves the global-mean gradient in every ``p.grad`` -- the reference's own
  ``src/engine/trainer.py`` loop (``zero_grad -> backward -> clip_grad_norm_ -> step``) runs unchanged on top of it.
* The backward (``backward.py``) reports each finished slice of its flat gradient buffer -- ConvDet + the 24x78 Fire
  modules first (86 % of the parameters), then the 48x156 and the 96x312 stages -- and the exchange all-reduces that
  bucket on a side stream while the remaining layers are still being differentiated.
* Shards may be unequal: every rank scales its bucket by its local image count, one extra float at the end of the
  buffer carries that count through the same all-reduce, and the sum is divided by the global count on the device --
  exactly ``mean`` over the gathered vector (trainer.py:43) for any ``chunk_sizes``, with no extra collective and no
  host sync.  ``clip_grad_norm_`` then sees the same global norm on every rank, SGD is local and deterministic.
"""
from __future__ import annotations

import time

import torch


def _dist(group=None):
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


def shard_sizes(batch_size, world):
    """Images per rank for a global batch (first ranks take the remainder): the even-split case of the
    reference's ``chunk_sizes`` (src/utils/config.py:102-110)."""
    q, r = divmod(int(batch_size), int(world))
    return [q + (i < r) for i in range(world)]


class GradientExchange:
    """All-reduce of the flat gradient buffer in buckets, overlapped with the backward that fills it.

    Driven by ``backward.run_backbone_backward``: ``begin(flat, total, local_batch)`` once the buffer exists (``flat``
    holds ``total`` gradient floats plus one trailing count slot), ``ready(lo, hi)`` whenever the slice ``[lo, hi)`` is
    final on the current stream, ``finish()`` before the gradients are handed to autograd.  Works on any backend;
    the side stream is only used for CUDA/HIP buffers."""

    def __init__(self, group=None, overlap=True):
        self.group = group
        self.overlap = overlap
        self.force = False                     # run the collectives even in a one-rank group (bench.py --force-dist)
        self._side = None
        self._flat = None
        self._pending = []
        self._captured_works = []
        self.buckets_last_step = []            # [(lo, hi)] of the latest backward, for tests / logging

    def world(self):
        d = _dist()
        return d.get_world_size(self.group) if d is not None else 1

    def begin(self, flat, total, local_batch):
        self._flat, self._total, self._b = flat, int(total), float(local_batch)
        self._pending = []
        self.buckets_last_step = []
        self._active = self.world() > 1 or (self.force and _dist() is not None)
        # weight of this rank's gradient in the global mean: the backward multiplies it in where the gradients are produced (the slab
        # reduction's ``scale``, ``scale_slice`` for the stem) -- no element-wise pass over the buckets
        self.scale = self._b if self._active else 1.0
        self._native = bool(self._active and flat.is_cuda)
        if self._active:
            if self._native:
                from . import _native as nat
                # the count slot, through the library (one thread): no torch kernel in the exchange
                nat.check(nat.lib().sqd_grad_scale(None, 0, 1.0, None, nat.c_p(flat.data_ptr() + 4 * self._total), self._b,
                                                   nat.stream_handle(flat.device)), 'sqd_grad_scale')
            else:
                flat[total:].fill_(self._b)
            if flat.is_cuda and self.overlap and self._side is None:
                self._side = torch.cuda.Stream(device=flat.device)

    def scale_slice(self, lo, hi):
        """Weight ``flat[lo:hi]`` (a gradient that did not come out of the slab reduction: the stem's) by this rank's image count."""
        if not self._active or hi <= lo:
            return
        if self._native:
            from . import _native as nat
            nat.check(nat.lib().sqd_grad_scale(nat.c_p(self._flat.data_ptr() + 4 * int(lo)), int(hi - lo), self.scale, None, None, 0.0,
                                               nat.stream_handle(self._flat.device)), 'sqd_grad_scale')
        else:
            self._flat[lo:hi].mul_(self.scale)

    def _divide(self, lo, grad_hi):
        """flat[lo:grad_hi] /= the summed image count (device scalar in the count slot), on the current stream."""
        from . import _native as nat
        nat.check(nat.lib().sqd_grad_scale(nat.c_p(self._flat.data_ptr() + 4 * int(lo)), int(grad_hi - lo), 1.0,
                                           nat.c_p(self._flat.data_ptr() + 4 * self._total), None, 0.0,
                                           nat.stream_handle(self._flat.device)), 'sqd_grad_scale')

    def ready(self, lo, hi):
        """``flat[lo:hi]`` is final on the current stream AND already weighted by ``scale``: all-reduce it (SUM) -- on the side stream when
        overlapping.  ``finish`` divides by the summed image count (the count slot travels with the first bucket handed over, the tail
        of the buffer)."""
        if not self._active or hi <= lo:
            return
        d = _dist()
        if hi == self._total:
            hi = self._flat.numel()             # the count slot travels with the tail bucket
        elif not self.buckets_last_step and self._native:
            raise RuntimeError('GradientExchange.ready: the first bucket must be the tail of the buffer (it carries the count slot)')
        self.buckets_last_step.append((int(lo), int(hi)))
        grad_hi = min(hi, self._total)
        if self._side is not None:
            ev = torch.cuda.Event()
            ev.record()
            with torch.cuda.stream(self._side):
                self._side.wait_event(ev)
                work = d.all_reduce(self._flat[lo:hi], op=d.ReduceOp.SUM, group=self.group, async_op=True)
        else:
            work = d.all_reduce(self._flat[lo:hi], op=d.ReduceOp.SUM, group=self.group, async_op=True)
        self._pending.append((work, lo, grad_hi))
        if self._flat.is_cuda and torch.cuda.is_current_stream_capturing():
            # a collective issued while a hipGraph is being captured: its Work object (and the events inside, recorded in the capturing
            # stream) is kept alive for the life of the exchange.  Released, those events go back to the process group's event cache and
            # the next EAGER collective (a barrier right behind the capture) reuses one; the group's watchdog thread has been seen to
            # query such an event while it still counted as "recorded in a capturing stream" and to abort the process (about one run
            # in ten of `bench.py --force-dist`).  A handful of objects per captured step.
            self._captured_works.append(work)

    def finish(self):
        if not self._active:
            return
        for w, _lo, _hi in self._pending:
            w.wait()                            # CUDA: the current stream waits for the collective; CPU: blocks
        if self._side is not None:
            torch.cuda.current_stream().wait_stream(self._side)
        if self._native:
            # ONE launch over the whole buffer, behind the last collective (the summed count is in the slot by then).  (Dividing every
            # bucket on the side stream right behind its own collective -- side waits on the collective's stream, the next collective
            # waits on side again -- captured into a graph that crashed hipStreamEndCapture on ROCm 7.2; 8 MB take ~5 us here.)
            self._divide(0, self._total)
        else:
            flat, total = self._flat, self._total
            flat[:total].div_(flat[total])      # global image count, summed by the same all-reduce
        self._pending = []
        self._flat = None


def broadcast_parameters(module, src=0, group=None):
    """Identical weights on every rank, ONE broadcast of a flat copy (not one per tensor); written back with
    ``copy_`` so version counters move and the packed-weight caches of the HIP plan refresh."""
    d = _dist()
    if d is None or d.get_world_size(group) == 1:
        return
    params = [p for p in module.parameters()]
    with torch.no_grad():
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        d.broadcast(flat, src=src, group=group)
        off = 0
        for p in params:
            n = p.numel()
            p.copy_(flat[off:off + n].view_as(p))
            off += n


def find_base(model):
    """The ``SqueezeDetBase`` inside ``model`` (``SqueezeDetWithLoss`` / ``SqueezeDet`` / the base itself / a ``.module``
    wrapper)."""
    from .model import SqueezeDetBase
    for m in model.modules():
        if isinstance(m, SqueezeDetBase):
            return m
    raise TypeError('no SqueezeDetBase inside the model')


# this process's random streams already differ from the other ranks' (seeded here or restored), and the seed they had then: a later
# torch.manual_seed() by the user makes all ranks equal again, which the next attach notices by the changed initial seed
_RANK_STREAMS = {'set': False, 'seed': None}


def mark_rank_streams_set(flag=True):
    """Tell ``attach_data_parallel`` that this process's random streams are already rank-specific (``checkpoint.load_checkpoint``
    calls this after restoring the rank's own streams, so a later ``Trainer(...)`` / ``attach_data_parallel`` leaves them alone);
    ``False``: they are NOT (a checkpoint with fewer streams than ranks was loaded) and the next attach offsets them again."""
    _RANK_STREAMS['set'] = bool(flag)
    _RANK_STREAMS['seed'] = torch.initial_seed() if flag else None


def attach_data_parallel(model, optimizer=None, group=None, overlap=True, broadcast=True, seed_offset=True):
    """Process-per-GPU replacement of the reference's ``DataParallel`` wrapper (src/engine/trainer.py:83-85): after this
    call ``loss.mean().backward()`` on the local shard leaves the gradient of the GLOBAL batch mean in ``p.grad`` on every
    rank.  Also replicates rank 0's weights (and optimizer state tensors) once and de-correlates the dropout streams of
    the ranks -- ONCE per process: a second call (the INTEGRATION.md recipe followed by ``Trainer``), or a call after
    ``load_checkpoint`` has restored this rank's own streams (the reference's resume order: load, then ``Trainer(...)``), does
    not touch the generators again.  No-op without an initialised process group.  Returns the ``GradientExchange`` (or None)."""
    d = _dist()
    base = find_base(model)
    if d is None:
        base.grad_sync = None
        return None
    ex = GradientExchange(group=group, overlap=overlap)
    base.grad_sync = ex
    if broadcast:
        broadcast_parameters(model, 0, group)
        if optimizer is not None:
            tensors = [v for st in optimizer.state.values() for v in st.values() if isinstance(v, torch.Tensor) and v.is_floating_point()]
            if tensors:
                with torch.no_grad():
                    flat = torch.cat([t.reshape(-1) for t in tensors])
                    d.broadcast(flat, src=0, group=group)
                    off = 0
                    for t in tensors:
                        t.copy_(flat[off:off + t.numel()].view_as(t)); off += t.numel()
    if seed_offset and (not _RANK_STREAMS['set'] or _RANK_STREAMS['seed'] != torch.initial_seed()):
        rank = d.get_rank(group)
        if rank:
            torch.manual_seed(torch.initial_seed() + rank)     # seeds the CPU and every GPU generator of this process
        _RANK_STREAMS['set'] = True
        _RANK_STREAMS['seed'] = torch.initial_seed()           # (the dropout in front of ConvDet derives its stream from this seed)
    return ex


def detach_data_parallel(model):
    find_base(model).grad_sync = None


def allreduce_gradients(params, world=None, group=None, local_batch=None):
    """Stand-alone form for gradients that did NOT come out of the HIP backward (tests with oracle gradients, foreign
    modules): averages ``p.grad`` over the ranks as one flat bucket -- weighted by ``local_batch`` when given (exact
    global mean for unequal shards), else a plain mean over ranks.  Consecutive views of one buffer (what the HIP
    backward emits) are reduced in place.  Returns the flat bucket."""
    d = _dist()
    params = [p for p in params if p.grad is not None]
    if not params:
        return None
    if world is None:
        world = d.get_world_size(group) if d is not None else 1
    g0 = params[0].grad
    off, in_place = 0, g0.is_contiguous()
    for p in params:
        g = p.grad
        if not (in_place and g.is_contiguous() and g.dtype == g0.dtype and g.device == g0.device
                and g.untyped_storage().data_ptr() == g0.untyped_storage().data_ptr()
                and g.storage_offset() == g0.storage_offset() + off):
            in_place = False
            break
        off += g.numel()
    if in_place:
        flat = g0.as_strided((off,), (1,), g0.storage_offset())
    else:
        flat = torch.cat([p.grad.reshape(-1) for p in params])
    if d is not None and world > 1:
        if local_batch is None:
            d.all_reduce(flat, op=d.ReduceOp.SUM, group=group)
            flat.mul_(1.0 / world)
        else:
            cnt = torch.full((1,), float(local_batch), dtype=flat.dtype, device=flat.device)
            flat.mul_(float(local_batch))
            d.all_reduce(flat, op=d.ReduceOp.SUM, group=group)
            d.all_reduce(cnt, op=d.ReduceOp.SUM, group=group)
            flat.div_(cnt)
    if not in_place:
        off = 0
        for p in params:
            n = p.numel()
            p.grad.copy_(flat[off:off + n].view_as(p))
            off += n
    return flat


def encode_sparse_batch(batch, cfg):
    """Collate helper: a batch carrying sparse annotations (``gt_boxes`` / ``gt_class_ids``: per-image lists, network-input
    coordinates) instead of the dense ``gt`` gets the dense tensor built ON THE GPU (``annotations.encode_annotations``;
    the reference does it per image in DataLoader workers, src/datasets/base.py:61-76).  With ``cfg.sparse_gt`` the batch gets
    ``'gt_sparse'`` (an ``ops.SparseGT``: the positives as a list, read by the sparse loss launches) instead and no dense tensor is
    built.  Dense batches pass through, whatever the flag.  ``cfg.ignore_overlap`` (needs ``cfg.sparse_gt``): ``batch['gt_ignore_boxes']``,
    a per-image list of ignore boxes (xyxy, network-input coordinates; absent: none), becomes ``'gt_ignore'``, the anchor ignore
    bitmap the masked loss reads; with the field unset the ignore boxes are dropped."""
    from .annotations import encode_annotations, ignore_overlap_of
    overlap = ignore_overlap_of(cfg, 'encode_sparse_batch')
    if 'gt' in batch or 'gt_sparse' in batch or 'gt_boxes' not in batch:
        return batch
    out = {k: v for k, v in batch.items() if k not in ('gt_boxes', 'gt_class_ids', 'gt_ignore_boxes')}
    sparse = bool(getattr(cfg, 'sparse_gt', False))
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


class HyperTable:
    """When the device copy of a few hyper-parameters is written: ``refresh(values)`` calls ``write(values)`` if they differ from what
    was written last (or ``force``), never otherwise; while a stream capture is under way it writes nothing and raises if it would
    have to -- the write would be recorded into the graph with the values of the capture."""

    def __init__(self, write):
        self.write = write
        self.written = None

    def refresh(self, values, capturing=False, force=False):
        values = tuple(float(v) for v in values)
        if values == self.written and not force:
            return False
        if capturing:
            raise RuntimeError(f'the device hyper-parameter table is stale under stream capture (holds {self.written}, wanted {values}): '
                               'call refresh_hyper() before the capture begins')
        self.write(values)
        self.written = values
        return True


class FusedClipBase(torch.optim.Optimizer):
    """What the one-launch optimizers (``FusedClipSGD``, ``FusedClipAdamW``) share: ONE parameter group whose ``param_groups[0]`` is read
    at every ``step()``; the detection of the backward's flat gradient buffer; the descriptor and chunk tables with their rebuild rule;
    the device hyper-parameter table (``HyperTable``); ``norm_value``; and the exponential moving average of the weights.

    The EMA (``ema_decay > 0``, fixed at construction) follows ``torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d))``:
    the first averaged step copies the new parameters, later ones ``e += (1 - d_t) (p - e)`` with ``d_t = d``, or with ``ema_warmup``
    ``min(d, (1 + n) / (10 + n))`` after ``n`` averaged steps.  It is computed inside the step launch (one more read and write while
    the fresh parameter is in a register), lives in ``ema_flat`` (views in ``state[p]['ema']``) and is part of ``state_dict()``.  The
    counts -- ``t`` optimizer steps (AdamW's bias correction) and ``n`` averaged steps -- live on the DEVICE and are advanced by a
    one-thread launch in front of every step (``sqd_optim_begin``), eager and captured alike: a replayed hipGraph needs no host write.
    ``averaged_weights()`` swaps the averaged values into the parameters for an evaluation, ``ema_state_dict(model)`` returns them."""

    def __init__(self, params, defaults, flat_grad=None):
        who = type(self).__name__
        params = [p for p in params if p.requires_grad]
        if not params or any(p.dtype != torch.float32 or not p.is_cuda for p in params):
            raise ValueError(f'{who}: fp32 parameters on the GPU only (the product path has no CPU fallback)')
        if not 0.0 <= float(defaults['ema_decay']) < 1.0:
            raise ValueError(f'{who}: ema_decay must be in [0, 1) (0 = no EMA), got {defaults["ema_decay"]!r}')
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f'{who}: one parameter group (the kernel applies one set of hyper-parameters to all tensors)')
        self.flat_grad = flat_grad                     # callable -> the flat gradient tensor the .grad views live in (or None)
        self.total = sum(p.numel() for p in self.params)
        self._table = self._table_key = self._chunks = None
        self._norm_ws = None                           # partial sums of squares + the norm (device)
        self.last_norm = None
        self._hyper_dev = None                         # the device hyper-parameter table
        self._hyper_table = HyperTable(self._write_hyper)
        self.ema_on = float(defaults['ema_decay']) > 0     # structural: the EMA launches and buffers exist or not
        self.ema_flat = self._emas = None
        self._steps_dev = None                         # int32 {t, n} | float32 derived {lr / bc1, 1 / sqrt(bc2), 1 - d_t, copy} (device)
        self._swap_tables = self._swap_key = None
        self._averaging = False
        if self.ema_on:
            self.ema_flat, self._emas = self._flat_state('ema')
            with torch.no_grad():                      # (meaningful before the first step; the first averaged step copies anyway)
                for e, p in zip(self._emas, self.params):
                    e.copy_(p.detach().reshape(-1))

    @property
    def params(self):
        return self.param_groups[0]['params']

    def _hyper(self, name):
        return float(self.param_groups[0][name])

    lr = property(lambda self: self._hyper('lr'))
    weight_decay = property(lambda self: self._hyper('weight_decay'))
    max_norm = property(lambda self: self._hyper('max_norm'))
    ema_decay = property(lambda self: self._hyper('ema_decay'))
    ema_warmup = property(lambda self: bool(self.param_groups[0]['ema_warmup']))

    def add_param_group(self, param_group):
        if getattr(self, 'param_groups', None):
            raise ValueError(f'{type(self).__name__}: one parameter group only')
        super().add_param_group(param_group)

    def _flat_state(self, name):
        """A zero flat buffer of the parameters' total size and its per-parameter views, registered as ``state[p][name]`` (views:
        ``attach_data_parallel`` broadcasts floating-point optimizer state tensors in place)."""
        flat = torch.zeros(self.total, device=self.params[0].device, dtype=torch.float32)
        views, off = [], 0
        for p in self.params:
            views.append(flat[off:off + p.numel()]); off += p.numel()
            self.state[p][name] = views[-1]
        return flat, views

    def _write_hyper(self, values):
        from . import _native as nat
        dev = self.params[0].device
        if self._hyper_dev is None or self._hyper_dev.device != dev or self._hyper_dev.numel() != len(values):
            self._hyper_dev = torch.zeros(len(values), device=dev, dtype=torch.float32)
        for i in range(0, len(values), 4):             # (one one-thread launch per four values: the SGD table without EMA is one launch)
            nat.check(nat.lib().sqd_fill_f32x4(nat.c_p(self._hyper_dev.data_ptr() + 4 * i), *[float(v) for v in values[i:i + 4]],
                                               nat.stream_handle(dev)), 'sqd_fill_f32x4')

    def refresh_hyper(self):
        """Bring the device hyper-parameter table up to date with ``param_groups[0]`` on the current stream (one-thread launches, only
        when a value changed since the last write): what a caller does in front of a replay of a captured step.  -> whether it wrote.
        Raises under stream capture if the table is stale (the write would become part of the graph with today's values)."""
        dev = self.params[0].device
        return self._hyper_table.refresh(self._hyper_values(), capturing=torch.cuda.is_current_stream_capturing(),
                                         force=self._hyper_dev is None or self._hyper_dev.device != dev)

    def _flat_base(self, grads):
        """The flat gradient tensor if the gradients are consecutive views of it (the HIP backward's layout), else None."""
        flat = self.flat_grad() if self.flat_grad is not None else None
        if flat is None or not flat.is_contiguous() or flat.numel() < self.total:
            return None
        ptr = flat.data_ptr()
        for g in grads:
            if not g.is_contiguous() or g.data_ptr() != ptr:
                return None
            ptr += g.numel() * 4
        return flat

    def _gradients(self):
        """-> (the flat gradient buffer or None, the gradients: contiguous when they are separate tensors)."""
        grads = [p.grad for p in self.params]
        if any(g is None for g in grads):
            raise RuntimeError(f'{type(self).__name__}.step: a parameter has no gradient')
        flat = self._flat_base(grads)
        if flat is None:
            grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
        return flat, grads

    def _ensure_tables(self, flat, grads, firsts, seconds=None):
        """The descriptor table holds the parameter and state addresses and, per tensor, its offset into the flat gradient buffer (whose
        own address is a launch argument) or the gradient's address: rows of 4 words {p, grad, first state, elements}, or of 6 with
        ``seconds`` or the EMA {.., second state, ema}.  Everything baked into it is part of the key: a parameter whose storage was
        replaced after the first step (model.to() / p.data = ...) rebuilds the table instead of letting the kernel write through a
        stale pointer."""
        from . import _native as nat
        params = self.params
        wide = seconds is not None or self.ema_on
        key = (('flat',) if flat is not None else tuple(g.data_ptr() for g in grads), tuple(p.data_ptr() for p in params),
               firsts[0].data_ptr()) + ((seconds[0].data_ptr() if seconds is not None else 0,
                                         self.ema_flat.data_ptr() if self.ema_on else 0) if wide else ())
        if key == self._table_key:
            return
        off, rows = 0, []
        for i, (p, g, b) in enumerate(zip(params, grads, firsts)):
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise RuntimeError(f'{type(self).__name__}.step: parameters must stay contiguous fp32 GPU tensors')
            row = [p.data_ptr(), off if flat is not None else g.data_ptr(), b.data_ptr(), p.numel()]
            if wide:
                row += [seconds[i].data_ptr() if seconds is not None else 0, self._emas[i].data_ptr() if self.ema_on else 0]
            rows.append(row); off += p.numel()
        self._table = torch.tensor(rows, dtype=torch.int64).to(params[0].device)
        # equal chunks of the 64 tensors (16 .. 500 k elements): one workgroup per chunk
        ce = int(nat.lib().sqd_sgd_chunk_elems())
        chunks = [[i, e] for i, p in enumerate(params) for e in range(0, p.numel(), ce)]
        self._chunks = torch.tensor(chunks, dtype=torch.int64).to(params[0].device)
        self._table_key = key

    def _sumsq(self, flat):
        """The norm of the flat gradient buffer: partial sums of squares by one small launch, finished (fixed order) inside the step.
        -> (parts, the 0-dim norm the step launch writes)."""
        from . import _native as nat
        if self._norm_ws is None:
            self._norm_ws = torch.empty(int(nat.lib().sqd_grad_sumsq_parts()) + 1, device=flat.device, dtype=torch.float32)
        parts, norm = self._norm_ws[:-1], self._norm_ws[-1]
        nat.check(nat.lib().sqd_grad_sumsq(nat.ptr(flat), self.total, nat.ptr(parts), nat.stream_handle(flat.device)), 'sqd_grad_sumsq')
        return parts, norm

    def _begin(self, adam):
        """The one-thread launch in front of a step: advances the device counts, writes the derived table -> (counters, derived)."""
        from . import _native as nat
        dev = self.params[0].device
        if self._steps_dev is None or self._steps_dev.device != dev:
            was = self._steps_dev
            self._steps_dev = torch.zeros(8, device=dev, dtype=torch.int32)
            if was is not None:
                self._steps_dev.copy_(was)
        counters, derived = self._steps_dev[:2], self._steps_dev[2:6].view(torch.float32)
        nat.check(nat.lib().sqd_optim_begin(nat.ptr(self._hyper_dev), nat.ptr(counters), nat.ptr(derived), int(adam), int(self.ema_on),
                                            nat.stream_handle(dev)), 'sqd_optim_begin')
        return counters, derived

    def step_counts(self):
        """(t, n): optimizer steps counted for the bias correction (0 for SGD) and averaged steps, read from the device (one host sync)."""
        if self._steps_dev is None:
            return 0, 0
        t, n = self._steps_dev[:2].tolist()
        return int(t), int(n)

    def _set_step_counts(self, t, n):
        dev = self.params[0].device
        if self._steps_dev is None or self._steps_dev.device != dev:
            self._steps_dev = torch.zeros(8, device=dev, dtype=torch.int32)
        self._steps_dev[:2].copy_(torch.tensor([int(t), int(n)], dtype=torch.int32))

    def norm_value(self):
        """The latest step's total gradient norm as a Python float (one host sync), or None before the first clipped step."""
        return None if self.last_norm is None else float(self.last_norm)

    # ---- the averaged weights ----
    def _swap(self):
        from . import _native as nat
        params = self.params
        key = (tuple(p.data_ptr() for p in params), self.ema_flat.data_ptr())
        if key != self._swap_key:
            if any(not p.is_contiguous() for p in params):
                raise RuntimeError(f'{type(self).__name__}.averaged_weights: parameters must stay contiguous fp32 GPU tensors')
            rows = [[p.data_ptr(), 0, 0, p.numel(), 0, e.data_ptr()] for p, e in zip(params, self._emas)]
            ce = int(nat.lib().sqd_sgd_chunk_elems())
            chunks = [[i, e] for i, p in enumerate(params) for e in range(0, p.numel(), ce)]
            dev = params[0].device
            self._swap_tables = (torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(chunks, dtype=torch.int64).to(dev))
            self._swap_key = key
        table, chunks = self._swap_tables
        nat.check(nat.lib().sqd_param_swap(nat.ptr(table), nat.ptr(chunks), chunks.shape[0], nat.stream_handle(params[0].device)),
                  'sqd_param_swap')
        torch.autograd.graph.increment_version(params)        # (the packed-weight caches key on the version counters: PlanCache re-packs)

    def averaged_weights(self):
        """Context manager: inside, the parameters hold the EMA (one swap launch; the version counters advance, so the packed-weight
        caches re-pack without a manual ``invalidate_plans``) -- evaluate or export there; leaving swaps back, and the parameters are
        bit-identical to before.  Raises when the EMA is off, when nested and under stream capture."""
        import contextlib
        who = type(self).__name__

        @contextlib.contextmanager
        def ctx():
            if not self.ema_on:
                raise RuntimeError(f'{who}.averaged_weights: the EMA is off (construct the optimizer with ema_decay > 0)')
            if self._averaging:
                raise RuntimeError(f'{who}.averaged_weights: already inside averaged_weights() (nested: the inner block would swap the '
                                   'training weights back in)')
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'{who}.averaged_weights: not under stream capture (the swap is not part of a training step)')
            self._averaging = True
            self._swap()
            try:
                yield self
            finally:
                self._swap()
                self._averaging = False
        return ctx()

    def ema_state_dict(self, model):
        """``model.state_dict()`` (clones) with every parameter this optimizer averages replaced by its EMA: what ``Detector``,
        ``save_model`` / ``load_model`` and ``load_state_dict`` take unchanged."""
        if not self.ema_on:
            raise RuntimeError(f'{type(self).__name__}.ema_state_dict: the EMA is off (construct the optimizer with ema_decay > 0)')
        if self._averaging:
            raise RuntimeError(f'{type(self).__name__}.ema_state_dict: inside averaged_weights() the parameters ARE the averaged values: '
                               'take model.state_dict()')
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        ema = {id(p): e for p, e in zip(self.params, self._emas)}
        for name, p in model.named_parameters():
            if id(p) in ema:
                if name not in sd:
                    raise RuntimeError(f'ema_state_dict: parameter {name} is not a key of the state_dict')
                sd[name] = ema[id(p)].detach().clone().view(p.shape)
        return sd

    def _check_step_allowed(self):
        if self._averaging:
            raise RuntimeError(f'{type(self).__name__}.step: inside averaged_weights() (the parameters hold the EMA)')

    def _ema_state(self):
        g = self.param_groups[0]
        out = {'ema_decay': g['ema_decay'], 'ema_warmup': bool(g['ema_warmup'])}
        if self.ema_on:
            out['ema_flat'] = self.ema_flat.clone()
        return out

    def _load_ema_state(self, sd):
        g = self.param_groups[0]
        if self.ema_on and sd.get('ema_flat') is not None:
            self.ema_flat.copy_(sd['ema_flat'].to(self.ema_flat.device))
        if self.ema_on and sd.get('ema_decay'):
            g['ema_decay'] = float(sd['ema_decay'])
        if sd.get('ema_warmup') is not None:
            g['ema_warmup'] = bool(sd['ema_warmup'])


class FusedClipSGD(FusedClipBase):
    """``torch.nn.utils.clip_grad_norm_(params, max_norm)`` + ``torch.optim.SGD(params, lr, momentum, weight_decay).step()``
    (src/engine/trainer.py:47-50) as ONE launch over all parameter tensors (csrc/optim.hip, sqd_sgd_clip_step): torch runs the pair
    as ~10 foreach / elementwise launches over the 64 tensors (about 0.15 ms of a 6.3 ms training step).  Same arithmetic in the
    same order per element; the gradient norm is one reduction over the backward's flat gradient buffer when the gradients are
    consecutive views of it (the HIP backward's layout), else torch's foreach norm; it is read on the device (no host sync, hipGraph
    capturable).

    A ``torch.optim.Optimizer`` with ONE parameter group: ``param_groups[0]`` carries ``lr`` / ``momentum`` / ``weight_decay`` /
    ``max_norm`` and is read at every ``step()``, so ``torch.optim.lr_scheduler.StepLR(opt, 60, 0.5)`` (the reference's schedule,
    src/train.py:36, stepped at src/engine/trainer.py:67) drives it like ``torch.optim.SGD``.  ``max_norm > 0`` clips INSIDE
    ``step()``: a caller that keeps the reference's explicit ``clip_grad_norm_`` line must construct it with ``max_norm=0`` (or
    drop the line, as ``Trainer._iteration`` does) -- otherwise the gradient is clipped twice.  By default the hyper-parameters are
    launch arguments: a hipGraph replay of a captured step keeps the values of the capture.  With ``hyper_on_device = True`` they live
    in a device ``float[4]`` table that the kernel reads (``sqd_sgd_clip_step_chunked_dev``; flat-gradient layout only): ``step()``
    rewrites the table -- one one-thread launch, only when a value of ``param_groups[0]`` changed -- and whoever replays a captured step
    calls ``refresh_hyper()`` in front of the replay, so an LR schedule needs no re-capture.  Only whether the norm is evaluated at all
    (``max_norm > 0``) is fixed by the capture: a caller that switches between zero and positive re-captures.

    ``ema_decay > 0`` adds the weight EMA of ``FusedClipBase`` to the launch (``sqd_sgd_clip_step_chunked_ema``: the same arithmetic
    and bits for the parameters and the momentum).  It needs the device hyper-parameter table (``hyper_on_device`` is switched on at
    construction) and the flat-gradient layout; at 0 nothing changes: the launches, the bits and the keys of ``state_dict()``."""

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, max_norm=0.0, flat_grad=None, ema_decay=0.0, ema_warmup=False):
        super().__init__(params, dict(lr=float(lr), momentum=float(momentum), weight_decay=float(weight_decay), max_norm=float(max_norm),
                                      ema_decay=float(ema_decay), ema_warmup=bool(ema_warmup)), flat_grad)
        self.momentum_flat, self._bufs = self._flat_state('momentum_buffer')
        self.hyper_on_device = self.ema_on             # the kernel reads {lr, momentum, weight_decay, max_norm} from device memory

    momentum = property(lambda self: self._hyper('momentum'))

    def _hyper_values(self):
        sgd = (self.lr, self.momentum, self.weight_decay, self.max_norm)
        return sgd + (self.ema_decay, float(self.ema_warmup), 0.0, 0.0) if self.ema_on else sgd

    @torch.no_grad()
    def step(self, closure=None):
        """One clip + SGD step.  Returns the total gradient norm (``clip_grad_norm_``'s return value) as a 0-dim DEVICE tensor that
        ALIASES a persistent workspace (also kept in ``last_norm``): the next ``step`` overwrites it in place -- a copy per step would
        be the one torch kernel of an otherwise torch-free captured training step.  Callers that keep norms across iterations take
        the value at once (``float(norm)`` / ``norm.item()``) or ``norm.clone()`` (``norm_value()`` = the float of the latest step)."""
        from . import _native as nat
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_step_allowed()
        params = self.params
        flat, grads = self._gradients()
        if self.ema_on and not (self.hyper_on_device and flat is not None):
            raise RuntimeError('FusedClipSGD.step: ema_decay > 0 runs in the chunked launch that reads its hyper-parameters from device '
                               'memory, not on the launch-argument path: it needs hyper_on_device = True and the flat-gradient layout '
                               '(flat_grad given and every p.grad a consecutive view of that buffer, as the HIP backward leaves them)')
        if self.hyper_on_device and flat is None:
            raise RuntimeError('FusedClipSGD.step: hyper_on_device needs the flat-gradient layout (flat_grad given and every p.grad a '
                               'consecutive view of that buffer, as the HIP backward leaves them); these gradients are separate tensors')
        self._ensure_tables(flat, grads, self._bufs)
        norm = None
        max_norm = self.max_norm
        if self.hyper_on_device:
            self.refresh_hyper()                       # (writes when a value changed; under capture: raises if it would have to)
            parts = None
            if max_norm > 0:                           # structural: a captured step keeps or lacks the norm launch
                parts, norm = self._sumsq(flat)
            if self.ema_on:
                _, derived = self._begin(adam=False)
                nat.check(nat.lib().sqd_sgd_clip_step_chunked_ema(nat.ptr(self._table), nat.ptr(self._chunks), self._chunks.shape[0],
                                                                  nat.ptr(flat), nat.ptr(parts), nat.ptr(norm), nat.ptr(self._hyper_dev),
                                                                  nat.ptr(derived), nat.stream_handle(params[0].device)),
                          'sqd_sgd_clip_step_chunked_ema')
            else:
                nat.check(nat.lib().sqd_sgd_clip_step_chunked_dev(nat.ptr(self._table), nat.ptr(self._chunks), self._chunks.shape[0],
                                                                  nat.ptr(flat), nat.ptr(parts), nat.ptr(norm), nat.ptr(self._hyper_dev),
                                                                  nat.stream_handle(params[0].device)), 'sqd_sgd_clip_step_chunked_dev')
        elif max_norm > 0 and flat is not None:
            parts, norm = self._sumsq(flat)
            nat.check(nat.lib().sqd_sgd_clip_step_chunked(nat.ptr(self._table), nat.ptr(self._chunks), self._chunks.shape[0], nat.ptr(flat),
                                                          nat.ptr(parts), nat.ptr(norm), max_norm, self.lr, self.momentum, self.weight_decay,
                                                          nat.stream_handle(params[0].device)), 'sqd_sgd_clip_step_chunked')
        else:
            if max_norm > 0:
                norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
            nat.check(nat.lib().sqd_sgd_clip_step(nat.ptr(self._table), len(params), nat.ptr(flat), nat.ptr(norm), max_norm, self.lr,
                                                  self.momentum, self.weight_decay, 64, nat.stream_handle(params[0].device)),
                      'sqd_sgd_clip_step')
        torch.autograd.graph.increment_version(params)        # (the packed-weight caches key on the version counters)
        self.last_norm = norm
        return norm if closure is None else loss

    def state_dict(self):
        """With the EMA on, also the averaged weights and the count of averaged steps (read from the device: one sync, at save time)."""
        g = self.param_groups[0]
        sd = {'momentum_flat': self.momentum_flat.clone(), 'lr': g['lr'], 'momentum': g['momentum'], 'weight_decay': g['weight_decay'],
              'max_norm': g['max_norm'], 'initial_lr': g.get('initial_lr')}
        if self.ema_on:
            sd.update(self._ema_state(), n=self.step_counts()[1])
        return sd

    def load_state_dict(self, sd):
        self.momentum_flat.copy_(sd['momentum_flat'].to(self.momentum_flat.device))
        g = self.param_groups[0]
        for k in ('lr', 'momentum', 'weight_decay', 'max_norm'):
            if sd.get(k) is not None:
                g[k] = float(sd[k])
        if sd.get('initial_lr') is not None:
            g['initial_lr'] = float(sd['initial_lr'])
        if self.ema_on:
            self._load_ema_state(sd)
            self._set_step_counts(0, sd.get('n', 0))


class FusedClipAdamW(FusedClipBase):
    """``torch.nn.utils.clip_grad_norm_(params, max_norm)`` + ``torch.optim.AdamW(params, lr, betas, eps, weight_decay).step()``
    (non-amsgrad, decoupled decay) and, with ``ema_decay > 0``, the weight EMA of ``FusedClipBase``, as the launches of ``FusedClipSGD``:
    the sum of squares of the flat gradient, a one-thread begin launch and ONE launch over all parameter tensors (csrc/optim.hip,
    ``sqd_adamw_clip_step_chunked``).  Per element, in torch's order: ``g = grad * coef; p -= lr wd p; m = b1 m + (1 - b1) g;
    v = b2 v + (1 - b2) g g; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)``.

    A ``torch.optim.Optimizer`` with ONE parameter group: ``param_groups[0]`` carries ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` /
    ``max_norm`` / ``ema_decay`` / ``ema_warmup`` and drives every step, so ``StepLR`` and warm-up schedules work.  The hyper-parameters are
    ALWAYS read from a device table (there is no launch-argument form: one form, one set of bits), rewritten only when a value changed;
    the step count of the bias correction lives on the device, so the step is capturable and ``GraphedStep`` / ``cfg.graph_step`` accept
    it.  ``max_norm > 0`` clips INSIDE ``step()`` (see ``FusedClipSGD``).  Gradients that are separate tensors are taken by address,
    their norm by torch's foreach norm.  State: ``state[p]['exp_avg']`` / ``['exp_avg_sq']`` / ``['ema']`` are views of flat buffers."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, ema_decay=0.0, ema_warmup=False,
                 flat_grad=None):
        betas = (float(betas[0]), float(betas[1]))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or not float(eps) >= 0.0:
            raise ValueError(f'FusedClipAdamW: betas in [0, 1) and eps >= 0, got {betas!r}, {eps!r}')
        super().__init__(params, dict(lr=float(lr), betas=betas, eps=float(eps), weight_decay=float(weight_decay), max_norm=float(max_norm),
                                      ema_decay=float(ema_decay), ema_warmup=bool(ema_warmup)), flat_grad)
        self.exp_avg_flat, self._m = self._flat_state('exp_avg')
        self.exp_avg_sq_flat, self._v = self._flat_state('exp_avg_sq')
        self.hyper_on_device = True                    # (always: GraphedStep sets and restores the attribute, nothing reads it here)

    betas = property(lambda self: tuple(float(b) for b in self.param_groups[0]['betas']))
    eps = property(lambda self: self._hyper('eps'))

    def _hyper_values(self):
        b1, b2 = self.betas
        return (self.lr, b1, b2, self.eps, self.weight_decay, self.max_norm, self.ema_decay, float(self.ema_warmup))

    @torch.no_grad()
    def step(self, closure=None):
        """One clip + AdamW (+ EMA) step.  Returns the total gradient norm as ``FusedClipSGD.step`` does: a 0-dim DEVICE tensor that the
        next step overwrites (flat layout), or None without clipping."""
        from . import _native as nat
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_step_allowed()
        params = self.params
        dev = params[0].device
        flat, grads = self._gradients()
        self._ensure_tables(flat, grads, self._m, self._v)
        self.refresh_hyper()                           # (writes when a value changed; under capture: raises if it would have to)
        parts = norm = total_norm = None
        if self.max_norm > 0:                          # structural: a captured step keeps or lacks the norm launch
            if flat is not None:
                parts, norm = self._sumsq(flat)
            else:
                norm = total_norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
        _, derived = self._begin(adam=True)
        nat.check(nat.lib().sqd_adamw_clip_step_chunked(nat.ptr(self._table), nat.ptr(self._chunks), self._chunks.shape[0], nat.ptr(flat),
                                                        nat.ptr(parts), nat.ptr(total_norm), nat.ptr(norm if parts is not None else None),
                                                        nat.ptr(self._hyper_dev), nat.ptr(derived), int(self.ema_on),
                                                        nat.stream_handle(dev)), 'sqd_adamw_clip_step_chunked')
        torch.autograd.graph.increment_version(params)        # (the packed-weight caches key on the version counters)
        self.last_norm = norm
        return norm if closure is None else loss

    def state_dict(self):
        """The moments, the EMA, the hyper-parameters and the device counts ``t`` / ``n`` (one sync to read them, at save time only)."""
        g = self.param_groups[0]
        t, n = self.step_counts()
        sd = {'exp_avg_flat': self.exp_avg_flat.clone(), 'exp_avg_sq_flat': self.exp_avg_sq_flat.clone(), 't': t, 'n': n,
              'lr': g['lr'], 'betas': tuple(g['betas']), 'eps': g['eps'], 'weight_decay': g['weight_decay'], 'max_norm': g['max_norm'],
              'initial_lr': g.get('initial_lr')}
        sd.update(self._ema_state())
        return sd

    def load_state_dict(self, sd):
        """``state_dict()`` of this class, or of a ``torch.optim.AdamW`` over the same parameter list (``exp_avg``, ``exp_avg_sq``, ``step``
        per parameter; its group's lr / betas / eps / weight_decay are taken over, the EMA starts afresh)."""
        g = self.param_groups[0]
        if 'state' in sd and 'param_groups' in sd:
            groups, state = sd['param_groups'], sd['state']
            ids = [i for grp in groups for i in grp['params']]
            if len(groups) != 1 or len(ids) != len(self.params):
                raise ValueError(f'FusedClipAdamW.load_state_dict: a torch optimizer state with {len(groups)} group(s) over {len(ids)} '
                                 f'parameters, this optimizer has one group over {len(self.params)}')
            if groups[0].get('amsgrad'):
                raise ValueError('FusedClipAdamW.load_state_dict: amsgrad state is not supported')
            steps = set()
            for i, m, v in zip(ids, self._m, self._v):
                st = state.get(i)
                if st is None:                         # (torch creates the state at a parameter's first step)
                    m.zero_(); v.zero_(); steps.add(0)
                    continue
                if st['exp_avg'].numel() != m.numel():
                    raise ValueError(f'FusedClipAdamW.load_state_dict: parameter {i} has {st["exp_avg"].numel()} elements in the state, '
                                     f'{m.numel()} here')
                m.copy_(st['exp_avg'].reshape(-1).to(m.device)); v.copy_(st['exp_avg_sq'].reshape(-1).to(v.device))
                steps.add(int(float(st['step'])))
            if len(steps) != 1:
                raise ValueError(f'FusedClipAdamW.load_state_dict: the parameters are at different steps {sorted(steps)} (one count here)')
            grp = groups[0]
            g['lr'], g['betas'], g['eps'] = float(grp['lr']), tuple(float(b) for b in grp['betas']), float(grp['eps'])
            g['weight_decay'] = float(grp['weight_decay'])
            if grp.get('initial_lr') is not None:
                g['initial_lr'] = float(grp['initial_lr'])
            self._set_step_counts(steps.pop(), 0)
            return
        self.exp_avg_flat.copy_(sd['exp_avg_flat'].to(self.exp_avg_flat.device))
        self.exp_avg_sq_flat.copy_(sd['exp_avg_sq_flat'].to(self.exp_avg_sq_flat.device))
        for k in ('lr', 'eps', 'weight_decay', 'max_norm'):
            if sd.get(k) is not None:
                g[k] = float(sd[k])
        if sd.get('betas') is not None:
            g['betas'] = tuple(float(b) for b in sd['betas'])
        if sd.get('initial_lr') is not None:
            g['initial_lr'] = float(sd['initial_lr'])
        self._load_ema_state(sd)
        self._set_step_counts(sd.get('t', 0), sd.get('n', 0))


SPARSE_CAP_MIN = 64
LOG_RING = 64                                    # batch means the device log keeps (a print interval reads the latest)
LOG_ROWS = ('class_loss', 'score_loss', 'bbox_loss', 'loss')      # row order of the loss launches' [4,B] output = of the device log


def sparse_capacity(total, current=0):
    """Entries the fixed sparse-gt buffers of a captured step hold: the next power of two at or above the largest ``total`` seen, at
    least ``SPARSE_CAP_MIN``; never shrinks (``current``: the capacity so far)."""
    cap = max(int(current), SPARSE_CAP_MIN)
    while cap < int(total):
        cap *= 2
    return cap


def gt_form(batch):
    """'dense' | 'sparse' | 'masked': which loss launches a batch runs."""
    if 'gt' in batch:
        return 'dense'
    if 'gt_sparse' not in batch:
        raise ValueError('GraphedStep: the batch carries neither gt nor gt_sparse')
    return 'masked' if batch.get('gt_ignore') is not None else 'sparse'


def step_signature(image_shape, form, cap, training, trainable, clip_on, loss_weights):
    """What a captured training step is valid for: a step whose signature differs runs other launches, other grids or other buffers.
    ``image_shape``: (B, H, W); ``form``: ``gt_form``; ``cap``: the sparse capacity (0 for dense); ``trainable``: names of the
    parameters that require grad; ``clip_on``: whether the gradient norm is evaluated; ``loss_weights``: launch arguments of the loss."""
    B, H, W = (int(v) for v in image_shape)
    return (B, H, W, str(form), int(cap), bool(training), tuple(trainable), bool(clip_on), tuple(float(w) for w in loss_weights))


class GraphedStep:
    """The training step -- ``forward_mean``, ``zero_grad``, ``backward``, ``optimizer.step`` and the device log -- replayed as ONE
    captured hipGraph, the product form of what ``bench.py --mode train`` measures.

    ``step(batch)`` -> (mean loss, 0-dim device tensor; stats dict of per-image device vectors).  The returned tensors (and the
    optimizer's ``last_norm``) are static: the next step overwrites them.  The first call with a new signature (``step_signature``)
    is a real eager step on this object's side stream and does every lazy initialisation; the second stages the batch into static
    buffers, captures and replays; later calls stage, refresh the optimizer's device hyper-parameter table and replay.  Every call is
    exactly one optimizer step of the all-eager loop, bit for bit.  The graphs are made for ONE batch size, the largest seen so far
    (``batch_size``): a smaller batch -- a ragged last one -- and a signature beyond ``max_graphs`` run the eager step on the same
    stream and objects; a larger one takes over and drops what was made for the smaller.

    Construction changes the optimizer it is given, because the captured step needs both: ``optimizer.hyper_on_device`` becomes True
    (``step()`` launches the device-table kernel from then on, inside and outside this object) and a missing ``flat_grad`` is pointed
    at the model's flat gradient buffer.  ``release()`` drops the graphs and gives the optimizer its two attributes back.

    After every replay the parameters' version counters are advanced, as the Python of ``FusedClipSGD.step`` that the replay skipped
    would have: the packed-weight caches key on them, and an eval forward / a ``Detector`` on the same parameters re-packs instead of
    computing with stale weights.  ``p.grad`` stays what the captured backward left: views of the graph pool's flat buffer, holding
    the latest step's unclipped gradients.  One process only: a process group with more than one rank is refused."""

    def __init__(self, model, optimizer, cfg=None, max_graphs=4):
        if not isinstance(optimizer, FusedClipBase):
            raise ValueError(f'GraphedStep: the optimizer must be a FusedClipSGD or a FusedClipAdamW (their steps are capturable and read '
                             f'their hyper-parameters and step counts from device memory), got {type(optimizer).__name__}')
        d = _dist()
        if d is not None and d.get_world_size() > 1:
            raise ValueError(f'GraphedStep: a process group with {d.get_world_size()} ranks -- the captured gradient exchange is not '
                             'supported, train multi-GPU with graph_step off')
        if not hasattr(model, 'forward_mean'):
            raise ValueError(f'GraphedStep: the model must have forward_mean (SqueezeDetWithLoss), {type(model).__name__} has none')
        self.model, self.optimizer, self.cfg = model, optimizer, cfg
        self.base = find_base(model)
        # the loss weights are launch arguments of the captured loss kernels: they are read where backward.py reads them, from the Loss
        from .model import Loss
        self._loss = next((m for m in model.modules() if isinstance(m, Loss)), None)
        if self._loss is None:
            raise ValueError(f'GraphedStep: no model.Loss module inside {type(model).__name__}: the loss weights a captured step holds '
                             'cannot be watched for changes')
        self._optimizer_was = (optimizer.hyper_on_device, optimizer.flat_grad)
        if optimizer.flat_grad is None:
            base = self.base
            optimizer.flat_grad = lambda: base.last_grad_flat
        optimizer.hyper_on_device = True
        self.device = optimizer.params[0].device
        self.stream = torch.cuda.Stream(device=self.device)
        self.pool = torch.cuda.graph_pool_handle()
        self.max_graphs = int(max_graphs)
        self.batch_size = None                   # the batch size the graphs are made for: the largest seen so far
        self.captures = 0
        self.replays = 0
        self.eager_steps = 0
        self._graphs = {}                        # signature -> (CUDAGraph, outputs, gradients, kept-alive operands)
        self._seen = set()                       # signatures (capacity left out) that had their eager step
        self._bufs = {}                          # (B, H, W, form) -> static batch
        self._cap = {}                           # (B, H, W, form) -> sparse capacity
        self._live = None                        # the signature whose gradients p.grad points at
        self._one = torch.ones((), device=self.device)
        # the device log in one buffer (one copy reads it): sums double[5] | ring float[LOG_RING][4] | cursor
        self._log = torch.zeros(40 + 16 * LOG_RING + 8, device=self.device, dtype=torch.uint8)
        self._log_sums, self._log_ring, self._log_cursor = self._log_views(self._log)

    @staticmethod
    def _log_views(buf):
        return (buf[:40].view(torch.float64), buf[40:40 + 16 * LOG_RING].view(torch.float32).view(LOG_RING, 4),
                buf[40 + 16 * LOG_RING:40 + 16 * LOG_RING + 4].view(torch.int32))

    # ---- the log ----
    def reset_log(self):
        """Zero the sums (the start of an epoch); the ring and its cursor go on."""
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self._log_sums.zero_()
        cur.wait_stream(self.stream)

    def read_log(self):
        """One copy and one host sync: -> (sums: {key: float64 sum of the per-image values since ``reset_log``} + 'images';
        latest: {key: batch mean of the latest step} or None before the first step; steps pushed so far)."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.stream)
        sums, ring, cursor = self._log_views(self._log.cpu())
        n = int(cursor[0]) & 0xffffffff
        out = {k: float(sums[i]) for i, k in enumerate(LOG_ROWS)}
        out['images'] = float(sums[4])
        latest = None if n == 0 else {k: float(ring[(n - 1) % LOG_RING, i]) for i, k in enumerate(LOG_ROWS)}
        return out, latest, n

    def _log_push(self, stats):
        from . import _native as nat
        rows = [stats[k] for k in LOG_ROWS]
        B = rows[0].shape[0]
        p0 = rows[0].data_ptr()
        if any(r.dtype != torch.float32 or r.dim() != 1 or r.shape[0] != B or not r.is_contiguous() or r.data_ptr() != p0 + 4 * B * i
               for i, r in enumerate(rows)):
            raise RuntimeError('GraphedStep: the loss statistics are not the rows of one fp32 [4,B] tensor (class, score, bbox, total)')
        nat.check(nat.lib().sqd_train_log_push(nat.c_p(p0), B, nat.ptr(self._log_sums), nat.ptr(self._log_ring), nat.ptr(self._log_cursor),
                                               LOG_RING, nat.stream_handle(self.device)), 'sqd_train_log_push')

    # ---- the step ----
    def _sequence(self, batch):
        """The step itself, on the current stream: eager, or recorded when that stream is capturing."""
        mean, stats = self.model.forward_mean(batch)
        self.optimizer.zero_grad()
        mean.backward(self._one)
        self.optimizer.step()
        self._log_push(stats)
        # detached: a loss kept with its autograd graph would keep this step's nodes alive into the next step
        return mean.detach(), {k: v.detach() for k, v in stats.items()}

    def signature(self, batch, cap=None):
        B, _, H, W = batch['image'].shape
        form = gt_form(batch)
        loss = self._loss
        weights = (loss.class_loss_weight, loss.positive_score_loss_weight, loss.negative_score_loss_weight, loss.bbox_loss_weight)
        if cap is None:
            cap = self._cap.get((B, H, W, form), 0)
        return step_signature((B, H, W), form, cap, self.model.training,
                              [n for n, p in self.model.named_parameters() if p.requires_grad], self.optimizer.max_norm > 0, weights)

    def _stage(self, key, batch):
        """Copy the batch into the static buffers of ``key`` (device to device, on the current stream) -> (the static batch, whether the
        sparse capacity grew)."""
        form = key[3]
        image = batch['image']
        bufs = self._bufs.get(key)
        grew = False
        if bufs is None:
            bufs = self._bufs[key] = {'image': torch.empty_like(image, memory_format=torch.contiguous_format)}
            if form == 'dense':
                bufs['gt'] = torch.empty_like(batch['gt'], memory_format=torch.contiguous_format)
        bufs['image'].copy_(image)
        if form == 'dense':
            bufs['gt'].copy_(batch['gt'])
            return bufs, grew
        from .ops import SparseGT
        sgt = batch['gt_sparse']
        total = int(sgt.anchor_idx.shape[0])
        cap = sparse_capacity(total, self._cap.get(key, 0))
        if cap != self._cap.get(key, 0):
            grew = key in self._cap
            self._cap[key] = cap
            dev = image.device
            bufs['gt_sparse'] = SparseGT(torch.zeros(cap, device=dev, dtype=torch.int32), torch.zeros(cap, 4, device=dev),
                                         torch.zeros(cap, 4, device=dev), torch.zeros(cap, device=dev, dtype=torch.int32),
                                         torch.zeros(image.shape[0] + 1, device=dev, dtype=torch.int32))
        st = bufs['gt_sparse']
        # offsets and the first `total` entries: the launches bound every image's list by offsets, entries past offsets[B] are never read
        st.offsets.copy_(sgt.offsets)
        if total:
            st.anchor_idx[:total].copy_(sgt.anchor_idx)
            st.boxes[:total].copy_(sgt.boxes)
            st.deltas[:total].copy_(sgt.deltas)
            st.class_ids[:total].copy_(sgt.class_ids)
        if form == 'masked':
            if 'gt_ignore' not in bufs:
                bufs['gt_ignore'] = torch.empty_like(batch['gt_ignore'], memory_format=torch.contiguous_format)
            bufs['gt_ignore'].copy_(batch['gt_ignore'])
        return bufs, grew

    def _capture(self, sbatch):
        import gc
        from . import timing
        params = self.optimizer.params
        torch.cuda.synchronize(self.device)
        # The captured forward must hold the re-pack launches of every packed weight copy, whatever ran since the last optimizer step
        # (an eval forward brings the caches up to date): make every copy stale.  One eager refresh first, so that the descriptor tables
        # of those launches exist -- a table built during the capture would be a host-to-device copy inside it.
        torch.autograd.graph.increment_version(params)
        self.base.refresh_plans()
        torch.autograd.graph.increment_version(params)
        self.optimizer.refresh_hyper()
        timer = timing._timer
        timing.set_timer(None)                   # (event brackets do not belong into a captured step)
        gc_was_on = gc.isenabled()
        g = torch.cuda.CUDAGraph()
        try:
            gc.collect()
            gc.disable()                         # (a collection inside the capture would run GPU finalisers between two captured launches)
            # thread_local: loader threads touch the runtime while this thread captures
            with torch.cuda.graph(g, stream=self.stream, pool=self.pool, capture_error_mode='thread_local'):
                out = self._sequence(sbatch)
        except Exception as e:
            raise RuntimeError(f'GraphedStep: capturing the training step failed ({type(e).__name__}: {e})') from e
        finally:
            timing.set_timer(timer)
            if gc_was_on:
                gc.enable()
        self.captures += 1
        grads = [p.grad for p in params]
        # what the graph reads and writes outside its pool stays alive with it (caches that are bounded would drop them otherwise)
        keep = (list(self.base.plan_cache._tables.values()), list(self.base._wgrad_batches.values()), self.base.last_grad_flat)
        return g, out, grads, keep

    def _drop_graphs(self):
        """Forget every graph and static buffer (nothing may still be replaying them)."""
        torch.cuda.synchronize(self.device)
        self._graphs.clear(); self._seen.clear(); self._bufs.clear(); self._cap.clear()
        self._live = None
        self.pool = torch.cuda.graph_pool_handle()

    def release(self):
        """Drop the graphs and give the optimizer back what construction changed (``hyper_on_device``, ``flat_grad``)."""
        self._drop_graphs()
        self.optimizer.hyper_on_device, self.optimizer.flat_grad = self._optimizer_was

    def _eager(self, batch):
        self.eager_steps += 1
        self._live = None
        return self._sequence(batch)

    def _run(self, batch):
        image = batch['image']
        B, _, H, W = image.shape
        if self.batch_size is None or B > self.batch_size:
            if self.batch_size is not None:
                self._drop_graphs()              # (the first batches were the odd ones: nothing made for them is used again)
            self.batch_size = B
        if B != self.batch_size:
            return self._eager(batch)            # a ragged last batch: no buffers, no graph
        form = gt_form(batch)
        key = (B, H, W, form)
        sbatch, grew = self._stage(key, batch)
        if grew:
            # the capacity doubled: the graphs of this shape hold the old buffers
            torch.cuda.synchronize(self.device)
            for s in [s for s in self._graphs if s[:4] == key]:
                del self._graphs[s]
            # later captures go to a pool of their own: the old one may have lost its last graph while p.grad still holds blocks of it
            self.pool = torch.cuda.graph_pool_handle()
        sig = self.signature(batch)
        seen_key = sig[:4] + sig[5:]
        entry = self._graphs.get(sig)
        if entry is None:
            if seen_key not in self._seen:
                self._seen.add(seen_key)
                return self._eager(sbatch)       # the first step of this signature: real, and every lazy initialisation
            if len(self._graphs) >= self.max_graphs:
                return self._eager(sbatch)
            entry = self._graphs[sig] = self._capture(sbatch)
        else:
            self.optimizer.refresh_hyper()
        g, out, grads, _keep = entry
        g.replay()
        self.replays += 1
        params = self.optimizer.params
        torch.autograd.graph.increment_version(params)        # the Python a replay skipped (the optimizer's step())
        if self._live != sig:
            for p, gr in zip(params, grads):
                p.grad = gr
            self.base.last_grad_flat = _keep[2]
            self._live = sig
        return out

    def step(self, batch):
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)             # the batch was produced on the caller's stream
        with torch.cuda.stream(self.stream):
            out = self._run(batch)
        cur.wait_stream(self.stream)             # the caller reads the outputs (and frees the batch) on its own stream
        return out


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
