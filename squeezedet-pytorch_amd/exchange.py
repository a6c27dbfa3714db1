"""The data-parallel gradient exchange of the training path (re-exported by ``trainer``).

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


def through_flat(tensors, collective):
    """``collective(flat)`` on ONE flat copy of ``tensors`` (not one call per tensor), the result written back through views with
    ``copy_``: version counters move, so the packed-weight caches of the HIP plan refresh.  -> the flat copy."""
    with torch.no_grad():
        flat = torch.cat([t.detach().reshape(-1) for t in tensors])
        collective(flat)
        off = 0
        for t in tensors:
            n = t.numel()
            t.copy_(flat[off:off + n].view_as(t))
            off += n
    return flat


def broadcast_parameters(module, src=0, group=None):
    """Identical weights on every rank, ONE broadcast of a flat copy (``through_flat``)."""
    d = _dist()
    if d is None or d.get_world_size(group) == 1:
        return
    through_flat(list(module.parameters()), lambda flat: d.broadcast(flat, src=src, group=group))


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
                through_flat(tensors, lambda flat: d.broadcast(flat, src=0, group=group))
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

    def mean(flat):
        if d is None or world <= 1:
            return
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
        return through_flat([p.grad for p in params], mean)
    flat = g0.as_strided((off,), (1,), g0.storage_offset())
    mean(flat)
    return flat
