"""The captured training step (re-exported by ``trainer``): ``GraphedStep`` replays forward, backward, the optimizer step and
the device log as one hipGraph; ``step_signature`` says what a capture is valid for."""
from __future__ import annotations

import torch

from .exchange import _dist, find_base
from .optim import FusedClipBase

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


def step_signature(image_shape, form, cap, training, trainable, clip_on, loss_weights, bbox_loss='l2'):
    """What a captured training step is valid for: a step whose signature differs runs other launches, other grids or other buffers.
    ``image_shape``: (B, H, W); ``form``: ``gt_form``; ``cap``: the sparse capacity (0 for dense); ``trainable``: names of the
    parameters that require grad; ``clip_on``: whether the gradient norm is evaluated; ``loss_weights`` and ``bbox_loss``: launch arguments of the
    loss (the regression kind selects its kernels)."""
    B, H, W = (int(v) for v in image_shape)
    return (B, H, W, str(form), int(cap), bool(training), tuple(trainable), bool(clip_on), tuple(float(w) for w in loss_weights),
            str(bbox_loss))


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
                              [n for n, p in self.model.named_parameters() if p.requires_grad], self.optimizer.max_norm > 0, weights,
                              getattr(loss, 'bbox_loss', 'l2'))

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
