"""The one-launch optimizers of the training path (csrc/optim.hip; re-exported by ``trainer``): ``FusedClipSGD`` and
``FusedClipAdamW`` -- ``clip_grad_norm_`` + the optimizer step (+ a weight EMA) over all parameter tensors in one launch -- on
``FusedClipBase``, which holds what they share: the tables, the device hyper-parameter table (``HyperTable``), the device step
counters, the scaffolding of ``step()`` and of the state dicts, and the averaged weights."""
from __future__ import annotations

import contextlib

import torch

from . import _native as nat


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
        self._chunks = self._chunk_table()
        self._table_key = key

    def _chunk_table(self):
        """[chunks][2] int64 {tensor, first element}: equal chunks of the 64 tensors (16 .. 500 k elements), one workgroup per chunk."""
        ce = int(nat.lib().sqd_sgd_chunk_elems())
        chunks = [[i, e] for i, p in enumerate(self.params) for e in range(0, p.numel(), ce)]
        return torch.tensor(chunks, dtype=torch.int64).to(self.params[0].device)

    def _sumsq(self, flat):
        """The norm of the flat gradient buffer: partial sums of squares by one small launch, finished (fixed order) inside the step.
        -> (parts, the 0-dim norm the step launch writes)."""
        if self._norm_ws is None:
            self._norm_ws = torch.empty(int(nat.lib().sqd_grad_sumsq_parts()) + 1, device=flat.device, dtype=torch.float32)
        parts, norm = self._norm_ws[:-1], self._norm_ws[-1]
        nat.check(nat.lib().sqd_grad_sumsq(nat.ptr(flat), self.total, nat.ptr(parts), nat.stream_handle(flat.device)), 'sqd_grad_sumsq')
        return parts, norm

    def _begin(self, adam):
        """The one-thread launch in front of a step: advances the device counts, writes the derived table -> (counters, derived)."""
        steps = self._steps()
        counters, derived = steps[:2], steps[2:6].view(torch.float32)
        nat.check(nat.lib().sqd_optim_begin(nat.ptr(self._hyper_dev), nat.ptr(counters), nat.ptr(derived), int(adam), int(self.ema_on),
                                            nat.stream_handle(steps.device)), 'sqd_optim_begin')
        return counters, derived

    def _steps(self):
        """The device counters and derived table: allocated on first use, moved (counts and all) when the parameters' device changed."""
        dev = self.params[0].device
        if self._steps_dev is None or self._steps_dev.device != dev:
            was = self._steps_dev
            self._steps_dev = torch.zeros(8, device=dev, dtype=torch.int32)
            if was is not None:
                self._steps_dev.copy_(was)
        return self._steps_dev

    def step_counts(self):
        """(t, n): optimizer steps counted for the bias correction (0 for SGD) and averaged steps, read from the device (one host sync)."""
        if self._steps_dev is None:
            return 0, 0
        t, n = self._steps_dev[:2].tolist()
        return int(t), int(n)

    def _set_step_counts(self, t, n):
        self._steps()[:2].copy_(torch.tensor([int(t), int(n)], dtype=torch.int32))

    def norm_value(self):
        """The latest step's total gradient norm as a Python float (one host sync), or None before the first clipped step."""
        return None if self.last_norm is None else float(self.last_norm)

    # ---- the averaged weights ----
    def _swap(self):
        params = self.params
        key = (tuple(p.data_ptr() for p in params), self.ema_flat.data_ptr())
        if key != self._swap_key:
            if any(not p.is_contiguous() for p in params):
                raise RuntimeError(f'{type(self).__name__}.averaged_weights: parameters must stay contiguous fp32 GPU tensors')
            rows = [[p.data_ptr(), 0, 0, p.numel(), 0, e.data_ptr()] for p, e in zip(params, self._emas)]
            self._swap_tables = (torch.tensor(rows, dtype=torch.int64).to(params[0].device), self._chunk_table())
            self._swap_key = key
        table, chunks = self._swap_tables
        nat.check(nat.lib().sqd_param_swap(nat.ptr(table), nat.ptr(chunks), chunks.shape[0], nat.stream_handle(params[0].device)),
                  'sqd_param_swap')
        torch.autograd.graph.increment_version(params)        # (the packed-weight caches key on the version counters: PlanCache re-packs)

    @contextlib.contextmanager
    def averaged_weights(self):
        """Context manager: inside, the parameters hold the EMA (one swap launch; the version counters advance, so the packed-weight
        caches re-pack without a manual ``invalidate_plans``) -- evaluate or export there; leaving swaps back, and the parameters are
        bit-identical to before.  Raises (on entry) when the EMA is off, when nested and under stream capture."""
        who = type(self).__name__
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

    # ---- what every step() starts and ends with ----
    def _step_begin(self, closure):
        """-> (the closure's loss or None, the flat gradient buffer or None, the gradients)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._averaging:
            raise RuntimeError(f'{type(self).__name__}.step: inside averaged_weights() (the parameters hold the EMA)')
        flat, grads = self._gradients()
        return loss, flat, grads

    @staticmethod
    def _foreach_norm(grads):
        """The total norm of gradients that are separate tensors, as ``clip_grad_norm_`` evaluates it (0-dim device tensor)."""
        return torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))

    def _chunked_head(self, flat):
        """The leading arguments of every chunked entry point: the descriptor table, the chunk table, its rows, the flat gradient."""
        return nat.ptr(self._table), nat.ptr(self._chunks), self._chunks.shape[0], nat.ptr(flat)

    def _step_end(self, norm, closure, loss):
        torch.autograd.graph.increment_version(self.params)   # (the packed-weight caches key on the version counters)
        self.last_norm = norm
        return norm if closure is None else loss

    # ---- the scalar hyper-parameters in a state dict ----
    def _hyper_state(self, keys):
        g = self.param_groups[0]
        sd = {k: tuple(g[k]) if isinstance(g[k], (tuple, list)) else g[k] for k in keys}
        sd['initial_lr'] = g.get('initial_lr')
        return sd

    def _load_hyper_state(self, sd, keys):
        g = self.param_groups[0]
        for k in tuple(keys) + ('initial_lr',):
            v = sd.get(k)
            if v is not None:
                g[k] = tuple(float(b) for b in v) if isinstance(v, (tuple, list)) else float(v)

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
        loss, flat, grads = self._step_begin(closure)
        params = self.params
        if self.ema_on and not (self.hyper_on_device and flat is not None):
            raise RuntimeError('FusedClipSGD.step: ema_decay > 0 runs in the chunked launch that reads its hyper-parameters from device '
                               'memory, not on the launch-argument path: it needs hyper_on_device = True and the flat-gradient layout '
                               '(flat_grad given and every p.grad a consecutive view of that buffer, as the HIP backward leaves them)')
        if self.hyper_on_device and flat is None:
            raise RuntimeError('FusedClipSGD.step: hyper_on_device needs the flat-gradient layout (flat_grad given and every p.grad a '
                               'consecutive view of that buffer, as the HIP backward leaves them); these gradients are separate tensors')
        self._ensure_tables(flat, grads, self._bufs)
        head, stream = self._chunked_head(flat), nat.stream_handle(params[0].device)
        norm = None
        max_norm = self.max_norm
        if self.hyper_on_device:
            self.refresh_hyper()                       # (writes when a value changed; under capture: raises if it would have to)
            parts = None
            if max_norm > 0:                           # structural: a captured step keeps or lacks the norm launch
                parts, norm = self._sumsq(flat)
            if self.ema_on:
                _, derived = self._begin(adam=False)
                nat.check(nat.lib().sqd_sgd_clip_step_chunked_ema(*head, nat.ptr(parts), nat.ptr(norm), nat.ptr(self._hyper_dev),
                                                                  nat.ptr(derived), stream), 'sqd_sgd_clip_step_chunked_ema')
            else:
                nat.check(nat.lib().sqd_sgd_clip_step_chunked_dev(*head, nat.ptr(parts), nat.ptr(norm), nat.ptr(self._hyper_dev), stream),
                          'sqd_sgd_clip_step_chunked_dev')
        elif max_norm > 0 and flat is not None:
            parts, norm = self._sumsq(flat)
            nat.check(nat.lib().sqd_sgd_clip_step_chunked(*head, nat.ptr(parts), nat.ptr(norm), max_norm, self.lr, self.momentum,
                                                          self.weight_decay, stream), 'sqd_sgd_clip_step_chunked')
        else:
            if max_norm > 0:
                norm = self._foreach_norm(grads)
            nat.check(nat.lib().sqd_sgd_clip_step(nat.ptr(self._table), len(params), nat.ptr(flat), nat.ptr(norm), max_norm, self.lr,
                                                  self.momentum, self.weight_decay, 64, stream), 'sqd_sgd_clip_step')
        return self._step_end(norm, closure, loss)

    _STATE_KEYS = ('lr', 'momentum', 'weight_decay', 'max_norm')

    def state_dict(self):
        """With the EMA on, also the averaged weights and the count of averaged steps (read from the device: one sync, at save time)."""
        sd = {'momentum_flat': self.momentum_flat.clone(), **self._hyper_state(self._STATE_KEYS)}
        if self.ema_on:
            sd.update(self._ema_state(), n=self.step_counts()[1])
        return sd

    def load_state_dict(self, sd):
        self.momentum_flat.copy_(sd['momentum_flat'].to(self.momentum_flat.device))
        self._load_hyper_state(sd, self._STATE_KEYS)
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
        loss, flat, grads = self._step_begin(closure)
        self._ensure_tables(flat, grads, self._m, self._v)
        self.refresh_hyper()                           # (writes when a value changed; under capture: raises if it would have to)
        parts = norm = total_norm = None
        if self.max_norm > 0:                          # structural: a captured step keeps or lacks the norm launch
            if flat is not None:
                parts, norm = self._sumsq(flat)
            else:
                norm = total_norm = self._foreach_norm(grads)
        _, derived = self._begin(adam=True)
        nat.check(nat.lib().sqd_adamw_clip_step_chunked(*self._chunked_head(flat), nat.ptr(parts), nat.ptr(total_norm),
                                                        nat.ptr(norm if parts is not None else None), nat.ptr(self._hyper_dev),
                                                        nat.ptr(derived), int(self.ema_on), nat.stream_handle(self.params[0].device)),
                  'sqd_adamw_clip_step_chunked')
        return self._step_end(norm, closure, loss)

    _STATE_KEYS = ('lr', 'betas', 'eps', 'weight_decay', 'max_norm')

    def state_dict(self):
        """The moments, the EMA, the hyper-parameters and the device counts ``t`` / ``n`` (one sync to read them, at save time only)."""
        t, n = self.step_counts()
        sd = {'exp_avg_flat': self.exp_avg_flat.clone(), 'exp_avg_sq_flat': self.exp_avg_sq_flat.clone(), 't': t, 'n': n,
              **self._hyper_state(self._STATE_KEYS)}
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
        self._load_hyper_state(sd, self._STATE_KEYS)
        self._load_ema_state(sd)
        self._set_step_counts(sd.get('t', 0), sd.get('n', 0))

