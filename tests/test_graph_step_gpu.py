"""GPU tier of the captured training step in the product (trainer.GraphedStep, FusedClipSGD.hyper_on_device, the device log,
``cfg.graph_step`` through ``Trainer``).

Everything a replay computes is compared BIT FOR BIT with the plain eager sequence (forward_mean, zero_grad, backward, step) run by a
second model from the same state dict and the same seed: parameters, momentum buffers, per-image loss vectors, the mean loss and the
gradient norm, after every step, dropout on.  The eager side runs the launch-argument optimizer kernel, the graph side the kernel that
reads its hyper-parameters from device memory, so their equality is part of every comparison.  Shapes: autograd_twin.SIZE (64x96: a
4x6 grid, 216 anchors), squeezedet, 3 classes, batches of 2 and 3 images."""
import numpy as np
import pytest
import torch

import fp64_ref as R
from autograd_twin import SIZE

pytestmark = pytest.mark.gpu

C = 3
LR = 1e-3                      # (six unclipped-size steps from the synthetic weights stay finite at this rate; asserted)
KEYS = ('loss', 'class_loss', 'score_loss', 'bbox_loss')


def bits_equal(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))


def make_cfg(**kw):
    import squeezedet_pytorch_amd as sqd
    kw.setdefault('dropout_prob', 0.5)
    return sqd.make_cfg(input_size=SIZE, num_classes=C, device='cuda', **kw)


def make_model(cfg, state_dict=None):
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(state_dict if state_dict is not None else synthetic.make_state_dict('squeezedet', seed=1234, num_classes=C))
    return m.cuda().train()


def make_opt(model, lr=LR, max_norm=5.0):
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, find_base
    base = find_base(model)
    return FusedClipSGD([p for p in model.parameters() if p.requires_grad], lr=lr, momentum=0.9, weight_decay=1e-4, max_norm=max_norm,
                        flat_grad=lambda: base.last_grad_flat)


def make_batch(cfg, form, B, seed, boxes=(3, 8), empty_image=None):
    """One device-resident batch.  sparse / masked: the list of positives of ``make_gt_boxes`` (its ``total`` varies with the seed);
    masked adds an ignore bitmap (two regions per image) and, with ``empty_image``, an image without any object."""
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.annotations import encode_annotations
    batch = {'image': synthetic.make_images(B, SIZE, seed=100 + seed).cuda()}
    if form == 'dense':
        batch['gt'] = synthetic.make_gt(B, cfg.anchors, SIZE, C, seed=seed, min_boxes=boxes[0], max_boxes=boxes[1]).cuda()
        return batch
    cls_list, box_list = synthetic.make_gt_boxes(B, SIZE, C, seed=seed, min_boxes=boxes[0], max_boxes=boxes[1])
    if form == 'sparse':
        batch['gt_sparse'] = encode_annotations(cls_list, box_list, cfg.anchors, C, dense=False)
        return batch
    if empty_image is not None:
        cls_list[empty_image], box_list[empty_image] = np.zeros(0, np.int64), np.zeros((0, 4), np.float32)
    rs = np.random.RandomState(500 + seed)
    ign = []
    for _ in range(B):
        x1, y1 = rs.uniform(0, SIZE[1] - 30, 2), rs.uniform(0, SIZE[0] - 30, 2)
        ign.append(np.stack([x1, y1, x1 + rs.uniform(8, 28, 2), y1 + rs.uniform(8, 28, 2)], 1).astype(np.float32))
    batch['gt_sparse'], batch['gt_ignore'] = encode_annotations(cls_list, box_list, cfg.anchors, C, dense=False, ignore_boxes_list=ign,
                                                                ignore_overlap=0.5)
    return batch


class Eager:
    """The plain sequence on its own model and (launch-argument) optimizer."""

    def __init__(self, cfg, state_dict=None, **opt_kw):
        self.model = make_model(cfg, state_dict)
        self.opt = make_opt(self.model, **opt_kw)
        self.one = torch.ones((), device='cuda')

    def step(self, batch):
        mean, stats = self.model.forward_mean(batch)
        self.opt.zero_grad()
        mean.backward(self.one)
        self.opt.step()
        return mean.detach(), {k: v.detach() for k, v in stats.items()}


class Graphed:
    def __init__(self, cfg, state_dict=None, **opt_kw):
        from squeezedet_pytorch_amd.trainer import GraphedStep
        self.model = make_model(cfg, state_dict)
        self.opt = make_opt(self.model, **opt_kw)
        self.gs = GraphedStep(self.model, self.opt, cfg)

    def step(self, batch):
        return self.gs.step(batch)


def assert_same_state(g, e, tag, out_g=None, out_e=None):
    torch.cuda.synchronize()
    if out_g is not None:
        assert bits_equal(out_g[0], out_e[0]), f'{tag}: mean loss differs: {float(out_g[0])!r} vs {float(out_e[0])!r}'
        assert bool(torch.isfinite(out_e[0])), f'{tag}: the eager loss is not finite'
        for k in KEYS:
            assert bits_equal(out_g[1][k], out_e[1][k]), f'{tag}: per-image {k} differs: {out_g[1][k].tolist()} vs {out_e[1][k].tolist()}'
        if e.opt.max_norm > 0:
            assert bits_equal(g.opt.last_norm, e.opt.last_norm), f'{tag}: norm {float(g.opt.last_norm)!r} vs {float(e.opt.last_norm)!r}'
    for (n, pg), (_, pe) in zip(g.model.named_parameters(), e.model.named_parameters()):
        assert bits_equal(pg, pe), f'{tag}: parameter {n} differs (max abs {float((pg - pe).abs().max()):.3e})'
    assert bool(torch.isfinite(e.opt.momentum_flat).all()), f'{tag}: momentum is not finite'
    assert bits_equal(g.opt.momentum_flat, e.opt.momentum_flat), f'{tag}: momentum buffers differ'


def run_pair(cfg, batches, after_step=None, seed=11, **opt_kw):
    torch.manual_seed(seed)
    g, e = Graphed(cfg, **opt_kw), Eager(cfg, **opt_kw)
    for i, b in enumerate(batches):
        out_g = g.step(b)
        out_e = e.step(b)
        assert_same_state(g, e, f'step {i}', out_g, out_e)
        if after_step is not None:
            after_step(i, g, e)
    return g, e


# ---- 1. the device-hyper kernel against the launch-argument kernel ----------------------------------------------------------------

LAYOUTS = {'mixed': [5, 4096, 3, 4097, 1, 12289, 262147, 1], 'n3': [3], 'tail_big': [4093, 6], 'x4096': [4096, 8192]}


def _chunk_tables(params, bufs):
    from squeezedet_pytorch_amd import _native as nat
    ce = int(nat.lib().sqd_sgd_chunk_elems())
    rows, off = [], 0
    for p, b in zip(params, bufs):
        rows.append([p.data_ptr(), off, b.data_ptr(), p.numel()]); off += p.numel()
    chunks = [[i, e0] for i, p in enumerate(params) for e0 in range(0, p.numel(), ce)]
    return torch.tensor(rows, dtype=torch.int64).cuda(), torch.tensor(chunks, dtype=torch.int64).cuda()


@pytest.mark.parametrize('layout', list(LAYOUTS))
@pytest.mark.parametrize('clip', ['on', 'off'])
def test_dev_kernel_equals_argument_kernel(layout, clip):
    """sqd_sgd_clip_step_chunked_dev (hyper-parameters in a device table written by sqd_fill_f32x4) against sqd_sgd_clip_step_chunked on
    copies: two steps, the second with lr halved THROUGH THE TABLE ONLY; parameters and momentum bit-equal, and within the existing
    bar L of the float64 step (fp64_ref.clip_sgd)."""
    from squeezedet_pytorch_amd import _native as nat
    lib = nat.lib()
    sizes = LAYOUTS[layout]
    n = sum(sizes)
    offs = np.cumsum([0] + sizes[:-1])
    if layout == 'mixed':
        assert any((4 * o) % 16 for o in offs)
    rs = np.random.RandomState(3)
    mom, wd, lr = 0.9, 1e-4, 0.01
    sides = {}
    for side in ('dev', 'arg'):
        rs2 = np.random.RandomState(4)
        params = [torch.from_numpy((rs2.standard_normal(k) * 0.05).astype(np.float32)).cuda() for k in sizes]
        mflat = torch.zeros(n, device='cuda')
        bufs = [mflat[o:o + k] for o, k in zip(offs, sizes)]
        sides[side] = (params, mflat, bufs) + _chunk_tables(params, bufs)
    hyper = torch.zeros(4, device='cuda')
    parts = {s: torch.zeros(int(lib.sqd_grad_sumsq_parts()), device='cuda') for s in sides}
    norm = {s: torch.zeros(1, device='cuda') for s in sides}
    st = nat.stream_handle('cuda')
    for it in range(2):
        g = (rs.standard_normal(n) * 0.01).astype(np.float32)
        if layout == 'tail_big':
            g[4 * (n >> 2):] = 3.0
        flat = torch.from_numpy(g).cuda()
        max_norm = 0.5 * float(flat.double().norm()) if clip == 'on' else 0.0
        lr_it = lr * 0.5 ** it
        p0 = [p.clone() for p in sides['arg'][0]]
        b0 = [b.clone() for b in sides['arg'][2]]
        g0 = [flat[o:o + k] for o, k in zip(offs, sizes)]
        for side, (params, mflat, bufs, table, chunks) in sides.items():
            pp = None
            if clip == 'on':
                pp = parts[side]
                nat.check(lib.sqd_grad_sumsq(nat.ptr(flat), n, nat.ptr(pp), st), 'sqd_grad_sumsq')
            if side == 'dev':
                nat.check(lib.sqd_fill_f32x4(nat.ptr(hyper), lr_it, mom, wd, max_norm, st), 'sqd_fill_f32x4')
                nat.check(lib.sqd_sgd_clip_step_chunked_dev(nat.ptr(table), nat.ptr(chunks), chunks.shape[0], nat.ptr(flat), nat.ptr(pp),
                                                            nat.ptr(norm[side]), nat.ptr(hyper), st), 'sqd_sgd_clip_step_chunked_dev')
            else:
                nat.check(lib.sqd_sgd_clip_step_chunked(nat.ptr(table), nat.ptr(chunks), chunks.shape[0], nat.ptr(flat), nat.ptr(pp),
                                                        nat.ptr(norm[side]), max_norm, lr_it, mom, wd, st), 'sqd_sgd_clip_step_chunked')
        torch.cuda.synchronize()
        assert hyper.tolist() == [np.float32(v).item() for v in (lr_it, mom, wd, max_norm)]
        for i, (pd, pa) in enumerate(zip(sides['dev'][0], sides['arg'][0])):
            assert bits_equal(pd, pa), f'{layout} clip {clip} step {it}: parameter {i} differs'
        assert bits_equal(sides['dev'][1], sides['arg'][1]), f'{layout} clip {clip} step {it}: momentum differs'
        if clip == 'on':
            assert bits_equal(norm['dev'], norm['arg'])
        tn64, coef, refp, refb = R.clip_sgd(p0, g0, b0, lr_it, mom, wd, max_norm)
        worst = 0.0
        for got_list, refs, what in ((sides['dev'][0], refp, 'p'), (sides['dev'][2], refb, 'buf')):
            for i, (got, r) in enumerate(zip(got_list, refs)):
                err = (got.double().cpu().reshape(r.ref64.shape) - r.ref64).abs()
                pos = r.M > 0
                if bool(pos.any()):
                    worst = max(worst, float((err[pos] / r.M[pos]).max()))
                assert bool((err <= R.BAR_L * r.M).all()), f'{layout} clip {clip} step {it}: {what} {i} outside bar L'
        print(f'dev kernel {layout:8s} clip {clip:3s} step {it} lr {lr_it:g} coef {coef:.4f}: max err/M {worst:.2e} (bar {R.BAR_L:.2e})')


# ---- 2. replayed against eager ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form,B', [('dense', 2), ('sparse', 3), ('masked', 3)])
def test_replay_equals_eager(form, B):
    cfg = make_cfg(sparse_gt=form != 'dense', ignore_overlap=0.5 if form == 'masked' else None)
    batches = [make_batch(cfg, form, B, seed=20 + i, empty_image=(1 if i == 2 else None)) for i in range(6)]
    if form != 'dense':
        totals = [int(b['gt_sparse'].anchor_idx.shape[0]) for b in batches]
        assert len(set(totals)) > 1 and max(totals) <= 64, totals          # the per-batch total varies, inside the first capacity
    if form == 'masked':
        off = batches[2]['gt_sparse'].offsets.tolist()
        assert off[2] == off[1], 'batch 2 has no object-free image'
    g, e = run_pair(cfg, batches)
    assert g.gs.captures == 1 and g.gs.replays == 5 and g.gs.eager_steps == 1
    # p.grad: views of one flat buffer, this step's unclipped gradients
    torch.cuda.synchronize()
    for pg, pe in zip(g.opt.params, e.opt.params):
        assert bits_equal(pg.grad, pe.grad)
    assert g.opt._flat_base([p.grad for p in g.opt.params]) is not None


# ---- 3. a learning-rate schedule without re-capture ---------------------------------------------------------------------------------

@pytest.mark.filterwarnings('ignore:Detected call of `lr_scheduler.step')      # (a replay runs no Python optimizer.step for torch to count)
def test_lr_schedule_without_recapture():
    cfg = make_cfg()
    batches = [make_batch(cfg, 'dense', 2, seed=40 + i) for i in range(6)]
    scheds = {}

    def after(i, g, e):
        if not scheds:
            scheds['g'] = torch.optim.lr_scheduler.StepLR(g.opt, 1, 0.5)
            scheds['e'] = torch.optim.lr_scheduler.StepLR(e.opt, 1, 0.5)
        scheds['g'].step(); scheds['e'].step()
    g, e = run_pair(cfg, batches, after_step=after, lr=0.004)
    assert g.gs.captures == 1 and g.gs.replays == 5
    assert g.opt.lr == 0.004 / 64 and e.opt.lr == 0.004 / 64
    torch.cuda.synchronize()
    assert g.opt._hyper_dev.tolist()[0] == np.float32(0.004 / 32).item()       # the table holds the rate of the last step taken


# ---- 4. capacity growth -------------------------------------------------------------------------------------------------------------

def test_sparse_capacity_growth_recaptures():
    cfg = make_cfg(sparse_gt=True)
    small = lambda s: make_batch(cfg, 'sparse', 3, seed=s)
    big = lambda s: make_batch(cfg, 'sparse', 3, seed=s, boxes=(30, 30))
    batches = [small(60), small(61), small(62), big(63), small(64), big(65)]
    assert int(batches[3]['gt_sparse'].anchor_idx.shape[0]) == 90 > 64
    seen = []
    g, e = run_pair(cfg, batches, after_step=lambda i, g, e: seen.append((g.gs.captures, dict(g.gs._cap))))
    assert [c for c, _ in seen] == [0, 1, 1, 2, 2, 2], seen
    assert list(seen[2][1].values()) == [64] and list(seen[3][1].values()) == [128]
    assert g.gs.eager_steps == 1 and g.gs.replays == 5


# ---- 5. no stale packed weights -----------------------------------------------------------------------------------------------------

def test_no_stale_packed_weights_after_replays():
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet, SqueezeDetWithLoss
    cfg = make_cfg(score_thresh=0.02)
    torch.manual_seed(5)
    g = Graphed(cfg)
    probe = make_batch(cfg, 'dense', 2, seed=70)
    shared = SqueezeDet(cfg)
    shared.base = g.model.base                       # a Detector on the SAME parameters (and packed-weight caches)
    det = Detector(shared, cfg)

    def eval_outputs(train_model, detector):
        train_model.eval()
        with torch.no_grad():
            loss, stats = train_model(probe)
            cnt, cls, sc, bx, idx = detector.detect_device(probe['image'])
        res = detector.detect({'image': probe['image']})
        train_model.train()
        return [loss.clone()] + [stats[k].clone() for k in KEYS] + [cnt.clone(), cls.clone(), sc.clone(), bx.clone(), idx.clone()], res
    def check_against_fresh(tag, previous):
        """The shared model and Detector, as they are now, against fresh ones loaded from the state_dict.  An eval brings every
        packed copy up to date with the counters: only a replay that advances them makes the NEXT eval re-pack."""
        got, got_res = eval_outputs(g.model, det)
        sd = {k: v.detach().clone() for k, v in g.model.state_dict().items()}
        fresh = SqueezeDetWithLoss(cfg)
        fresh.load_state_dict(sd)
        fresh = fresh.cuda()
        fresh_inf = SqueezeDet(cfg)
        fresh_inf.load_state_dict(sd)
        want, want_res = eval_outputs(fresh, Detector(fresh_inf, cfg))
        assert not bits_equal(want[0], previous[0]), f'{tag}: training did not change the eval loss: the probe shows nothing'
        for i, (a, b) in enumerate(zip(got, want)):
            assert bits_equal(a, b), f'{tag}: eval output {i} differs from a fresh model with the same state_dict (stale packed weights)'
        assert int(want[5].sum()) > 0, f'{tag}: no detection at all: the Detector comparison shows nothing'
        assert len(got_res) == len(want_res)
        for a, b in zip(got_res, want_res):
            assert set(a) == set(b)
            for k in ('class_ids', 'scores', 'boxes', 'anchor_idx'):
                if k in a:
                    assert np.array_equal(a[k], b[k]), (tag, k)
        return want
    before, _ = eval_outputs(g.model, det)           # fills every inference-side plan with the INITIAL weights
    for i in range(3):                               # one eager step, then two replays
        g.step(make_batch(cfg, 'dense', 2, seed=71 + i))
    assert g.gs.replays == 2 and g.gs.captures == 1
    mid = check_against_fresh('after replay 2', before)          # (leaves every copy fresh at the current counters)
    for i in range(3, 5):                            # two more replays: the weights move again, only the post-replay advance says so
        g.step(make_batch(cfg, 'dense', 2, seed=71 + i))
    assert g.gs.replays == 4 and g.gs.captures == 1 and g.gs.eager_steps == 1
    check_against_fresh('after replay 4', mid)


def test_eval_between_steps_keeps_the_replays_right():
    """An eval forward between the eager first step and the capture brings the packed copies up to date, so the captured forward would
    hold no re-pack launch and every replay would compute with the weights of the capture; evals between replays make the copies
    fresh at the counters the next replay has to move.  Evals after steps 0, 2, 3 and 4 of six -- none after step 1, so that the
    replay of step 2 has nothing but the captured re-pack to give it step 1's weights: the graph side still equals the eager twin bit
    for bit, in the training state after each step and in the eval outputs themselves."""
    cfg = make_cfg()
    probe = make_batch(cfg, 'dense', 2, seed=90)
    batches = [make_batch(cfg, 'dense', 2, seed=91 + i) for i in range(6)]

    def eval_loss(model):
        model.eval()
        with torch.no_grad():
            loss, stats = model(probe)
        model.train()
        return [loss.clone()] + [stats[k].clone() for k in KEYS]
    seen = []

    def after(i, g, e):
        if i not in (0, 2, 3, 4):
            return
        a, b = eval_loss(g.model), eval_loss(e.model)
        for j, (x, y) in enumerate(zip(a, b)):
            assert bits_equal(x, y), f'eval after step {i}: output {j} of the graph side differs from the eager twin (stale packed weights)'
        if seen:
            assert not bits_equal(a[0], seen[-1]), f'eval after step {i}: the eval loss did not move'
        seen.append(a[0])
    g, e = run_pair(cfg, batches, after_step=after)
    assert g.gs.captures == 1 and g.gs.replays == 5 and g.gs.eager_steps == 1 and len(seen) == 4


def test_larger_batch_takes_over():
    """The graphs are made for the largest batch size seen: a run whose FIRST batch is the odd, smaller one still captures the full
    size (2, then 3, 3, 3: eager, eager first step, capture, replay), and a smaller batch afterwards runs eagerly."""
    cfg = make_cfg()
    sizes = [2, 3, 3, 3, 2]
    batches = [make_batch(cfg, 'dense', B, seed=95 + i) for i, B in enumerate(sizes)]
    g, e = run_pair(cfg, batches)
    assert g.gs.batch_size == 3 and g.gs.captures == 1 and g.gs.replays == 2 and g.gs.eager_steps == 3


# ---- 6. the device log --------------------------------------------------------------------------------------------------------------

def test_device_log():
    from squeezedet_pytorch_amd.trainer import LOG_ROWS
    cfg = make_cfg()
    torch.manual_seed(6)
    g = Graphed(cfg)
    B = 3
    sums = {k: 0.0 for k in KEYS}
    means = []
    for i in range(5):
        _, stats = g.step(make_batch(cfg, 'dense', B, seed=80 + i))
        step = {}
        for k in KEYS:
            acc = 0.0
            for v in stats[k].tolist():                  # fp32 values, added in index order in float64
                acc += v
            step[k] = acc
            sums[k] += acc
        means.append(step)
    got, latest, n = g.gs.read_log()
    assert n == 5 and got['images'] == 5.0 * B
    for k in KEYS:
        assert np.isfinite(sums[k]) and abs(got[k] - sums[k]) <= 1e-12 * abs(sums[k]), (k, got[k], sums[k])
    ring = g.gs._log_ring.cpu().numpy()
    for i, step in enumerate(means):
        for j, k in enumerate(LOG_ROWS):
            assert ring[i, j] == np.float32(step[k] / B), (i, k, ring[i, j], step[k] / B)
    assert latest == {k: float(np.float32(means[-1][k] / B)) for k in KEYS}
    g.gs.reset_log()
    got2, latest2, n2 = g.gs.read_log()
    assert n2 == 5 and latest2 == latest and all(got2[k] == 0.0 for k in KEYS) and got2['images'] == 0.0


# ---- 7. through Trainer -------------------------------------------------------------------------------------------------------------

def _trainer(cfg, state_dict=None):
    from squeezedet_pytorch_amd.trainer import Trainer
    m = make_model(cfg, state_dict)
    opt = make_opt(m, max_norm=cfg.grad_norm)
    return Trainer(m, opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)


def _host_batches(cfg, sizes, seed):
    from squeezedet_pytorch_amd import synthetic
    return [{'image': synthetic.make_images(B, SIZE, seed=seed + i),
             'gt': synthetic.make_gt(B, cfg.anchors, SIZE, C, seed=seed + 50 + i), 'image_meta': {}} for i, B in enumerate(sizes)]


def _trainer_cfg(graph_step):
    cfg = make_cfg(graph_step=graph_step, lr=LR)
    cfg.num_iters, cfg.print_interval, cfg.grad_norm, cfg.gpus, cfg.chunk_sizes = -1, 2, 5.0, [0], [3]
    return cfg


def test_trainer_graph_step_equals_eager(capsys):
    loader = None
    runs = {}
    for flag in (True, False):
        torch.manual_seed(9)
        cfg = _trainer_cfg(flag)
        if loader is None:
            loader = _host_batches(cfg, [3, 3, 3, 3, 2], seed=200)
        tr = _trainer(cfg)
        per_image = []
        if not flag:
            inner = tr.model.forward_mean

            def recording(batch, _f=inner):
                mean, stats = _f(batch)
                per_image.append({k: stats[k].detach().clone() for k in KEYS})
                return mean, stats
            tr.model.forward_mean = recording
        out = tr.train_epoch(1, loader)
        if not flag:
            del tr.model.forward_mean
        val = tr.val_epoch(1, loader[:2])
        runs[flag] = (tr, out, val, per_image)
    on, off = runs[True], runs[False]
    gs = on[0].graphed_step()
    assert gs.captures == 1 and gs.replays == 3 and gs.eager_steps == 2            # first step, three replays, the ragged last batch
    torch.cuda.synchronize()
    for (n, pa), (_, pb) in zip(on[0].model.named_parameters(), off[0].model.named_parameters()):
        assert bits_equal(pa, pb), f'parameter {n} differs between graph_step on and off'
    assert bits_equal(on[0].optimizer.momentum_flat, off[0].optimizer.momentum_flat)
    images = sum(v['loss'].shape[0] for v in off[3])
    assert images == 14
    for k in KEYS:
        want = sum(float(x) for v in off[3] for x in v[k].tolist()) / images
        assert abs(on[1][k] - want) <= 1e-12 * abs(want), (k, on[1][k], want)
        assert on[2][k] == off[2][k], (k, on[2][k], off[2][k])
    text = capsys.readouterr().out
    lines = [l for l in text.splitlines() if l.startswith('epoch 1: train')]
    assert len(lines) == 6 and all('| loss ' in l and '| data ' in l and '| net ' in l for l in lines), text      # 3 per run (it = 0, 2, 4)


def test_checkpoint_resume_under_graph_step(tmp_path):
    from squeezedet_pytorch_amd.checkpoint import load_checkpoint, save_checkpoint
    cfg = make_cfg()
    batches = [make_batch(cfg, 'dense', 2, seed=300 + i) for i in range(6)]
    torch.manual_seed(13)
    straight = Graphed(cfg)
    for b in batches:
        straight.step(b)
    torch.manual_seed(13)
    first = Graphed(cfg)
    sched = torch.optim.lr_scheduler.StepLR(first.opt, 60, gamma=0.5)
    for b in batches[:3]:
        first.step(b)
    path = str(tmp_path / 'ckpt.pth')
    save_checkpoint(path, first.model, first.opt, sched, epoch=1)
    torch.manual_seed(99)                                   # the resumed process has other streams until the file restores them
    resumed = Graphed(cfg, state_dict={k: torch.zeros_like(v) for k, v in first.model.state_dict().items()})
    sched2 = torch.optim.lr_scheduler.StepLR(resumed.opt, 60, gamma=0.5)
    assert load_checkpoint(path, resumed.model, resumed.opt, sched2) == 1
    resumed.model.train()
    for b in batches[3:]:
        resumed.step(b)
    assert resumed.gs.eager_steps == 1 and resumed.gs.captures == 1 and resumed.gs.replays == 2
    assert_same_state(resumed, straight, 'resumed 3 + 3 against 6 straight')


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals():
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, GraphedStep, Trainer
    cfg = _trainer_cfg(True)
    m = make_model(cfg)
    sgd = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    with pytest.raises(ValueError, match='FusedClipSGD.*SGD'):
        Trainer(m, sgd, torch.optim.lr_scheduler.StepLR(sgd, 60, gamma=0.5), cfg)
    with pytest.raises(ValueError, match='FusedClipSGD.*SGD'):
        GraphedStep(m, sgd, cfg)
    with pytest.raises(ValueError, match='forward_mean'):
        GraphedStep(m.base, make_opt(m), cfg)

    class NoLoss(torch.nn.Module):                   # forward_mean, but no model.Loss whose weights could be watched
        def __init__(self, base):
            super().__init__()
            self.base = base

        def forward_mean(self, batch):
            raise AssertionError('never called')
    opt_ok = make_opt(m)
    with pytest.raises(ValueError, match='Loss'):
        GraphedStep(NoLoss(m.base), opt_ok, cfg)
    assert opt_ok.hyper_on_device is False           # a refusal leaves the optimizer as it was
    # Trainer: the captured step clips inside the optimizer launch, the eager loop would clip with a torch call it lacks
    opt0 = make_opt(m, max_norm=0.0)
    with pytest.raises(ValueError, match='max_norm'):
        Trainer(m, opt0, torch.optim.lr_scheduler.StepLR(opt0, 60, gamma=0.5), cfg)
    assert opt0.hyper_on_device is False
    # release() gives the optimizer back what construction changed
    gs = GraphedStep(m, opt_ok, cfg)
    assert opt_ok.hyper_on_device is True
    gs.release()
    assert opt_ok.hyper_on_device is False
    # hyper_on_device needs the flat layout
    params = [torch.nn.Parameter(torch.randn(10, device='cuda')) for _ in range(3)]
    opt = FusedClipSGD(params, lr=0.01, momentum=0.9, max_norm=1.0)
    opt.hyper_on_device = True
    for p in params:
        p.grad = torch.randn(10, device='cuda')
    before = [p.detach().clone() for p in params]
    with pytest.raises(RuntimeError, match='flat-gradient layout'):
        opt.step()
    torch.cuda.synchronize()
    assert all(bits_equal(p, b) for p, b in zip(params, before)), 'a refused step changed the parameters'
