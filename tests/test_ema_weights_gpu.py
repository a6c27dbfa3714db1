"""GPU tier: the averaged weights of the fused optimizers (``optimizer.averaged_weights()``, ``ema_state_dict``, ``cfg.ema_eval``).

Inside ``averaged_weights()`` an eval forward and ``Detector.detect`` on the training model's own parameters (and packed-weight caches)
must equal, bit for bit, those of a fresh model loaded from ``ema_state_dict``; after leaving, the parameters are bit-identical to before
and both the eval outputs and a training forward equal the ones taken before entry -- no stale packed copy survives in either direction.
Shapes: those of tests/test_graph_step_gpu.py (64x96, 3 classes, 2 images), dropout off so that two training forwards are comparable."""
import numpy as np
import pytest
import torch

import test_graph_step_gpu as G
from test_graph_step_gpu import bits_equal

pytestmark = pytest.mark.gpu


def _adamw(model, ema_decay=0.9, **kw):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, find_base
    base = find_base(model)
    return FusedClipAdamW([p for p in model.parameters() if p.requires_grad], lr=1e-4, weight_decay=1e-2, max_norm=5.0, ema_decay=ema_decay,
                          flat_grad=lambda: base.last_grad_flat, **kw)


def _train(model, opt, cfg, steps, seed):
    one = torch.ones((), device='cuda')
    for i in range(steps):
        mean, _ = model.forward_mean(G.make_batch(cfg, 'dense', 2, seed=seed + i))
        opt.zero_grad()
        mean.backward(one)
        opt.step()


def _eval_outputs(train_model, detector, probe):
    train_model.eval()
    with torch.no_grad():
        loss, stats = train_model(probe)
        cnt, cls, sc, bx, idx = detector.detect_device(probe['image'])
    res = detector.detect({'image': probe['image']})
    train_model.train()
    return [loss.clone()] + [stats[k].clone() for k in G.KEYS] + [cnt.clone(), cls.clone(), sc.clone(), bx.clone(), idx.clone()], res


def _same(got, want, tag):
    (a, ares), (b, bres) = got, want
    for i, (x, y) in enumerate(zip(a, b)):
        assert bits_equal(x, y), f'{tag}: eval output {i} differs'
    assert len(ares) == len(bres)
    for x, y in zip(ares, bres):
        assert set(x) == set(y)
        for k in ('class_ids', 'scores', 'boxes', 'anchor_idx'):
            if k in x:
                assert np.array_equal(x[k], y[k]), (tag, k)


def test_averaged_weights_equal_a_fresh_model_and_leave_no_trace():
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet, SqueezeDetWithLoss
    cfg = G.make_cfg(score_thresh=0.02, dropout_prob=0.0)
    torch.manual_seed(5)
    model = G.make_model(cfg)
    opt = _adamw(model)
    probe = G.make_batch(cfg, 'dense', 2, seed=70)
    shared = SqueezeDet(cfg)
    shared.base = model.base                         # a Detector on the SAME parameters (and packed-weight caches)
    det = Detector(shared, cfg)
    _train(model, opt, cfg, 3, seed=71)
    before = _eval_outputs(model, det, probe)        # every inference-side plan now holds the TRAINING weights
    train_before = [t.detach().clone() for t in (lambda m, s: [m] + [s[k] for k in G.KEYS])(*model.forward_mean(probe))]
    p_before = [p.detach().clone() for p in opt.params]
    e_before = opt.ema_flat.clone()
    sd = opt.ema_state_dict(model)
    fresh = SqueezeDetWithLoss(cfg)
    fresh.load_state_dict(sd)
    fresh = fresh.cuda()
    fresh_inf = SqueezeDet(cfg)
    fresh_inf.load_state_dict(sd)
    want = _eval_outputs(fresh, Detector(fresh_inf, cfg), probe)
    assert not bits_equal(want[0][0], before[0][0]), 'the averaged model evaluates like the training weights: the probe shows nothing'
    assert int(want[0][5].sum()) > 0, 'no detection at all: the Detector comparison shows nothing'
    versions = [p._version for p in opt.params]
    with opt.averaged_weights():
        assert all(p._version > v for p, v in zip(opt.params, versions))
        for p, e in zip(opt.params, opt._emas):
            assert bits_equal(p.detach().reshape(-1), e_before[e.storage_offset():e.storage_offset() + e.numel()])
        _same(_eval_outputs(model, det, probe), want, 'inside averaged_weights')
        assert {k: v.shape for k, v in model.state_dict().items()} == {k: v.shape for k, v in sd.items()}
        for k, v in model.state_dict().items():
            assert bits_equal(v, sd[k]), f'state_dict inside averaged_weights: {k} differs from ema_state_dict'
    torch.cuda.synchronize()
    for p, q in zip(opt.params, p_before):
        assert bits_equal(p, q), 'a parameter changed across averaged_weights()'
    assert bits_equal(opt.ema_flat, e_before)
    _same(_eval_outputs(model, det, probe), before, 'after averaged_weights')
    mean, stats = model.forward_mean(probe)
    for a, b in zip([mean] + [stats[k] for k in G.KEYS], train_before):
        assert bits_equal(a, b), 'the training forward after averaged_weights() differs from the one before (stale packed weights)'
    _train(model, opt, cfg, 1, seed=80)              # and training goes on
    assert opt.step_counts() == (4, 4)


def test_refusals():
    cfg = G.make_cfg(dropout_prob=0.0)
    model = G.make_model(cfg)
    opt = _adamw(model)
    with opt.averaged_weights():
        with pytest.raises(RuntimeError, match='nested'):
            with opt.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match='averaged_weights'):
            opt.step()
        with pytest.raises(RuntimeError, match='averaged_weights'):
            opt.ema_state_dict(model)
    off = _adamw(model, ema_decay=0.0)
    with pytest.raises(RuntimeError, match='EMA is off'):
        with off.averaged_weights():
            pass
    with pytest.raises(RuntimeError, match='EMA is off'):
        off.ema_state_dict(model)
    # under stream capture
    before = [p.detach().clone() for p in opt.params]
    x = torch.zeros(4, device='cuda')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        x.add_(1.0)
        with pytest.raises(RuntimeError, match='stream capture'):
            with opt.averaged_weights():
                pass
    torch.cuda.synchronize()
    assert opt._averaging is False and all(bits_equal(p, q) for p, q in zip(opt.params, before))
    # the launch-argument path of SGD has no EMA
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    params = [torch.nn.Parameter(torch.randn(10, device='cuda')) for _ in range(3)]
    sgd = FusedClipSGD(params, lr=0.01, momentum=0.9, ema_decay=0.99)
    for p in params:
        p.grad = torch.randn(10, device='cuda')
    with pytest.raises(RuntimeError, match='launch-argument path'):
        sgd.step()


def test_make_train_step_follows_cfg_optimizer():
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, FusedClipSGD, make_train_step
    sd = synthetic.make_state_dict('squeezedet', seed=1234, num_classes=G.C)
    x = synthetic.make_images(2, G.SIZE, seed=0).cuda()
    for kw, cls, ema in ((dict(lr=1e-3), FusedClipSGD, False), (dict(optimizer='adamw', ema_decay=0.99, ema_warmup=True, lr=1e-4), FusedClipAdamW, True),
                         (dict(ema_decay=0.99, lr=1e-3), FusedClipSGD, True)):
        torch.manual_seed(0)
        cfg = G.make_cfg(**kw)
        parts = {}
        step, desc, _ = make_train_step(cfg, sd, x, 0, 1, None, parts=parts)
        opt = parts['optimizer']
        assert type(opt) is cls and opt.ema_on is ema and opt.max_norm == cfg.grad_norm and opt.ema_warmup is bool(kw.get('ema_warmup', False))
        assert ('AdamW' in desc) == (cls is FusedClipAdamW) and ('EMA' in desc) == ema
        losses = [float(step()) for _ in range(3)]
        assert all(np.isfinite(v) for v in losses), losses
        assert opt.step_counts() == ((3 if cls is FusedClipAdamW else 0), (3 if ema else 0))
    with pytest.raises(ValueError, match='cfg.optimizer'):
        make_train_step(G.make_cfg(optimizer='lamb'), sd, x, 0, 1, None)


def test_trainer_val_epoch_under_ema_eval():
    from squeezedet_pytorch_amd.trainer import Trainer
    runs = {}
    loader = None
    for flag in (True, False):
        torch.manual_seed(9)
        cfg = G._trainer_cfg(False)
        cfg.ema_eval = flag
        if loader is None:
            loader = G._host_batches(cfg, [3, 3, 3], seed=200)
        m = G.make_model(cfg)
        opt = _adamw(m)
        tr = Trainer(m, opt, torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5), cfg)
        tr.train_epoch(1, loader)
        runs[flag] = (tr, tr.val_epoch(1, loader[:2]))
    on, off = runs[True], runs[False]
    for (n, pa), (_, pb) in zip(on[0].model.named_parameters(), off[0].model.named_parameters()):
        assert bits_equal(pa, pb), f'parameter {n}: ema_eval changed the training'
    # the averaged model, evaluated by a plain Trainer
    cfg = G._trainer_cfg(False)
    avg = G.make_model(cfg, off[0].optimizer.ema_state_dict(off[0].model))
    sgd = G.make_opt(avg)
    want = Trainer(avg, sgd, torch.optim.lr_scheduler.StepLR(sgd, 60, gamma=0.5), cfg).val_epoch(1, loader[:2])
    for k in G.KEYS:
        assert on[1][k] == want[k], (k, on[1][k], want[k])
        assert np.isfinite(want[k])
    assert on[1]['loss'] != off[1]['loss'], 'the averaged weights evaluate like the training weights: the test shows nothing'
    sgd_plain = G.make_opt(G.make_model(cfg))
    cfg.ema_eval = True
    with pytest.raises(ValueError, match='ema_eval'):
        Trainer(avg, sgd_plain, torch.optim.lr_scheduler.StepLR(sgd_plain, 60, gamma=0.5), cfg).val_epoch(1, loader[:1])
