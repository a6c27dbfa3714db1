"""GPU tier: the captured training step (trainer.GraphedStep) with the fused AdamW + EMA and with SGD + EMA, on the helpers and sizes of
tests/test_graph_step_gpu.py.

A replayed step must equal the all-eager loop BIT FOR BIT -- parameters, both moments (or the momentum), the EMA, the loss vectors, the
gradient norm, and the device counts t / n -- over six steps with a StepLR change half-way and ONE capture; a run resumed from a
checkpoint written after step 3 (fresh model, optimizer and scheduler objects) must equal the uninterrupted run, eager and graphed."""
import pytest
import torch

import test_graph_step_gpu as G
from test_graph_step_gpu import bits_equal

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('ignore:Detected call of `lr_scheduler.step')]

LR = {'adamw': 1e-4, 'sgd': G.LR}
STATE = {'adamw': ('exp_avg_flat', 'exp_avg_sq_flat', 'ema_flat'), 'sgd': ('momentum_flat', 'ema_flat')}


def make_opt(model, kind):
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, FusedClipSGD, find_base
    base = find_base(model)
    params = [p for p in model.parameters() if p.requires_grad]
    if kind == 'adamw':
        return FusedClipAdamW(params, lr=LR[kind], weight_decay=1e-2, max_norm=5.0, ema_decay=0.999, ema_warmup=True,
                              flat_grad=lambda: base.last_grad_flat)
    return FusedClipSGD(params, lr=LR[kind], momentum=0.9, weight_decay=1e-4, max_norm=5.0, ema_decay=0.999,
                        flat_grad=lambda: base.last_grad_flat)


class Side:
    """A model, its optimizer and scheduler; the step eager or through a GraphedStep."""

    def __init__(self, cfg, kind, graphed, state_dict=None):
        from squeezedet_pytorch_amd.trainer import GraphedStep
        self.model = G.make_model(cfg, state_dict)
        self.opt = make_opt(self.model, kind)
        self.sched = torch.optim.lr_scheduler.StepLR(self.opt, 3, 0.5)
        self.gs = GraphedStep(self.model, self.opt, cfg) if graphed else None
        self.one = torch.ones((), device='cuda')

    def step(self, batch):
        if self.gs is not None:
            out = self.gs.step(batch)
        else:
            mean, stats = self.model.forward_mean(batch)
            self.opt.zero_grad()
            mean.backward(self.one)
            self.opt.step()
            out = mean.detach(), {k: v.detach() for k, v in stats.items()}
        self.sched.step()
        return out


def assert_same(a, b, kind, tag, out_a=None, out_b=None):
    torch.cuda.synchronize()
    if out_a is not None:
        assert bool(torch.isfinite(out_b[0])), f'{tag}: the loss is not finite'
        assert bits_equal(out_a[0], out_b[0]), f'{tag}: mean loss differs: {float(out_a[0])!r} vs {float(out_b[0])!r}'
        for k in G.KEYS:
            assert bits_equal(out_a[1][k], out_b[1][k]), f'{tag}: per-image {k} differs'
        assert bits_equal(a.opt.last_norm, b.opt.last_norm), f'{tag}: norm {float(a.opt.last_norm)!r} vs {float(b.opt.last_norm)!r}'
    for (n, pa), (_, pb) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert bits_equal(pa, pb), f'{tag}: parameter {n} differs (max abs {float((pa - pb).abs().max()):.3e})'
    for name in STATE[kind]:
        sa, sb = getattr(a.opt, name), getattr(b.opt, name)
        assert bool(torch.isfinite(sb).all()), f'{tag}: {name} is not finite'
        assert bits_equal(sa, sb), f'{tag}: {name} differs (max abs {float((sa - sb).abs().max()):.3e})'
    assert a.opt.step_counts() == b.opt.step_counts(), f'{tag}: counts {a.opt.step_counts()} vs {b.opt.step_counts()}'
    assert a.opt.lr == b.opt.lr


@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_replay_equals_eager(kind):
    cfg = G.make_cfg()
    batches = [G.make_batch(cfg, 'dense', 2, seed=400 + i) for i in range(6)]
    torch.manual_seed(11)
    g, e = Side(cfg, kind, True), Side(cfg, kind, False)
    p_start = [p.detach().clone() for p in e.opt.params]
    for i, b in enumerate(batches):
        out_g, out_e = g.step(b), e.step(b)
        assert_same(g, e, kind, f'{kind} step {i}', out_g, out_e)
    assert g.gs.captures == 1 and g.gs.replays == 5 and g.gs.eager_steps == 1       # the lr halved after step 3: no re-capture
    assert e.opt.lr == LR[kind] / 4 and g.opt.lr == LR[kind] / 4
    assert e.opt.step_counts() == ((6 if kind == 'adamw' else 0), 6)
    torch.cuda.synchronize()
    assert g.opt._hyper_dev.tolist()[0] == torch.tensor(LR[kind] / 2, dtype=torch.float32).item()      # the rate of the last step taken
    # the average moved, and differs from the weights
    assert not any(bits_equal(a, p.detach().reshape(-1)) for a, p in zip(e.opt._emas, e.opt.params) if p.numel() > 64)
    assert not any(bits_equal(a, p.reshape(-1)) for a, p in zip(e.opt._emas, p_start) if p.numel() > 64)


@pytest.mark.parametrize('graphed', [False, True], ids=['eager', 'graphed'])
@pytest.mark.parametrize('kind', ['adamw', 'sgd'])
def test_checkpoint_resume(tmp_path, kind, graphed):
    from squeezedet_pytorch_amd.checkpoint import load_checkpoint, save_checkpoint
    cfg = G.make_cfg()
    batches = [G.make_batch(cfg, 'dense', 2, seed=500 + i) for i in range(6)]
    torch.manual_seed(13)
    straight = Side(cfg, kind, graphed)
    for b in batches:
        straight.step(b)
    torch.manual_seed(13)
    first = Side(cfg, kind, graphed)
    for b in batches[:3]:
        first.step(b)
    path = str(tmp_path / 'ckpt.pth')
    save_checkpoint(path, first.model, first.opt, first.sched, epoch=1)
    torch.manual_seed(99)                                   # the resumed process has other streams until the file restores them
    resumed = Side(cfg, kind, graphed, state_dict={k: torch.zeros_like(v) for k, v in first.model.state_dict().items()})
    assert load_checkpoint(path, resumed.model, resumed.opt, resumed.sched) == 1
    assert resumed.opt.step_counts() == ((3 if kind == 'adamw' else 0), 3) and resumed.opt.lr == LR[kind] / 2
    assert_same(resumed, first, kind, 'loaded against saved')
    resumed.model.train()
    for b in batches[3:]:
        resumed.step(b)
    if graphed:
        assert resumed.gs.eager_steps == 1 and resumed.gs.captures == 1 and resumed.gs.replays == 2
    assert_same(resumed, straight, kind, f'{kind} resumed 3 + 3 against 6 straight')
