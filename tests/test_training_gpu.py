"""GPU tier, training rows (SURVEY.md section 8a rows L, M, N and the backward of A-G): loss forward /
analytic backward, weight gradients, the full backward chain and one optimiser step against the
oracle (CPU autograd over the restated forward) and the reference's golden vectors."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import synthetic

pytestmark = pytest.mark.gpu


def _rand(*shape, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _decode_pred():
    rs = np.random.RandomState(11)
    return torch.from_numpy((rs.standard_normal((2, 16848, 8)) * np.array([2, 2, 2, 2, .4, .4, .4, .4])).astype(np.float32))


def _loss_gt(golden_dir, cfg):
    g = np.load(os.path.join(golden_dir, "loss.npz"))
    gts = [oracle.encode_gt(g[f"gtcls{b}"], g[f"gtboxes{b}"], cfg.anchors) for b in range(2)]
    return g, torch.from_numpy(np.stack(gts))


def test_loss_fwd_bwd_vs_golden_and_oracle(golden_dir):
    from squeezedet_pytorch_amd.model import Loss
    cfg = sqd.make_cfg()
    g, gt = _loss_gt(golden_dir, cfg)
    pred = _decode_pred().cuda().requires_grad_(True)
    loss_mod = Loss(cfg)
    loss, stats = loss_mod(pred, gt.cuda())
    np.testing.assert_allclose(loss.detach().cpu().numpy(), g["loss"], rtol=1e-5)
    for k in ("class_loss", "score_loss", "bbox_loss"):
        np.testing.assert_allclose(stats[k].detach().cpu().numpy(), g[k], rtol=1e-5)
    loss.mean().backward()
    gr = pred.grad.cpu().numpy()
    # oracle: full dense gradient through CPU autograd (includes the un-detached IoU path)
    po = _decode_pred().requires_grad_(True)
    lo, _ = oracle.multitask_loss(po, gt, cfg.anchors, cfg.input_size)
    lo.mean().backward()
    ref = po.grad.numpy()
    np.testing.assert_allclose(gr, ref, rtol=2e-4, atol=1e-8)
    # and the reference's own rows
    for b in range(2):
        pos = np.nonzero(gt[b, :, 0].numpy())[0]
        np.testing.assert_allclose(gr[b][pos], g[f"grad_pos{b}"], rtol=2e-4, atol=1e-7)
        assert np.abs(gr[b][pos][:, 6:]).max() > 0          # IoU path reaches dw, dh
    np.testing.assert_allclose(gr[:, g["neg"]], g["grad_neg"], rtol=2e-4, atol=1e-9)


def test_loss_component_gradients():
    """Gradients of the individual stats (not only `loss`) flow correctly."""
    from squeezedet_pytorch_amd.model import Loss
    cfg = sqd.make_cfg(input_size=(64, 96))
    gt = synthetic.make_gt(2, cfg.anchors, (64, 96), seed=2, min_boxes=2, max_boxes=3)
    pred0 = _rand(2, cfg.num_anchors, 8, seed=3)
    for key in ("class_loss", "score_loss", "bbox_loss"):
        p = pred0.clone().cuda().requires_grad_(True)
        _, st = Loss(cfg)(p, gt.cuda())
        st[key].sum().backward()
        po = pred0.clone().requires_grad_(True)
        _, so = oracle.multitask_loss(po, gt, cfg.anchors, cfg.input_size)
        so[key].sum().backward()
        np.testing.assert_allclose(p.grad.cpu().numpy(), po.grad.numpy(), rtol=2e-4, atol=1e-7)


@pytest.mark.parametrize("taps,C,N,B,H,W", [
    (1, 64, 16, 2, 12, 20), (1, 16, 64, 2, 12, 20), (1, 768, 96, 1, 6, 10), (1, 96, 384, 1, 5, 9), (1, 48, 192, 1, 7, 11),
    (9, 16, 64, 2, 12, 20), (9, 96, 384, 1, 5, 17), (9, 768, 72, 1, 6, 18), (9, 32, 128, 1, 9, 33),
])
def test_conv_wgrad(taps, C, N, B, H, W):
    from squeezedet_pytorch_amd import ops
    k = 3 if taps == 9 else 1
    x = _rand(B, C, H, W, seed=1)
    w = _rand(N, C, k, k, seed=2, scale=0.1).requires_grad_(True)
    b = _rand(N, seed=3).requires_grad_(True)
    y = F.conv2d(x, w, b, padding=k // 2)
    dy = _rand(B, N, H, W, seed=4)
    y.backward(dy)
    # embed operands in wider buffers to exercise the channel windows
    dyb = torch.zeros(B, H, W, N + 8); dyb[..., 4:4 + N] = _nhwc(dy)
    xb = torch.zeros(B, H, W, C + 4); xb[..., 4:] = _nhwc(x)
    dw, db = ops.conv_wgrad(dyb.cuda(), 4, N, xb.cuda(), 4, C, taps)
    tol = 1e-4 * max(1.0, float(w.grad.abs().max()))
    assert (dw.cpu() - w.grad).abs().max().item() <= tol
    assert (db.cpu() - b.grad).abs().max().item() <= 1e-4 * max(1.0, float(b.grad.abs().max()))
    # deterministic: a second run is bitwise identical (slab reduction, no atomics)
    dw2, db2 = ops.conv_wgrad(dyb.cuda(), 4, N, xb.cuda(), 4, C, taps)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize("k,N,H,W", [(3, 64, 64, 96), (3, 64, 33, 47), (7, 96, 64, 96)])
def test_stem_wgrad(k, N, H, W):
    from squeezedet_pytorch_amd import ops
    x = _rand(2, 3, H, W, seed=11)
    w = _rand(N, 3, k, k, seed=12, scale=0.2).requires_grad_(True)
    b = _rand(N, seed=13).requires_grad_(True)
    y = F.conv2d(x, w, b, stride=2, padding=1 if k == 3 else 3)
    dy = _rand(*y.shape, seed=14)
    y.backward(dy)
    dw, db = ops.stem_wgrad(_nhwc(dy).cuda(), x.cuda(), N, k)
    assert (dw.cpu() - w.grad).abs().max().item() <= 1e-4 * max(1.0, float(w.grad.abs().max()))
    assert (db.cpu() - b.grad).abs().max().item() <= 1e-4 * max(1.0, float(b.grad.abs().max()))



def _check_grads_flip_aware(named_params, grads_ref, tight=('base.convdet.weight', 'base.convdet.bias')):
    """Gradients of a ReLU/max-pool network are discontinuous in the activations: one pre-activation
    within fp32 rounding of 0 flips a mask and moves every upstream gradient by ~1e-3 relative (the CPU
    fp32 run deviates from a float64 run by 3e-3..1e-2 for exactly that reason, see DESIGN.md
    "Backward parity").  ConvDet has no mask between it and the loss, so it is checked tightly; the
    rest is bounded at 5e-2 max-abs (relative to the tensor's scale) and 2e-2 relative L2 -- a wiring bug gives O(1)."""
    for name, p in named_params:
        ref = grads_ref[name].float()
        got = p.grad.cpu()
        scale = max(float(ref.abs().max()), 1e-3)
        err = (got - ref).abs().max().item() / scale
        rel2 = float((got - ref).norm() / max(float(ref.norm()), 1e-12))
        if name in tight:
            assert err <= 2e-4, f'{name}: {err}'
        assert err <= 5e-2 and rel2 <= 2e-2, f'{name}: max-rel {err} relL2 {rel2}'


def _train_model(arch, size, dropout_prob=0.0):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    cfg = sqd.make_cfg(arch=arch, input_size=size, dropout_prob=dropout_prob)
    m = SqueezeDetWithLoss(cfg)
    sd = synthetic.make_state_dict(arch, seed=1234)
    m.load_state_dict(sd, strict=True)
    return cfg, m.cuda().train(), sd


@pytest.mark.parametrize("arch", ["squeezedet", "squeezedetplus"])
def test_full_backward_vs_oracle(arch):
    size = (64, 96)
    cfg, m, sd = _train_model(arch, size)
    x = synthetic.make_images(2, size, seed=3)
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3)
    loss, stats = m({'image': x.cuda(), 'gt': gt.cuda()})
    loss.mean().backward()
    # ground truth in float64: the fp32 CPU run suffers its own mask flips (see _check_grads_flip_aware)
    sd64 = {k: v.double() for k, v in sd.items()}
    _, _, grads, total, loss_vec, _ = oracle.train_step_reference(sd64, None, x.double(), gt.double(),
                                                                  cfg.anchors.astype(np.float64), size, arch=arch)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), loss_vec.numpy(), rtol=1e-4)
    _check_grads_flip_aware(m.named_parameters(), grads)
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters())))
    assert abs(gn - total) <= 1e-2 * total


def test_train_step_vs_golden(golden_dir):
    """One step: fwd, loss.mean(), backward, clip_grad_norm_(5), SGD(momentum, wd) vs the reference's own run."""
    g = np.load(os.path.join(golden_dir, "train_step_small.npz"))
    size = (64, 96)
    cfg, m, sd = _train_model('squeezedet', size)
    x = synthetic.make_images(2, size, seed=3)
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3)
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    loss, stats = m({'image': x.cuda(), 'gt': gt.cuda()})
    loss = loss.mean()
    opt.zero_grad()
    loss.backward()
    names = [n for n, _ in m.named_parameters()]
    assert names == [str(n) for n in g["names"]]
    gn = np.array([float(p.grad.double().norm()) for _, p in m.named_parameters()])
    np.testing.assert_allclose(gn, g["grad_norms"], rtol=2e-2, atol=1e-6)      # flip-aware, see _check_grads_flip_aware
    total = float(torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0))
    assert abs(total - g["total_norm"][0]) <= 1e-2 * g["total_norm"][0]
    opt.step()
    assert abs(loss.item() - g["loss"][0]) <= 1e-4 * abs(g["loss"][0])
    ps = np.array([float(p.double().abs().sum()) for _, p in m.named_parameters()])
    np.testing.assert_allclose(ps, g["new_param_abs"], rtol=1e-4)
    np.testing.assert_allclose(m.base.convdet.bias.grad.cpu().numpy(), g["convdet_bias_grad"], rtol=2e-3, atol=1e-7)


def test_dropout_backward_with_injected_mask():
    size = (64, 96)
    cfg, m, sd = _train_model('squeezedet', size, dropout_prob=0.5)
    x = synthetic.make_images(2, size, seed=3)
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3)
    rs = np.random.RandomState(9)
    mask = torch.from_numpy((rs.uniform(size=(2, 768, 4, 6)) >= 0.5).astype(np.float32) * 2.0)
    m.base._forced_drop_mask = mask
    loss, _ = m({'image': x.cuda(), 'gt': gt.cuda()})
    loss.mean().backward()
    _, _, grads, total, loss_vec, _ = oracle.train_step_reference(sd, None, x, gt, cfg.anchors, size, drop_mask=mask)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), loss_vec.numpy(), rtol=1e-4)
    _check_grads_flip_aware(m.named_parameters(), grads)
    # eval mode: no dropout even if a mask is set
    m.eval()
    with torch.no_grad():
        pred = m.base(x.cuda())
    np.testing.assert_allclose(pred.cpu().numpy(), oracle.backbone_forward(x, sd).numpy(), atol=1e-4)


def test_kitti_size_backward_spot_check():
    """Full 1248x384, bs=2: loss + a few gradient tensors vs the oracle (CPU autograd ~ seconds)."""
    size = (384, 1248)
    cfg, m, sd = _train_model('squeezedet', size)
    x = synthetic.make_images(2, size, seed=0)
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=1)
    loss, _ = m({'image': x.cuda(), 'gt': gt.cuda()})
    loss.mean().backward()
    _, _, grads, total, loss_vec, _ = oracle.train_step_reference(sd, None, x, gt, cfg.anchors, size)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), loss_vec.numpy(), rtol=1e-4)
    _check_grads_flip_aware(m.named_parameters(), grads)


@pytest.mark.parametrize("k,N,H,W", [(3, 64, 64, 96), (3, 64, 50, 70), (7, 96, 64, 96)])
def test_stem_wgrad_pooled(k, N, H, W):
    """Fused forward (conv+ReLU+pool with argmax) + backward folded into the stem wgrad vs CPU autograd."""
    from squeezedet_pytorch_amd import ops
    x = _rand(2, 3, H, W, seed=31)
    w = _rand(N, 3, k, k, seed=32, scale=0.2).requires_grad_(True)
    b = _rand(N, seed=33, scale=0.1).requires_grad_(True)
    y = F.max_pool2d(F.relu(F.conv2d(x, w, b, stride=2, padding=1 if k == 3 else 3)), 3, 2, ceil_mode=True)
    dy = _rand(*y.shape, seed=34)
    y.backward(dy)
    am = torch.empty(*_nhwc(y.detach()).shape, dtype=torch.uint8, device='cuda')
    pooled = ops.stem_pool(x.cuda(), w.detach().cuda(), b.detach().cuda(), argmax=am)
    dw, db = ops.stem_wgrad_pooled(_nhwc(dy).cuda(), pooled, am, x.cuda(), N, k)
    assert (dw.cpu() - w.grad).abs().max().item() <= 2e-4 * max(1.0, float(w.grad.abs().max()))
    assert (db.cpu() - b.grad).abs().max().item() <= 2e-4 * max(1.0, float(b.grad.abs().max()))
    dw2, db2 = ops.stem_wgrad_pooled(_nhwc(dy).cuda(), pooled, am, x.cuda(), N, k)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)          # deterministic
    # the arg-max codes carry the ReLU mask (15 = pooled value 0): without the pooled tensor the result is the same, bit for bit
    dw3, db3 = ops.stem_wgrad_pooled(_nhwc(dy).cuda(), None, am, x.cuda(), N, k)
    assert torch.equal(dw, dw3) and torch.equal(db, db3)


@pytest.mark.parametrize("H,W", [(12, 16), (37, 44), (64, 96)])
def test_stem_wgrad_pooled_dense_and_gather_agree(H, W, monkeypatch):
    """The two kernels behind ops.stem_wgrad_pooled for the 3x3 / 64 stem -- the gather kernel (shipped) and the dense
    stem_wgrad_pooled_kernel (SQD_STEM_WGRAD_GATHER=0, read per call) -- on the SAME arg-max codes: dW and db agree to 1e-5 of
    max(1, |grad|max) (the bound of tools/fuzz_stem.py: they sum the same terms in different orders), and each is bit-identical
    run to run.  A map smaller than one tile, partial tiles with all four borders, whole tiles."""
    from squeezedet_pytorch_amd import ops
    x = _rand(2, 3, H, W, seed=41)
    w = _rand(64, 3, 3, 3, seed=42, scale=0.2).requires_grad_(True)
    b = _rand(64, seed=43, scale=0.1).requires_grad_(True)
    y = F.max_pool2d(F.relu(F.conv2d(x, w, b, stride=2, padding=1)), 3, 2, ceil_mode=True)
    dy = _rand(*y.shape, seed=44)
    y.backward(dy)
    gmax, bmax = max(1.0, float(w.grad.abs().max())), max(1.0, float(b.grad.abs().max()))
    xg, dyg = x.cuda(), _nhwc(dy).cuda()
    am = torch.empty(*_nhwc(y.detach()).shape, dtype=torch.uint8, device='cuda')
    ops.stem_pool(xg, w.detach().cuda(), b.detach().cuda(), argmax=am)
    res = {}
    for gather in ('0', '1'):
        monkeypatch.setenv('SQD_STEM_WGRAD_GATHER', gather)
        res[gather] = ops.stem_wgrad_pooled(dyg, None, am, xg, 64, 3)
        again = ops.stem_wgrad_pooled(dyg, None, am, xg, 64, 3)
        assert torch.equal(res[gather][0], again[0]) and torch.equal(res[gather][1], again[1]), gather
    monkeypatch.delenv('SQD_STEM_WGRAD_GATHER')
    dflt = ops.stem_wgrad_pooled(dyg, None, am, xg, 64, 3)                       # unset = the gather kernel
    assert torch.equal(dflt[0], res['1'][0]) and torch.equal(dflt[1], res['1'][1])
    ed = (res['1'][0] - res['0'][0]).abs().max().item() / gmax
    edb = (res['1'][1] - res['0'][1]).abs().max().item() / bmax
    print(f'{H}x{W}: dW {ed:.2e}, db {edb:.2e} of the gradient maximum')
    assert ed <= 1e-5 and edb <= 1e-5, (ed, edb)


def test_trainer_epochs_dense_and_sparse_annotations():
    """Trainer.train_epoch / val_epoch (src/engine/trainer.py:18-80) over a list "loader": logged losses match the
    oracle's step-by-step run, and batches with sparse annotations (encoded on the GPU) give the same run as
    batches with the host-encoded dense gt."""
    from squeezedet_pytorch_amd.trainer import Trainer
    size = (64, 96)
    logs = {}
    for mode in ("dense", "sparse"):
        cfg, m, sd = _train_model('squeezedet', size)
        cfg.num_iters, cfg.print_interval, cfg.grad_norm, cfg.device = -1, 1000, 5.0, 'cuda'
        cfg.gpus, cfg.chunk_sizes = [0], [2]
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.StepLR(opt, 60, gamma=0.5)
        tr = Trainer(m, opt, sched, cfg)
        loader = []
        for it in range(3):
            x = synthetic.make_images(2, size, seed=3 + it)
            cls_list, box_list = synthetic.make_gt_boxes(2, size, seed=20 + it, min_boxes=2, max_boxes=3)
            if mode == "dense":
                gt = torch.from_numpy(np.stack([oracle.encode_gt(c, b, cfg.anchors, 3, ties="lowest") for c, b in zip(cls_list, box_list)]))
                loader.append({'image': x, 'gt': gt, 'image_meta': {}})
            else:
                loader.append({'image': x, 'gt_boxes': box_list, 'gt_class_ids': cls_list, 'image_meta': {}})
        stats = tr.train_epoch(1, loader)
        vstats = tr.val_epoch(1, loader[:1])
        logs[mode] = (stats, vstats, [p.detach().clone() for p in m.parameters()])
        assert set(stats) == {'loss', 'class_loss', 'score_loss', 'bbox_loss', 'epoch_time'}
        assert m.training is False                       # val_epoch leaves the model in eval mode like the reference
    for k in ('loss', 'class_loss', 'score_loss', 'bbox_loss'):
        assert abs(logs['dense'][0][k] - logs['sparse'][0][k]) <= 1e-6 * abs(logs['dense'][0][k])
        assert abs(logs['dense'][1][k] - logs['sparse'][1][k]) <= 1e-6 * abs(logs['dense'][1][k])
    for a, b in zip(logs['dense'][2], logs['sparse'][2]):
        assert torch.equal(a, b)
    # the oracle's functional train step over the same three batches
    params = {k: v.clone() for k, v in sd.items()}
    mom = None
    losses = []
    for it in range(3):
        x = synthetic.make_images(2, size, seed=3 + it)
        cls_list, box_list = synthetic.make_gt_boxes(2, size, seed=20 + it, min_boxes=2, max_boxes=3)
        gt = torch.from_numpy(np.stack([oracle.encode_gt(c, b, cfg.anchors, 3, ties="lowest") for c, b in zip(cls_list, box_list)]))
        params, mom, _, _, loss_vec, _ = oracle.train_step_reference(params, mom, x, gt, cfg.anchors, size, arch='squeezedet')
        losses.append(float(loss_vec.mean()))
    assert abs(logs['dense'][0]['loss'] - np.mean(losses)) <= 2e-3 * abs(np.mean(losses))


def test_train_step_vs_golden_through_winograd_kernels(golden_dir, monkeypatch):
    """The reference's own training step (golden) with every 3x3 forward, data gradient and weight gradient forced onto the
    Winograd kernels: same tolerances as the default path."""
    from squeezedet_pytorch_amd import ops
    monkeypatch.setattr(ops, 'choose_wino_cfg', lambda C, N, npix: (2 if C % 8 == 0 else None))
    monkeypatch.setattr(ops, 'WINO_WGRAD', True)
    test_train_step_vs_golden(golden_dir)
    calls = {'wino': 0}
    real = ops.conv_wino

    def counting(*a, **k):
        calls['wino'] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, 'conv_wino', counting)
    test_train_step_vs_golden(golden_dir)
    assert calls['wino'] >= 21                               # 11 forward + >= 10 data gradients went through conv_wino


def test_fused_clip_sgd_matches_torch():
    """trainer.FusedClipSGD (clip_grad_norm_ + SGD with momentum and weight decay in one launch, csrc/optim.hip) against the two
    torch calls of the reference's training step (src/engine/trainer.py:47-50) over several steps: parameters and momentum agree to
    fp32 rounding (torch contracts `g + wd * p` into an fma), with the clip active (large gradients) and inactive (small)."""
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    torch.manual_seed(0)
    shapes = [(64, 3, 3, 3), (64,), (16, 64, 1, 1), (16,), (72, 768, 3, 3), (72,), (5,)]
    ref = [torch.nn.Parameter(torch.randn(*s, device='cuda') * 0.1) for s in shapes]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    topt = torch.optim.SGD(ref, lr=0.01, momentum=0.9, weight_decay=1e-4)
    fopt = FusedClipSGD(mine, lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=5.0)
    for step in range(5):
        scale = 3.0 if step % 2 == 0 else 1e-3            # clipped / not clipped
        grads = [torch.randn(*s, device='cuda') * scale for s in shapes]
        for p, q, g in zip(ref, mine, grads):
            p.grad = g.clone(); q.grad = g.clone()
        tn = torch.nn.utils.clip_grad_norm_(ref, 5.0)
        topt.step()
        v0 = mine[0]._version
        fn = fopt.step()
        assert mine[0]._version > v0                        # the packed-weight caches key on it
        assert abs(float(tn) - float(fn)) <= 1e-5 * float(tn)
        for p, q in zip(ref, mine):
            assert torch.allclose(p, q, rtol=2e-6, atol=1e-8), (step, float((p - q).abs().max()))
        for p, b in zip(ref, fopt._bufs):
            assert torch.allclose(topt.state[p]['momentum_buffer'].reshape(-1), b, rtol=2e-6, atol=1e-8)
    sd = fopt.state_dict()
    fopt2 = FusedClipSGD(mine, lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=5.0)
    fopt2.load_state_dict(sd)
    assert torch.equal(fopt2.momentum_flat, fopt.momentum_flat)


def test_train_steps_with_fused_optimizer_vs_torch_and_golden(golden_dir):
    """The training step bench.py times -- fwd, loss.mean(), HIP backward into the flat gradient buffer, FusedClipSGD (clip + SGD in
    one launch, gradients addressed as offsets into the flat buffer) -- against (a) the reference's own run of the first step
    (golden: loss, total gradient norm, |params| after the update) and (b) three steps of the same model driven by
    clip_grad_norm_ + torch.optim.SGD: parameters agree to fp32 rounding, and the packed-weight caches follow the in-place updates
    (the second step's loss matches)."""
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    g = np.load(os.path.join(golden_dir, "train_step_small.npz"))
    size = (64, 96)
    cfg, ma, sd = _train_model('squeezedet', size)
    _, mb, _ = _train_model('squeezedet', size)
    x = synthetic.make_images(2, size, seed=3).cuda()
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3).cuda()
    fo = FusedClipSGD(ma.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, max_norm=5.0, flat_grad=lambda: ma.base.last_grad_flat)
    to = torch.optim.SGD(mb.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    for step in range(3):
        la, _ = ma({'image': x, 'gt': gt}); la = la.mean(); fo.zero_grad(); la.backward()
        lb, _ = mb({'image': x, 'gt': gt}); lb = lb.mean(); to.zero_grad(); lb.backward()
        assert fo._flat_base([p.grad for p in fo.params]) is not None          # the one-reduction norm / offset table path
        norm = float(fo.step())
        tn = float(torch.nn.utils.clip_grad_norm_(mb.parameters(), 5.0)); to.step()
        assert abs(norm - tn) <= 1e-5 * tn
        assert abs(la.item() - lb.item()) <= 1e-5 * abs(lb.item()), step
        for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), (step, n, float((p - q).abs().max()))
        if step == 0:
            assert abs(norm - g["total_norm"][0]) <= 1e-2 * g["total_norm"][0]
            assert abs(la.item() - g["loss"][0]) <= 1e-4 * abs(g["loss"][0])
            ps = np.array([float(p.double().abs().sum()) for _, p in ma.named_parameters()])
            np.testing.assert_allclose(ps, g["new_param_abs"], rtol=1e-4)


def test_trainer_with_steplr_and_fused_optimizer():
    """FusedClipSGD is a torch.optim.Optimizer: the reference's schedule (src/train.py:36 StepLR, stepped once per epoch at
    src/engine/trainer.py:67) drives its learning rate, Trainer clips exactly once (inside the fused launch), and two epochs through
    ``Trainer`` equal the same two epochs driven by clip_grad_norm_ + torch.optim.SGD + StepLR.  Also: a parameter whose storage is
    replaced after the first step rebuilds the descriptor table (no write through a stale pointer)."""
    from squeezedet_pytorch_amd.trainer import FusedClipSGD, Trainer
    size = (64, 96)
    cfg, ma, sd = _train_model('squeezedet', size)
    _, mb, _ = _train_model('squeezedet', size)
    cfg.num_iters, cfg.print_interval = -1, 1000
    x = synthetic.make_images(2, size, seed=3)
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3)
    loader = [{'image': x, 'gt': gt}, {'image': x.flip(0), 'gt': gt.flip(0)}]
    fo = FusedClipSGD(ma.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4, max_norm=cfg.grad_norm, flat_grad=lambda: ma.base.last_grad_flat)
    fs = torch.optim.lr_scheduler.StepLR(fo, 1, 0.5)               # raises TypeError on a non-Optimizer
    to = torch.optim.SGD(mb.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)
    ts = torch.optim.lr_scheduler.StepLR(to, 1, 0.5)
    ta, tb = Trainer(ma, fo, fs, cfg), Trainer(mb, to, ts, cfg)
    for epoch in range(2):
        ra, rb = ta.train_epoch(epoch, loader), tb.train_epoch(epoch, loader)
        assert abs(ra['loss'] - rb['loss']) <= 1e-5 * abs(rb['loss'])
        assert fo.param_groups[0]['lr'] == to.param_groups[0]['lr'] == 0.02 * 0.5 ** (epoch + 1)
        for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
            assert torch.allclose(p, q, rtol=2e-5, atol=1e-7), (epoch, n, float((p - q).abs().max()))
    sd1 = fo.state_dict()
    assert sd1['lr'] == 0.005 and sd1['initial_lr'] == 0.02
    # storage replaced behind the optimizer's back: the table must follow (same update as torch on the new storage)
    key0 = fo._table_key
    with torch.no_grad():
        for p, q in zip(ma.parameters(), mb.parameters()):
            p.data = p.data.clone()
    la, _ = ma({'image': x.cuda(), 'gt': gt.cuda()}); fo.zero_grad(); la.mean().backward(); fo.step()
    lb, _ = mb({'image': x.cuda(), 'gt': gt.cuda()}); to.zero_grad(); lb.mean().backward()
    torch.nn.utils.clip_grad_norm_(mb.parameters(), cfg.grad_norm); to.step()
    assert fo._table_key != key0
    for (n, p), q in zip(ma.named_parameters(), mb.parameters()):
        assert torch.allclose(p, q, rtol=2e-5, atol=1e-7), n


@pytest.mark.parametrize("C,N,B,H,W,mask", [(64, 16, 2, 24, 39, False), (128, 16, 2, 17, 23, True), (256, 32, 2, 12, 20, True),
                                            (384, 48, 3, 7, 13, True), (512, 64, 2, 9, 11, True), (768, 96, 2, 24, 78, True),
                                            (48, 96, 1, 5, 7, True), (512, 96, 20, 24, 78, True)])
def test_squeeze_bwd_one_launch(C, N, B, H, W, mask):
    """ops.squeeze_bwd (a Fire squeeze's weight gradient slabs + data gradient + the previous Fire's ReLU mask in one launch) vs
    autograd of relu -> conv1x1 on the CPU, and vs the two separate kernels it replaces: the slabs are bitwise those of
    conv_wgrad's tiling when the tilings coincide, the data gradient equals the conv kernel's to fp32 rounding; odd pixel
    counts (partial last block), channel counts off the 64-channel tile, mask on and off."""
    from squeezedet_pytorch_amd import ops
    pre = _rand(B, C, H, W, seed=41).requires_grad_(True)
    xin = F.relu(pre) if mask else pre
    w = _rand(N, C, 1, 1, seed=42, scale=(2.0 / C) ** 0.5).requires_grad_(True)
    b = _rand(N, seed=43, scale=0.1).requires_grad_(True)
    y = F.conv2d(xin, w, b)
    dy = _rand(*y.shape, seed=44)
    y.backward(dy)
    x_nhwc = _nhwc(xin.detach()).cuda()
    dy_nhwc = _nhwc(dy).cuda()
    S, stride = ops.wgrad_split(N, C, 1, B, H, W, fused_dgrad=True)
    slab = torch.full((S * stride,), float('nan'), device='cuda')
    dx = torch.full_like(x_nhwc, float('nan'))
    ops.squeeze_bwd(dy_nhwc, x_nhwc, w.detach().cuda().contiguous(), slab, dx, relu_mask=mask)
    torch.cuda.synchronize()
    red = slab.view(S, stride).double().sum(0).cpu()
    assert not torch.isnan(red).any() and not torch.isnan(dx).any()
    dw = red[:N * C].view(N, C, 1, 1)
    db = red[N * C:]
    scale_w = max(1.0, float(w.grad.abs().max()))
    assert (dw - w.grad.double()).abs().max().item() <= 2e-4 * scale_w
    assert (db - b.grad.double()).abs().max().item() <= 2e-4 * max(1.0, float(b.grad.abs().max()))
    want_dx = _nhwc(pre.grad)                       # through the ReLU when mask: dpre = dx * (pre > 0)
    assert (dx.cpu() - want_dx).abs().max().item() <= 2e-5 * max(1.0, float(want_dx.abs().max()))
    # the separate kernels it replaces
    plan = ops.ConvPlan(w.detach().cuda(), None, ops.choose_cfg(1, N, C, B * H * W), dgrad=True)
    dx2 = torch.empty_like(x_nhwc)
    ops.conv(dy_nhwc, 0, plan, dx2, 0, ymask=x_nhwc if mask else None)
    assert (dx - dx2).abs().max().item() <= 1e-5 * max(1.0, float(want_dx.abs().max()))
    # run-to-run reproducible
    slab2 = torch.empty_like(slab); dx3 = torch.empty_like(dx)
    ops.squeeze_bwd(dy_nhwc, x_nhwc, w.detach().cuda().contiguous(), slab2, dx3, relu_mask=mask)
    assert torch.equal(slab, slab2) and torch.equal(dx, dx3)


def test_backward_with_and_without_fused_squeeze_bwd_agree():
    """Whole backward, SqueezeDetBase.fuse_squeeze_bwd on vs off: same gradients to fp32 rounding (the weight-gradient split
    differs, so not bitwise), flat-buffer layout intact either way."""
    size = (64, 96)
    cfg, m, sd = _train_model('squeezedet', size)
    x = synthetic.make_images(2, size, seed=3).cuda()
    gt = synthetic.make_gt(2, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3).cuda()
    grads = {}
    for flag in (True, False):
        m.base.fuse_squeeze_bwd = flag
        m.zero_grad()
        loss, _ = m({'image': x, 'gt': gt})
        loss.mean().backward()
        grads[flag] = {n: p.grad.clone() for n, p in m.named_parameters()}
    for n in grads[True]:
        a, b = grads[True][n], grads[False][n]
        assert (a - b).abs().max().item() <= 2e-5 * max(float(b.abs().max()), 1e-3), n


@pytest.mark.parametrize("s,e1,B,H,W", [(16, 64, 2, 24, 39), (32, 128, 2, 13, 21), (16, 128, 1, 7, 9)])
def test_fused_1x1_backward_serves_expand1x1(s, e1, B, H, W):
    """The same launch as a Fire's expand1x1 backward (N = e1 <= 128): dy = the expand1x1 WINDOW of the Fire output's gradient
    (pitch 2 e1), x = the squeeze output, no mask here (the expand3x3 data gradient accumulates onto dx and masks)."""
    from squeezedet_pytorch_amd import ops
    sq = _rand(B, s, H, W, seed=51).requires_grad_(True)
    w = _rand(e1, s, 1, 1, seed=52, scale=(2.0 / s) ** 0.5).requires_grad_(True)
    b = _rand(e1, seed=53, scale=0.1).requires_grad_(True)
    y = F.conv2d(sq, w, b)
    dy = _rand(*y.shape, seed=54)
    y.backward(dy)
    dA = torch.randn(B, H, W, 2 * e1, device='cuda')              # [expand1x1 | expand3x3] halves of the Fire output's gradient
    dA[..., :e1] = _nhwc(dy).cuda()
    S, stride = ops.wgrad_split(e1, s, 1, B, H, W, fused_dgrad=True)
    slab = torch.full((S * stride,), float('nan'), device='cuda')
    dx = torch.full((B, H, W, s), float('nan'), device='cuda')
    ops.squeeze_bwd(dA, _nhwc(sq.detach()).cuda(), w.detach().cuda().contiguous(), slab, dx, relu_mask=False, dy_coff=0, N=e1)
    red = slab.view(S, stride).double().sum(0).cpu()
    assert (red[:e1 * s].view(e1, s, 1, 1) - w.grad.double()).abs().max().item() <= 2e-4 * max(1.0, float(w.grad.abs().max()))
    assert (red[e1 * s:] - b.grad.double()).abs().max().item() <= 2e-4 * max(1.0, float(b.grad.abs().max()))
    assert (dx.cpu() - _nhwc(sq.grad)).abs().max().item() <= 2e-5 * max(1.0, float(sq.grad.abs().max()))


def test_mean_loss_node_equals_loss_mean():
    """``SqueezeDetWithLoss.forward_mean`` (loss.mean() and its backward inside the loss kernels, backward.LossMeanFn) == the
    reference's two lines ``loss, stats = model(batch); loss.mean().backward()`` (src/engine/trainer.py:42-47): the scalar to fp32
    rounding of the mean, the per-image statistics bit for bit, every parameter gradient to rounding (the upstream coefficient 1/B
    is formed inside the kernel instead of by torch's broadcast)."""
    size = (64, 96)
    cfg, m, sd = _train_model('squeezedet', size)
    x = synthetic.make_images(3, size, seed=3).cuda()
    gt = synthetic.make_gt(3, cfg.anchors, size, seed=2, min_boxes=2, max_boxes=3).cuda()
    loss, stats = m({'image': x, 'gt': gt})
    loss.mean().backward()
    ref = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    m.zero_grad()
    mean, stats2 = m.forward_mean({'image': x, 'gt': gt})
    assert mean.dim() == 0 and abs(float(mean) - float(loss.mean())) <= 1e-6 * abs(float(loss.mean()))
    for k in ('loss', 'class_loss', 'score_loss', 'bbox_loss'):
        assert torch.equal(stats[k].detach(), stats2[k])
    mean.backward(torch.ones((), device='cuda'))
    for n, p in m.named_parameters():
        scale = float(ref[n].abs().max()) + 1e-20
        assert float((p.grad - ref[n]).abs().max()) <= 2e-5 * scale, n
