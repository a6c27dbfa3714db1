"""GPU tier: a SqueezeDet of any class count.  ConvDet's width anchors_per_grid * (num_classes + 5) is a multiple of 4 for 3, 7, 11, ...
classes only; every other width runs zero-padded (``ops.convdet_width``) with a pack / unpack launch around it, and past 16 classes
the head runs on the many-class kernels.  Forward, one training step and the detector paths against the oracle, at sizes where
ConvDet is tiny even at 768 -> 768 channels."""
import numpy as np
import pytest
import torch

import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import ops, synthetic
from test_lanes_gpu import _images, _same

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.mark.parametrize('arch,C,size,B', [('squeezedet', 5, (64, 96), 2), ('squeezedet', 20, (70, 100), 1),
                                          ('squeezedet', 80, (64, 96), 2), ('squeezedetplus', 20, (64, 96), 1)])
def test_forward_any_class_count(arch, C, size, B):
    from squeezedet_pytorch_amd.model import SqueezeDet
    cfg = sqd.make_cfg(arch=arch, input_size=size, num_classes=C)
    assert ops.convdet_padded(cfg.anchors_per_grid, C)
    m = SqueezeDet(cfg)
    sd = synthetic.make_state_dict(arch, seed=1234, num_classes=C)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    shapes = oracle.param_shapes(arch, 9, C)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(v) for k, v in shapes.items()}
    x = synthetic.make_images(B, size, seed=5)
    with torch.no_grad():
        det = m({'image': x.cuda()})
        pred = m.base(x.cuda())
        ref = oracle.backbone_forward(x, sd, arch, C)
    assert tuple(pred.shape) == tuple(ref.shape) == (B, cfg.num_anchors, C + 5) and pred.is_contiguous()
    err = (pred.cpu() - ref).abs().max().item()
    print(f'any width {arch} C{C} {size}: max |pred - oracle| {err:.3e}')
    assert err <= TOL
    ids, sc, bx = oracle.inference_head(ref, cfg.anchors, size, C)
    np.testing.assert_allclose(det['scores'].cpu().numpy(), sc.numpy(), atol=TOL)
    np.testing.assert_allclose(det['boxes'].cpu().numpy(), bx.numpy(), atol=5e-3)
    assert det['class_ids'].dtype == torch.int64 and int(det['class_ids'].max()) < C
    # ConvDet called on its own, as the reference's nn.Conv2d allows: NCHW in, NCHW out of the parameter's own width
    feat = torch.relu(torch.from_numpy(np.random.RandomState(C).standard_normal((B, m.base.convdet.in_channels, 4, 6)).astype(np.float32)))
    alone = m.base.convdet(feat.cuda())
    want = torch.nn.functional.conv2d(feat, sd['base.convdet.weight'], sd['base.convdet.bias'], padding=1)
    assert tuple(alone.shape) == tuple(want.shape) and (alone.cpu() - want).abs().max().item() <= TOL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('C,drop', [(5, False), (20, False), (80, False), (20, True)])
def test_training_step_any_class_count(C, drop):
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    from squeezedet_pytorch_amd.trainer import FusedClipSGD
    arch, size, B = 'squeezedet', (64, 96), 2
    cfg = sqd.make_cfg(arch=arch, input_size=size, num_classes=C, dropout_prob=0.5 if drop else 0.0)
    m = SqueezeDetWithLoss(cfg)
    sd = synthetic.make_state_dict(arch, seed=1234, num_classes=C)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().train()
    x = synthetic.make_images(B, size, seed=3)
    gt = synthetic.make_gt(B, cfg.anchors, size, num_classes=C, seed=2, min_boxes=2, max_boxes=3)
    mask = None
    if drop:
        rs = np.random.RandomState(9)
        mask = torch.from_numpy((rs.uniform(size=(B, 768, 4, 6)) >= 0.5).astype(np.float32) * 2.0)
        m.base._forced_drop_mask = mask
    loss, _ = m({'image': x.cuda(), 'gt': gt.cuda()})
    loss.mean().backward()
    sd64 = {k: v.double() for k, v in sd.items()}
    _, _, grads, total, loss_vec, _ = oracle.train_step_reference(sd64, None, x.double(), gt.double(), cfg.anchors.astype(np.float64), size,
                                                                  arch=arch, num_classes=C,
                                                                  drop_mask=None if mask is None else mask.double())
    np.testing.assert_allclose(loss.detach().cpu().numpy(), loss_vec.numpy(), rtol=1e-4)
    params = dict(m.named_parameters())
    # ConvDet's own gradients, and the last Fire's expand weights: the padded data gradient reaches them
    for name in ('base.convdet.weight', 'base.convdet.bias', 'base.features.14.expand1x1.weight', 'base.features.14.expand3x3.weight'):
        ref = grads[name].float()
        got = params[name].grad.cpu()
        err = (got - ref).abs().max().item()
        print(f'any width C{C} drop={drop} {name}: max err {err:.3e} of max |ref| {float(ref.abs().max()):.3e}')
        assert err <= 2e-4 * max(float(ref.abs().max()), 1e-3), name
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters())))
    assert abs(gn - total) <= 2e-2 * total
    w = params['base.convdet.weight']
    assert w.grad.shape == w.shape == (9 * (C + 5), 768, 3, 3)
    flat = m.base.last_grad_flat
    lo = (w.grad.data_ptr() - flat.data_ptr()) // 4
    assert w.grad.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() and 0 <= lo and lo + w.numel() <= flat.numel()
    assert torch.equal(flat[lo:lo + w.numel()].view(w.shape), w.grad)
    # one fused clip + SGD step moves every parameter
    before = {k: p.detach().clone() for k, p in params.items()}
    opt = FusedClipSGD(list(m.parameters()), lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay, max_norm=cfg.grad_norm,
                       flat_grad=lambda: m.base.last_grad_flat)
    opt.step()
    torch.cuda.synchronize()
    for k, p in params.items():
        assert not torch.equal(p.detach(), before[k]), f'{k} did not change'
    # the next forward sees the updated ConvDet (the padded stand-in follows the parameters)
    m.eval()
    with torch.no_grad():
        pred = m.base(x.cuda())
        ref = oracle.backbone_forward(x, {k: v.detach().cpu() for k, v in m.state_dict().items()}, arch, C)
    assert (pred.cpu() - ref).abs().max().item() <= TOL


@pytest.mark.parametrize('K', [64, 100])
def test_detector_twenty_classes(K):
    from squeezedet_pytorch_amd.model import SqueezeDet
    from squeezedet_pytorch_amd.detector import Detector
    C, size = 20, (64, 96)
    cfg = sqd.make_cfg(input_size=size, num_classes=C, keep_top_k=K, score_thresh=0.1, batch_size=2)
    m = SqueezeDet(cfg)
    m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234, num_classes=C))
    det = Detector(m, cfg)
    x = synthetic.make_images(2, size, seed=5).cuda()
    with torch.no_grad():
        dense = det.model({'image': x})
    res = det.detect({'image': x})
    kept = 0
    for b in range(2):
        exp = oracle.filter_detections(dense['class_ids'][b].cpu().numpy(), dense['scores'][b].cpu().numpy(),
                                       dense['boxes'][b].cpu().numpy(), K, cfg.nms_thresh, cfg.score_thresh, C)
        assert (exp is None) == ('scores' not in res[b])
        if exp is not None:
            for k in ('class_ids', 'anchor_idx'):
                assert np.array_equal(res[b][k], exp[k]), k
            for k in ('scores', 'boxes'):
                assert np.array_equal(res[b][k].view(np.int32), exp[k].view(np.int32)), k
            kept += len(exp['scores'])
            # Detector.filter on the dense dict of one image: the same rows
            f = det.filter({k: v[b] for k, v in dense.items()})
            assert np.array_equal(f['anchor_idx'].cpu().numpy(), exp['anchor_idx'])
    assert kept > 20
    # the captured-lane path with the many-class buffers: three batches of 2, bit for bit what detect_images gives
    images = _images(6, [(70, 100), (64, 96), (61, 93)])
    batches = [images[i:i + 2] for i in range(0, 6, 2)]
    got = list(det.detect_stream(batches))
    ndet = 0
    for bt, rs in zip(batches, got):
        for r, w in zip(rs, det.detect_images(bt)):
            _same(r, w)
            ndet += len(w.get('scores', ()))
    assert ndet > 0 and not det.stream().degraded


def test_launch_plans_equal_real_launches_twenty_classes():
    """plan.inference_launch_plan / training_launch_plan list the padded ConvDet, the pack / unpack launches and the many-class
    detect exactly as the executors issue them (default dropout: the counter-based stream, ConvDet's data gradient on the balanced
    Winograd kernel with the padded width as its C)."""
    from squeezedet_pytorch_amd import plan
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet, SqueezeDetWithLoss
    C, size, B = 20, (64, 96), 2
    cfg = sqd.make_cfg(input_size=size, num_classes=C)
    sd = synthetic.make_state_dict('squeezedet', seed=1234, num_classes=C)
    x = synthetic.make_images(B, size, seed=0).cuda()

    def bracketed(fn):
        fn()
        timer = ops.KernelTimer()
        ops.set_timer(timer)
        try:
            fn()
        finally:
            ops.set_timer(None)
        torch.cuda.synchronize()
        return [(r[0], r[1]) for r in timer.records]
    m = SqueezeDet(cfg)
    m.load_state_dict(sd)
    det = Detector(m, cfg)
    got = bracketed(lambda: det.detect_device(x))
    want = plan.inference_launch_plan('squeezedet', B, size, num_classes=C)
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:4] + [len(got), len(want)]
    assert want[-1] == ('detect', 'detect_many A216 K64')
    t = SqueezeDetWithLoss(cfg)
    t.load_state_dict(sd)
    t = t.cuda().train()
    batch = {'image': x, 'gt': synthetic.make_gt(B, cfg.anchors, size, num_classes=C, seed=1).cuda()}

    def step():
        loss, _ = t(batch)
        t.zero_grad()
        loss.mean().backward()
    got = bracketed(step)
    want = plan.training_launch_plan('squeezedet', B, size, num_classes=C)
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:4] + [len(got), len(want)]
    assert all(torch.isfinite(p.grad).all() for p in t.parameters())
