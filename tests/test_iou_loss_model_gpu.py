"""GPU tier of ``cfg.bbox_loss`` through the module surface: ``SqueezeDetWithLoss(make_cfg(bbox_loss=...))`` at the smallest
whole-step point of tests/test_fp64_offbench_gpu.py (squeezedet, batch 1, 48x48: a 3x3 grid, 81 anchors).  ``forward`` (per-image
losses, the coef backward) and ``forward_mean`` (the mean inside the launch, the gmean backward) are held to the float64 twin of
tests/iou_loss_ref.py at bar L on the model's own ``pred``: the statistics and the dpred that arrives at the backbone.  Then three
steps of the captured training step equal the eager loop bit for bit, by the method of tests/test_graph_step_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ref as R  # noqa: E402
import iou_loss_ref as Q  # noqa: E402
import test_fp64_loss_gpu as LG  # noqa: E402
import test_fp64_offbench_gpu as OB  # noqa: E402
import test_graph_step_gpu as GS  # noqa: E402

pytestmark = pytest.mark.gpu

ARCH, BATCH, SIZE = min(OB.POINTS, key=lambda p: (p[2][0] * p[2][1], p[1]))
C = 3
KEYS = ('class_loss', 'score_loss', 'bbox_loss', 'loss')


def _model(cfg):
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict(ARCH, seed=1234, num_classes=C))
    return m.cuda().train()


def _run(kind, batch, gt_dense, ign=None, **cfg_kw):
    """forward + backward and forward_mean + backward of one batch -> both against the twin on the pred the model computed."""
    import squeezedet_pytorch_amd as sqd
    assert (ARCH, BATCH, SIZE) == ('squeezedet', 1, (48, 48))
    cfg = sqd.make_cfg(arch=ARCH, input_size=SIZE, num_classes=C, device='cuda', dropout_prob=0.0, bbox_loss=kind, **cfg_kw)
    model = _model(cfg)
    assert model.loss.bbox_loss == kind
    seen = []

    def keep(_module, _inputs, out):
        out.retain_grad()
        seen.append(out)
    model.base.register_forward_hook(keep)
    loss, stats = model(batch)
    loss.mean().backward()
    mean, mstats = model.forward_mean(batch)
    mean.backward()
    torch.cuda.synchronize()
    (p0, p1) = seen
    assert torch.equal(p0.detach(), p1.detach())
    pred = p0.detach().cpu()
    anchors = model.loss.resolver.anchors_on('cuda').cpu()
    weights = (cfg.class_loss_weight, cfg.positive_score_loss_weight, cfg.negative_score_loss_weight, cfg.bbox_loss_weight)
    coef = torch.full((3, BATCH), 1.0 / BATCH)
    if ign is None:
        ref = Q.loss(pred, gt_dense, anchors, SIZE, C, weights, kind, gmean=1.0, coef=coef)
    else:
        ref = Q.masked_loss(kind, pred, gt_dense, ign, anchors, SIZE, C, weights, gmean=1.0, coef=coef)
    flips = int(ref['flips'].sum())
    res = {'forward': R.bars_nan(torch.stack([stats[k] for k in KEYS]).detach().cpu(), ref['losses'], 'vec', 2),
           'forward_mean': R.bars_nan(torch.stack([mstats[k] for k in KEYS]).detach().cpu(), ref['losses'], 'vec', 2),
           'mean': R.bars_nan(mean.detach().cpu().reshape(1), R.Ref(*(t[3:4] for t in ref['mean4'])), 'vec', 2)}
    assert torch.equal(loss.detach(), stats['loss'].detach()) and bool(torch.isfinite(loss).all())
    for name, got, key in (('dpred (forward)', p0.grad.cpu(), 'dcoef'), ('dpred (forward_mean)', p1.grad.cpu(), 'dmean')):
        res[name] = R.bars_nan(got, R.pick(got, ref[key], ref[key + '_alt'], ref['flips']), 'dpred', 2)
    for k, b in res.items():
        print(f'module {kind:5s} {k:22s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e}) flips {flips}')
    assert all(b['l_ok'] for b in res.values()), {k: b for k, b in res.items() if not b['l_ok']}
    assert flips <= LG.MAX_FLIPS
    assert float(ref['losses'].ref64[2].abs().max()) > 0, 'the batch has no box term'


def test_dense_giou_through_the_module():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    cfg = sqd.make_cfg(arch=ARCH, input_size=SIZE, num_classes=C, device='cpu')
    gt = synthetic.make_gt(BATCH, cfg.anchors, SIZE, C, seed=3, min_boxes=3, max_boxes=5)
    batch = {'image': synthetic.make_images(BATCH, SIZE, seed=5).cuda(), 'gt': gt.cuda()}
    _run('giou', batch, gt)


def test_sparse_ciou_with_ignore_regions_through_the_module():
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import boxes, ops, synthetic
    from squeezedet_pytorch_amd.annotations import encode_annotations
    cfg = sqd.make_cfg(arch=ARCH, input_size=SIZE, num_classes=C, device='cpu')
    cls_list, box_list = synthetic.make_gt_boxes(BATCH, SIZE, C, seed=3, min_boxes=3, max_boxes=5)
    ign_boxes = [np.array([[0., 0., 47., 30.]], np.float32)] * BATCH       # the anchors that lie to one half on the upper 30 rows
    sgt, bitmap = encode_annotations(cls_list, box_list, cfg.anchors, C, dense=False, ignore_boxes_list=ign_boxes, ignore_overlap=0.5)
    A = cfg.num_anchors
    ign = boxes.unpack_ignore_bits(bitmap.cpu().numpy(), A)
    assert 0 < int(ign.sum()) < ign.size
    batch = {'image': synthetic.make_images(BATCH, SIZE, seed=5).cuda(), 'gt_sparse': sgt, 'gt_ignore': bitmap}
    _run('ciou', batch, ops.sparse_gt_to_dense(sgt, A, C).cpu(), ign=ign, sparse_gt=True, ignore_overlap=0.5)


def test_three_captured_steps_equal_the_eager_loop():
    """An eager first step, a capture, a replay (GraphedStep): parameters, momentum, losses and the norm equal the eager loop's bits
    after every step, with the box kind in the captured launches; a step under another kind has another signature."""
    cfg = GS.make_cfg(bbox_loss='giou', graph_step=True)
    batches = [GS.make_batch(cfg, 'dense', 2, seed) for seed in (1, 2, 3)]
    g, e = GS.run_pair(cfg, batches)
    assert g.gs.captures >= 1 and g.gs.replays >= 1 and g.gs.eager_steps == 1
    sig = g.gs.signature(batches[0])
    assert sig[-1] == 'giou'
    g.model.loss.bbox_loss = 'l2'                             # (what a capture is valid for: another kind is another step)
    assert g.gs.signature(batches[0]) == sig[:-1] + ('l2',)
