"""GPU tier, N > 1 path on the HIP backward: two processes (gloo rendezvous, both on this box's one GPU) run the reference's
training iteration (src/engine/trainer.py:42-50: model(batch) -> loss.mean() -> zero_grad -> backward -> clip -> step) on
UNEQUAL shards (3 + 2 images) with ``attach_data_parallel``; the gradient every rank ends up with must be the gradient of
the mean over the global batch, i.e. what ONE process computes on all 5 images -- through the staged slab reductions, the
three buckets handed to the all-reduce during the backward and the count-weighted average.

That comparison carries the ReLU-flip noise of another batch partition (bar 1e-2).  The exchange itself is held tightly: every worker
first runs its shard with no exchange attached, and rank 0's exchanged buffer must be the count-weighted mean of those two local
gradients within 2^-18 M on every element (tests/dp_exchange_ref.py) -- through the real two-process collective."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (64, 96)


def _setup(B_lo, B_hi):
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    from squeezedet_pytorch_amd.model import SqueezeDetWithLoss
    cfg = sqd.make_cfg(input_size=SIZE, dropout_prob=0.0, device='cuda')
    m = SqueezeDetWithLoss(cfg)
    m.load_state_dict(synthetic.make_state_dict('squeezedet', seed=1234))
    m = m.cuda().train()
    x = synthetic.make_images(5, SIZE, seed=3)[B_lo:B_hi].cuda()
    gt = synthetic.make_gt(5, cfg.anchors, SIZE, seed=2, min_boxes=2, max_boxes=3)[B_lo:B_hi].cuda()
    return cfg, m, {'image': x, 'gt': gt}


def _local_gradient(m, batch):
    """This rank's gradient of its LOCAL mean on the weights it holds now, no exchange attached (on the CPU): what the exchange is a
    linear map of (tests/dp_exchange_ref.py).  The attached exchange is put back."""
    ex, m.base.grad_sync = m.base.grad_sync, None
    try:
        loss, _ = m(batch)
        m.zero_grad()
        loss.mean().backward()
        torch.cuda.synchronize()
        return m.base.last_grad_flat.detach().cpu().clone()
    finally:
        m.zero_grad()
        m.base.grad_sync = ex


def check_exchange_against_local_gradients(got, locals_, shards, tag):
    """``|got - (sum b_r g_r) / sum b_r| <= 2^-18 M`` on every element of the flat buffer (tests/dp_exchange_ref.py)."""
    import dp_exchange_ref as X
    want, M = X.expected_and_M(locals_, shards)
    ok, ratio, nbad = X.hold_bar(got, want, M)
    print(f'dp exchange {tag:44s} max |d|/M {ratio:.3e} (bar {X.BAR_L:.3e})  outside {nbad} of {got.numel()}')
    assert ok, f'{tag}: {nbad} elements outside 2^-18 M, worst ratio {ratio:.3e}'


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from squeezedet_pytorch_amd.trainer import attach_data_parallel
    lo, hi = (0, 3) if rank == 0 else (3, 5)
    cfg, m, batch = _setup(lo, hi)
    if rank == 1:                                           # start from different weights: the attach must replicate rank 0's
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01)
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    ex = attach_data_parallel(m, opt)
    local = _local_gradient(m, batch)
    loss, _ = m(batch)
    opt.zero_grad()
    loss.mean().backward()
    torch.cuda.synchronize()
    assert len(ex.buckets_last_step) == 4                   # 24x78 stage + ConvDet, 48x156 stage, 96x312 stage, stem
    assert ex.buckets_last_step[0][1] == m.base.last_grad_flat.numel() + 1
    flat = m.base.last_grad_flat.detach().cpu().clone()
    torch.nn.utils.clip_grad_norm_(m.parameters(), 5.0)
    opt.step()
    w = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()
    torch.save({'grad': flat, 'weights': w, 'local': local}, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_unequal_shards_equal_single_process_global_batch(tmp_path):
    world, port = 2, 34500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(str(tmp_path / 'r0.pt')); r1 = torch.load(str(tmp_path / 'r1.pt'))
    assert torch.equal(r0['grad'], r1['grad']), 'ranks disagree after the exchange'
    assert torch.equal(r0['weights'], r1['weights']), 'replicas diverged after one step'
    # the exchange itself, through the real two-process collective: the count-weighted mean of what each rank computed alone
    check_exchange_against_local_gradients(r0['grad'], [r0['local'], r1['local']], (3, 2), 'two processes (3, 2), gloo')
    cfg, m, batch = _setup(0, 5)                            # the same 5 images in ONE process
    loss, _ = m(batch)
    loss.mean().backward()
    ref = m.base.last_grad_flat.detach().cpu()
    # different batch partition = other tile configurations = different fp32 summation order: ConvDet (no ReLU mask between it
    # and the loss) must agree tightly, the layers upstream up to the occasional mask flip (see test_training_gpu)
    ncd = m.base.convdet.weight.numel() + m.base.convdet.bias.numel()
    cd_ref, cd_got = ref[-ncd:], r0['grad'][-ncd:]
    assert float((cd_got - cd_ref).abs().max()) <= 2e-4 * float(cd_ref.abs().max())
    rel2 = float((r0['grad'] - ref).norm() / ref.norm())
    assert rel2 <= 1e-2, rel2
