"""GPU tier, two processes on one GPU (the launch pattern of tests/test_data_parallel_gpu.py): after ``attach_data_parallel`` -- which
replicates rank 0's weights and, in place, the floating-point optimizer state: both moments and the EMA are views of flat buffers in
``optimizer.state`` -- and three steps of ``FusedClipAdamW`` with the EMA on unequal shards, both ranks hold bit-identical parameters,
moments and EMA, and equal device counts.  The first step's exchanged gradient is the count-weighted mean of the two ranks' local
gradients within 2^-18 M on every element (tests/dp_exchange_ref.py)."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_data_parallel_gpu import ROOT, _local_gradient, _setup, check_exchange_against_local_gradients

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from squeezedet_pytorch_amd.trainer import FusedClipAdamW, attach_data_parallel
    lo, hi = (0, 3) if rank == 0 else (3, 5)
    cfg, m, batch = _setup(lo, hi)
    if rank == 1:                                           # other weights, hence another initial EMA; and junk in the moments
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01)
    opt = FusedClipAdamW(m.parameters(), lr=1e-4, weight_decay=1e-2, max_norm=5.0, ema_decay=0.9, ema_warmup=True,
                         flat_grad=lambda: m.base.last_grad_flat)
    if rank == 1:
        opt.exp_avg_flat.fill_(0.5); opt.exp_avg_sq_flat.fill_(0.25)
    attach_data_parallel(m, opt)
    local = _local_gradient(m, batch)                       # (on the replicated weights, before the first step)
    for it in range(3):
        loss, _ = m(batch)
        opt.zero_grad()
        loss.mean().backward()
        if it == 0:
            torch.cuda.synchronize()
            first_grad = m.base.last_grad_flat.detach().cpu().clone()
        opt.step()
    torch.cuda.synchronize()
    w = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()
    torch.save({'weights': w, 'm': opt.exp_avg_flat.cpu(), 'v': opt.exp_avg_sq_flat.cpu(), 'ema': opt.ema_flat.cpu(),
                'counts': opt.step_counts(), 'local': local, 'grad': first_grad}, os.path.join(out_dir, f'r{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_hold_identical_adamw_and_ema_state(tmp_path):
    world, port = 2, 36500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(str(tmp_path / 'r0.pt')); r1 = torch.load(str(tmp_path / 'r1.pt'))
    assert r0['counts'] == r1['counts'] == (3, 3)
    assert torch.equal(r0['grad'], r1['grad']), 'ranks disagree after the first exchange'
    check_exchange_against_local_gradients(r0['grad'], [r0['local'], r1['local']], (3, 2), 'two processes (3, 2), AdamW step 0')
    for k in ('weights', 'm', 'v', 'ema'):
        assert bool(torch.isfinite(r0[k]).all()), k
        assert torch.equal(r0[k].view(torch.int32), r1[k].view(torch.int32)), f'ranks disagree in {k} after three steps'
    assert float(r0['v'].max()) < 0.25 and not torch.equal(r0['ema'], r0['weights'])      # rank 0's state won; the average lags
