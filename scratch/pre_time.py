"""Isolated time of the uint8 -> fp32 input kernels on a resident KITTI-sized batch (20 x 375x1242 -> 384x1248).
A/B against another build of the same ABI: SQD_HIP_LIBRARY=/path/to/libsqdhip.so (see _native)."""
import sys
import numpy as np, torch
sys.path.insert(0, '.')
from squeezedet_pytorch_amd.preprocess import KITTI_RGB_MEAN, KITTI_RGB_STD, launch_u8
B, H0, W0, H, W = 20, 375, 1242, 384, 1248
rs = np.random.RandomState(0)
src = torch.from_numpy(rs.randint(0, 256, (B * H0 * W0 * 3,), dtype=np.uint8)).cuda()
off = torch.arange(B, dtype=torch.int64).cuda() * (H0 * W0 * 3)
sizes = torch.tensor([[H0, W0]] * B, dtype=torch.int32).cuda()
out = torch.empty(B, 3, H, W, device='cuda'); sc = torch.empty(B, 2, device='cuda')
def resize(): launch_u8('resize', src, off, sizes, out, B, H, W, KITTI_RGB_MEAN, KITTI_RGB_STD, out.device, scales=sc)
def padcrop(): launch_u8('padcrop', src, off, sizes, out, B, H, W, KITTI_RGB_MEAN, KITTI_RGB_STD, out.device, shifts=sc)
def letterbox(): launch_u8('letterbox', src, off, sizes, out, B, H, W, KITTI_RGB_MEAN, KITTI_RGB_STD, out.device, scales=sc)
for name, fn in (('resize', resize), ('padcrop', padcrop), ('letterbox', letterbox)):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(100): fn()
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 10
    mb = (B * H0 * W0 * 3 + B * 3 * H * W * 4) / 1e6
    print(f'{name}: {us:.1f} us per batch of {B}  ({mb:.0f} MB algorithmic -> {mb / us * 1e3:.0f} GB/s)')
