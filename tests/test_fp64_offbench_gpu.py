"""GPU tier: the float64 sweep of tests/test_fp64_launches_gpu.py away from the benchmark -- batch 1, half size, ragged grids.

The schedule (``plan.forward_schedule`` / ``backward_schedule``) decides differently at every batch and size the tuning table does not
hold: ``tiles.choose_cfg`` answers from the nearest row (without its workgroup cap) or from the cost heuristic, ``choose_fused_cfg`` turns
``fire_expand`` on, ``stem_pool_squeeze_ok`` turns the fused stem off and the split-K counts clamp to the number of pixel blocks.  Each
point below runs one inference and one training step through the same harness (same models, weights, image and ground-truth seeds,
dropout at p = 0), asserts that the launches equal the plan, and holds every output of every launch to the same two bars (L: 2^-18 M per
element; P: k times the plain fp32 chain's error, k = 2 direct, 4 Winograd), ``maxpool_fwd`` bit-exact, ``nobj`` exact, at most 4
branch-flip anchors per loss launch.

| point | grids | what it reaches |
|---|---|---|
| squeezedet b1 192x624 | 48x156, 24x78, 12x39 | the four ``fire_expand`` tilings, the three ``conv_igemm``, the batch-1 rows of the table through the nearest-row rule |
| squeezedetplus b1 192x624 | same | the 7x7 stem, the direct 3x3 kernel at SqueezeDet+ widths |
| squeezedet b3 70x100 | 17x25, 8x12, 4x6 | odd batch, partial tiles in every layer, the heuristic tilings |
| squeezedetplus b3 70x100 | same | the same for SqueezeDet+ |
| squeezedet b2 186x310 | 46x77, 23x38, 11x19 | ``stem_pool<3>`` (the unfused stem) and its training counterpart, odd widths at every level |
| squeezedet b1 48x48 | 12x12, 6x6, 3x3 | a final grid below one 4x16 Winograd weight-gradient tile group (S clamps to 1), A = 81 |

``OFFBENCH`` has one case per distinct (arch, batch, size, kernel, tag) of those plans; tests/test_fp64_coverage.py keeps it equal to the
planners and checks that every kernel name the planners can produce over a grid of batches and sizes has a case here or in the
benchmarked sweep.

Forced forms (``FORCED``): ``conv_wino_us``, ``conv_wino_vs`` and the four bridge forms run only where the table has a row, that is on
the even benchmarked grids.  One more point, squeezedet b3 70x100, runs with the look-ups of ``ops`` swapped (``forced_forms``): the planners
read the same look-ups, so the launches still equal the plan.  What the swap cannot force, by name:
* ``fire_bridge`` / ``fire_bridge_save`` beyond fire3 -> fire4: the storing form exists for configuration 12 only, which runs squeeze
  widths C <= 16 (``fire_bridge_cfg_ok``); fire6 -> fire7 (C = 32) would need configuration 10, inference only, and the later pairs
  have next-squeeze widths above 32.  The swap returns 12 or nothing, so inference and training take the same pairs.
* ``fire_pool_bridge`` / ``_save`` beyond fire4 -> pool -> fire6: ``fire_pool_bridge_ok`` needs C <= 16.
* ``conv_wino_us`` on layers with more than 128 input channels: the U-stationary LDS plan (``wino_cfg_ok``) does not fit; they run
  ``conv_wino<2,4>`` there.  ``conv_wino_vs`` has the plain bias / ReLU epilogue and N <= 80: ConvDet's forward only.

Every point here runs 3 classes on KITTI's nine anchors with a dense ground truth, so ConvDet is 72 channels wide throughout: the class /
anchor-count / sparse-gt axis, which decides ConvDet's own launches and the loss kernels, is tests/test_fp64_widths_gpu.py's, on the
backbone of the two 70x100 points here.

``test_every_compiled_tiling``: every configuration id the library compiles (``ops.cfg_table()`` / ``ops.wino_cfgs()``), whether or not a
plan names it, through ``ops.conv`` / ``ops.conv_wino`` on one small ragged shape per tap count, with and without a workgroup cap, into
a channel window of a NaN-filled buffer, against ``fp64_ref.conv`` under the same bars.
"""
import contextlib

import pytest
import torch

import fp64_ref as R
import test_fp64_launches_gpu as L

pytestmark = pytest.mark.gpu

POINTS = [
    ('squeezedet', 1, (192, 624)),
    ('squeezedetplus', 1, (192, 624)),
    ('squeezedet', 3, (70, 100)),
    ('squeezedetplus', 3, (70, 100)),
    ('squeezedet', 2, (186, 310)),
    ('squeezedet', 1, (48, 48)),
]
FORCED_POINT = ('squeezedet', 3, (70, 100))
# the families the benchmarked sweep never launches: their teeth come from their first launch at this point
NEW_FAMILIES = ['conv_igemm', 'fire_expand']
TEETH_POINT = ('squeezedet', 1, (192, 624))
# the training step's ground-truth seed per point (1 = the benchmark's; another one only where the float32 oracle chain alone exceeds
# the branch-flip cap on the point's operands)
GT_SEED = {}

POOL_BRIDGE_SEGMENTS = 3
CONVDET_WIDTH = 72          # 9 anchors x (3 classes + 5): the one layer the V-shared kernel takes


def forced_fire_bridge_cfg(C, N1, N3, Nsq, npix):
    from squeezedet_pytorch_amd import ops
    return 12 if ops.fire_bridge_cfg_ok(12, C, N3, N1, Nsq) else None


def forced_fire_pool_bridge(C, N1, N3, Nsq, npix):
    from squeezedet_pytorch_amd import ops
    return POOL_BRIDGE_SEGMENTS if ops.fire_pool_bridge_ok(C, N3, N1, Nsq) else None


def forced_wino_cfg(C, N, npix):
    """ConvDet's forward on the V-shared kernel; every other 3x3 launch on a U-stationary configuration where its LDS plan fits (the ids
    taken in turn with the input width, so that more than one runs), else on conv_wino<2,4>."""
    from squeezedet_pytorch_amd import ops
    if C % 8:
        return None
    if N == CONVDET_WIDTH:
        return ops.WINO_VS_CFG
    us = [i for i in (8, 9, 10, 11) if ops.wino_cfg_ok(i, C, N)]
    return us[(C // 16) % len(us)] if us else 2


@contextlib.contextmanager
def forced_forms():
    from squeezedet_pytorch_amd import ops, plan
    swaps = {'choose_fire_bridge_cfg': forced_fire_bridge_cfg, 'choose_fire_pool_bridge': forced_fire_pool_bridge,
             'choose_wino_cfg': forced_wino_cfg}
    saved = {n: getattr(ops, n) for n in swaps}
    plan.forward_schedule.cache_clear(); plan.backward_schedule.cache_clear()
    for n, f in swaps.items():
        setattr(ops, n, f)
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        plan.forward_schedule.cache_clear(); plan.backward_schedule.cache_clear()


# one (kernel, tag) per distinct launch of the two plans of each point, in plan order; OFFBENCH / FORCED below: (arch, batch, size, kernel, tag)
_OFFBENCH = {
    ('squeezedet', 1, (192, 624)): [
        ('stem_pool_sq<3>', 'stem+pool+squeeze 192x624 S16'), ('fire_expand<9,16,2,4,4>', 'expand C16 E64 48x156'),
        ('conv_dma<1,64,1,2,4>', '1tap C128 N16 48x156'), ('maxpool_fwd', 'pool C128 48x156'),
        ('conv_dma<1,32,1,1,4>', '1tap C128 N32 24x78'), ('fire_expand<9,16,1,4,8>', 'expand C32 E128 24x78'),
        ('conv_dma<1,64,1,2,4>', '1tap C256 N32 24x78'), ('maxpool_fwd', 'pool C256 24x78'),
        ('conv_dma<1,64,2,2,4>', '1tap C256 N48 12x39'), ('fire_expand<9,16,1,4,4>', 'expand C48 E192 12x39'),
        ('conv_dma<1,64,1,2,4>', '1tap C384 N48 12x39'), ('conv_dma<1,64,1,2,4>', '1tap C384 N64 12x39'),
        ('fire_expand<9,16,1,2,8>', 'expand C64 E256 12x39'), ('conv_dma<1,64,1,2,4>', '1tap C512 N64 12x39'),
        ('conv_dma<1,64,1,2,4>', '1tap C512 N96 12x39'), ('fire_expand<9,16,1,4,8>', 'expand C96 E384 12x39'),
        ('conv_dma<1,64,1,2,4>', '1tap C768 N96 12x39'), ('conv_dma<9,16,1,1,4>', '9tap C768 N72 12x39'),
        ('stem_pool_sq_train<3>', 'stem+pool+squeeze 192x624 S16'), ('conv_dma<1,32,4,1,4>', '1tap C16 N64 48x156'),
        ('conv_wino<2,4>', '9tap C16 N64 48x156'), ('conv_dma<1,32,2,2,8>', '1tap C32 N128 24x78'),
        ('conv_wino<1,4>', '9tap C32 N128 24x78'), ('conv_igemm<1,32,2,2>', '1tap C48 N192 12x39'),
        ('conv_dma<9,16,1,1,4>', '9tap C48 N192 12x39'), ('conv_igemm<1,32,1,3>', '1tap C64 N256 12x39'),
        ('conv_dma<9,16,1,2,4>', '9tap C64 N256 12x39'), ('conv_dma<1,32,1,2,4>', '1tap C96 N384 12x39'),
        ('conv_dma<9,16,1,3,4>', '9tap C96 N384 12x39'), ('conv_ws<6,8>', '1tap C96 N384 12x39'), ('conv_wino_sk', '9tap C96 N384 12x39'),
        ('loss_fwd', 'loss A4212'), ('loss_bwd', 'lossbwd A4212'), ('conv_wgrad_wino', 'wgrad 9tap C768 N72 12x39'),
        ('conv_wino_sk', '9tap C72 N768 12x39'), ('conv_dma<1,64,1,2,4>', '1tap C384 N96 12x39'),
        ('conv_dma<9,16,1,1,4>', '9tap C384 N96 12x39'), ('squeeze_bwd', 'sqbwd C768 N96 12x39'), ('squeeze_bwd', 'sqbwd C512 N96 12x39'),
        ('conv_dma<1,32,1,2,4>', '1tap C256 N64 12x39'), ('conv_dma<9,16,1,1,4>', '9tap C256 N64 12x39'),
        ('squeeze_bwd', 'sqbwd C512 N64 12x39'), ('conv_wgrad_group<1>', 'wgrad 1tap C96 N384 + C96 N384 + C64 N256 + C64 N256 12x39'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C96 N384 + C96 N384 + C64 N256 + C64 N256 12x39'), ('squeeze_bwd', 'sqbwd C384 N64 12x39'),
        ('conv_igemm<1,64,1,2>', '1tap C192 N48 12x39'), ('conv_dma<9,16,1,1,4>', '9tap C192 N48 12x39'),
        ('squeeze_bwd', 'sqbwd C384 N48 12x39'), ('conv_wgrad_group<1>', 'wgrad 1tap C48 N192 + C48 N192 12x39'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C48 N192 + C48 N192 12x39'), ('squeeze_bwd', 'sqbwd C256 N48 12x39'),
        ('maxpool_bwd', 'poolbwd C256 24x78'), ('squeeze_bwd', 'sqbwd C32 N128 24x78'), ('conv_dma<9,16,1,1,4>', '9tap C128 N32 24x78'),
        ('squeeze_bwd', 'sqbwd C256 N32 24x78'), ('conv_wgrad_wino_group', 'wgrad 9tap C32 N128 + C32 N128 24x78'),
        ('squeeze_bwd', 'sqbwd C128 N32 24x78'), ('maxpool_bwd', 'poolbwd C128 48x156'), ('squeeze_bwd', 'sqbwd C16 N64 48x156'),
        ('conv_dma<9,16,2,1,4>', '9tap C64 N16 48x156'), ('squeeze_bwd', 'sqbwd C128 N16 48x156'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C16 N64 + C16 N64 48x156'), ('squeeze_bwd', 'sqbwd C64 N16 48x156'),
        ('stem_wgrad_pooled<3>', 'stem wgrad (pooled) 192x624'), ('wgrad_reduce_batched', '31 layers'),
    ],
    ('squeezedetplus', 1, (192, 624)): [
        ('stem_pool<7>', 'stem+pool 192x624'), ('conv_dma<1,32,1,6,4>', '1tap C96 N96 48x156'),
        ('conv_dma<1,32,1,4,4>', '1tap C96 N64 48x156'), ('conv_dma<9,16,1,4,4>', '9tap C96 N64 48x156'),
        ('conv_dma<1,32,1,6,4>', '1tap C128 N96 48x156'), ('conv_dma<1,32,1,6,4>', '1tap C128 N192 48x156'),
        ('conv_dma<1,32,1,4,4>', '1tap C192 N128 48x156'), ('conv_dma<9,16,1,4,4>', '9tap C192 N128 48x156'),
        ('maxpool_fwd', 'pool C256 48x156'), ('conv_dma<1,32,1,6,4>', '1tap C256 N192 24x78'),
        ('conv_dma<1,32,1,4,4>', '1tap C192 N128 24x78'), ('conv_dma<9,16,1,4,4>', '9tap C192 N128 24x78'),
        ('conv_dma<1,32,1,6,4>', '1tap C256 N288 24x78'), ('conv_dma<1,32,1,6,4>', '1tap C288 N192 24x78'),
        ('conv_dma<9,16,1,4,4>', '9tap C288 N192 24x78'), ('conv_dma<1,32,1,6,4>', '1tap C384 N288 24x78'),
        ('conv_dma<1,32,1,6,4>', '1tap C384 N384 24x78'), ('conv_dma<1,32,1,4,4>', '1tap C384 N256 24x78'),
        ('conv_dma<9,16,1,4,4>', '9tap C384 N256 24x78'), ('maxpool_fwd', 'pool C512 24x78'),
        ('conv_dma<1,32,1,6,4>', '1tap C512 N384 12x39'), ('conv_dma<1,32,1,4,4>', '1tap C384 N256 12x39'),
        ('conv_dma<9,16,1,4,4>', '9tap C384 N256 12x39'), ('conv_dma<9,16,1,1,4>', '9tap C512 N72 12x39'),
        ('conv_ws<4,8>', '1tap C384 N256 12x39'), ('conv_wino_sk', '9tap C384 N256 12x39'), ('loss_fwd', 'loss A4212'),
        ('loss_bwd', 'lossbwd A4212'), ('conv_wgrad_wino', 'wgrad 9tap C512 N72 12x39'), ('conv_wino_sk', '9tap C72 N512 12x39'),
        ('conv_dma<1,32,1,6,4>', '1tap C256 N384 12x39'), ('conv_dma<9,16,1,4,4>', '9tap C256 N384 12x39'),
        ('conv_wgrad<1>', 'wgrad 1tap C512 N384 12x39'), ('conv_dma<1,32,1,4,4>', '1tap C384 N512 12x39'),
        ('conv_wgrad_group<1>', 'wgrad 1tap C384 N256 + C384 N256 + C384 N256 12x39'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C384 N256 + C384 N256 + C384 N256 12x39'), ('maxpool_bwd', 'poolbwd C512 24x78'),
        ('conv_dma<1,32,1,6,4>', '1tap C256 N384 24x78'), ('conv_dma<9,16,1,4,4>', '9tap C256 N384 24x78'),
        ('conv_wgrad<1>', 'wgrad 1tap C384 N384 24x78'), ('conv_dma<1,32,1,6,4>', '1tap C192 N288 24x78'),
        ('conv_dma<9,16,1,3,4>', '9tap C192 N288 24x78'), ('conv_wgrad<1>', 'wgrad 1tap C384 N288 24x78'),
        ('conv_dma<1,32,1,6,4>', '1tap C288 N384 24x78'), ('conv_wgrad_group<1>', 'wgrad 1tap C384 N256 + C288 N192 + C288 N192 24x78'),
        ('conv_wgrad<1>', 'wgrad 1tap C256 N288 24x78'), ('conv_dma<1,32,1,4,4>', '1tap C288 N256 24x78'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C384 N256 + C288 N192 + C288 N192 + C192 N128 24x78'),
        ('squeeze_bwd', 'sqbwd C192 N128 24x78'), ('conv_dma<9,16,1,4,4>', '9tap C128 N192 24x78'),
        ('conv_wgrad<1>', 'wgrad 1tap C256 N192 24x78'), ('conv_dma<1,32,1,4,4>', '1tap C192 N256 24x78'),
        ('maxpool_bwd', 'poolbwd C256 48x156'), ('squeeze_bwd', 'sqbwd C192 N128 48x156'),
        ('conv_dma<9,16,1,4,4>', '9tap C128 N192 48x156'), ('conv_wgrad<1>', 'wgrad 1tap C128 N192 48x156'),
        ('squeeze_bwd', 'sqbwd C96 N64 48x156'), ('conv_dma<9,16,1,3,4>', '9tap C64 N96 48x156'), ('squeeze_bwd', 'sqbwd C128 N96 48x156'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C192 N128 + C96 N64 + C96 N64 48x156'), ('squeeze_bwd', 'sqbwd C96 N96 48x156'),
        ('stem_wgrad_pooled<7>', 'stem wgrad (pooled) 192x624'), ('wgrad_reduce_batched', '31 layers'),
    ],
    ('squeezedet', 3, (70, 100)): [
        ('stem_pool_sq<3>', 'stem+pool+squeeze 70x100 S16'), ('conv_dma<1,16,1,4,4>', '1tap C16 N64 17x25'),
        ('conv_dma<9,16,1,4,4>', '9tap C16 N64 17x25'), ('conv_dma<1,32,1,1,4>', '1tap C128 N16 17x25'), ('maxpool_fwd', 'pool C128 17x25'),
        ('conv_dma<1,32,1,2,4>', '1tap C128 N32 8x12'), ('conv_dma<1,16,1,4,4>', '1tap C32 N128 8x12'),
        ('conv_dma<9,16,1,4,4>', '9tap C32 N128 8x12'), ('conv_dma<1,32,1,2,4>', '1tap C256 N32 8x12'), ('maxpool_fwd', 'pool C256 8x12'),
        ('conv_dma<1,32,1,3,4>', '1tap C256 N48 4x6'), ('conv_dma<1,16,1,4,4>', '1tap C48 N192 4x6'),
        ('conv_dma<9,16,1,4,4>', '9tap C48 N192 4x6'), ('conv_dma<1,32,1,3,4>', '1tap C384 N48 4x6'),
        ('conv_dma<1,32,1,4,4>', '1tap C384 N64 4x6'), ('conv_dma<1,32,1,4,4>', '1tap C64 N256 4x6'),
        ('conv_dma<9,16,1,4,4>', '9tap C64 N256 4x6'), ('conv_dma<1,32,1,4,4>', '1tap C512 N64 4x6'),
        ('conv_dma<1,32,1,6,4>', '1tap C512 N96 4x6'), ('conv_dma<1,32,1,6,4>', '1tap C96 N384 4x6'),
        ('conv_dma<9,16,1,4,4>', '9tap C96 N384 4x6'), ('conv_dma<1,32,1,6,4>', '1tap C768 N96 4x6'),
        ('conv_dma<9,16,1,1,4>', '9tap C768 N72 4x6'), ('stem_pool_sq_train<3>', 'stem+pool+squeeze 70x100 S16'),
        ('conv_ws<6,8>', '1tap C96 N384 4x6'), ('conv_wino_sk', '9tap C96 N384 4x6'), ('loss_fwd', 'loss A216'),
        ('loss_bwd', 'lossbwd A216'), ('conv_wgrad_wino', 'wgrad 9tap C768 N72 4x6'), ('conv_wino_sk', '9tap C72 N768 4x6'),
        ('conv_dma<1,32,1,6,4>', '1tap C384 N96 4x6'), ('conv_dma<9,16,1,3,4>', '9tap C384 N96 4x6'), ('squeeze_bwd', 'sqbwd C768 N96 4x6'),
        ('squeeze_bwd', 'sqbwd C512 N96 4x6'), ('conv_dma<1,32,1,4,4>', '1tap C256 N64 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C256 N64 4x6'),
        ('squeeze_bwd', 'sqbwd C512 N64 4x6'), ('conv_wgrad_group<1>', 'wgrad 1tap C96 N384 + C96 N384 + C64 N256 + C64 N256 4x6'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C96 N384 + C96 N384 + C64 N256 + C64 N256 4x6'), ('squeeze_bwd', 'sqbwd C384 N64 4x6'),
        ('conv_dma<1,32,1,3,4>', '1tap C192 N48 4x6'), ('conv_dma<9,16,1,3,4>', '9tap C192 N48 4x6'), ('squeeze_bwd', 'sqbwd C384 N48 4x6'),
        ('conv_wgrad_group<1>', 'wgrad 1tap C48 N192 + C48 N192 4x6'), ('conv_wgrad_wino_group', 'wgrad 9tap C48 N192 + C48 N192 4x6'),
        ('squeeze_bwd', 'sqbwd C256 N48 4x6'), ('maxpool_bwd', 'poolbwd C256 8x12'), ('squeeze_bwd', 'sqbwd C32 N128 8x12'),
        ('conv_dma<9,16,1,2,4>', '9tap C128 N32 8x12'), ('squeeze_bwd', 'sqbwd C256 N32 8x12'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C32 N128 + C32 N128 8x12'), ('squeeze_bwd', 'sqbwd C128 N32 8x12'),
        ('maxpool_bwd', 'poolbwd C128 17x25'), ('squeeze_bwd', 'sqbwd C16 N64 17x25'), ('conv_dma<9,16,1,1,4>', '9tap C64 N16 17x25'),
        ('squeeze_bwd', 'sqbwd C128 N16 17x25'), ('conv_wgrad_wino_group', 'wgrad 9tap C16 N64 + C16 N64 17x25'),
        ('squeeze_bwd', 'sqbwd C64 N16 17x25'), ('stem_wgrad_pooled<3>', 'stem wgrad (pooled) 70x100'),
        ('wgrad_reduce_batched', '31 layers'),
    ],
    ('squeezedetplus', 3, (70, 100)): [
        ('stem_pool<7>', 'stem+pool 70x100'), ('conv_dma<1,32,1,6,4>', '1tap C96 N96 17x25'),
        ('conv_dma<1,32,1,4,4>', '1tap C96 N64 17x25'), ('conv_dma<9,16,1,4,4>', '9tap C96 N64 17x25'),
        ('conv_dma<1,32,1,6,4>', '1tap C128 N96 17x25'), ('conv_dma<1,32,1,6,4>', '1tap C128 N192 17x25'),
        ('conv_dma<1,32,1,4,4>', '1tap C192 N128 17x25'), ('conv_dma<9,16,1,4,4>', '9tap C192 N128 17x25'),
        ('maxpool_fwd', 'pool C256 17x25'), ('conv_dma<1,32,1,6,4>', '1tap C256 N192 8x12'),
        ('conv_dma<1,32,1,4,4>', '1tap C192 N128 8x12'), ('conv_dma<9,16,1,4,4>', '9tap C192 N128 8x12'),
        ('conv_dma<1,32,1,6,4>', '1tap C256 N288 8x12'), ('conv_dma<1,32,1,6,4>', '1tap C288 N192 8x12'),
        ('conv_dma<9,16,1,4,4>', '9tap C288 N192 8x12'), ('conv_dma<1,32,1,6,4>', '1tap C384 N288 8x12'),
        ('conv_dma<1,32,1,6,4>', '1tap C384 N384 8x12'), ('conv_dma<1,32,1,4,4>', '1tap C384 N256 8x12'),
        ('conv_dma<9,16,1,4,4>', '9tap C384 N256 8x12'), ('maxpool_fwd', 'pool C512 8x12'), ('conv_dma<1,32,1,6,4>', '1tap C512 N384 4x6'),
        ('conv_dma<1,32,1,4,4>', '1tap C384 N256 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C384 N256 4x6'),
        ('conv_dma<9,16,1,1,4>', '9tap C512 N72 4x6'), ('conv_ws<4,8>', '1tap C384 N256 4x6'), ('conv_wino_sk', '9tap C384 N256 4x6'),
        ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'), ('conv_wgrad_wino', 'wgrad 9tap C512 N72 4x6'),
        ('conv_wino_sk', '9tap C72 N512 4x6'), ('conv_dma<1,32,1,6,4>', '1tap C256 N384 4x6'),
        ('conv_dma<9,16,1,4,4>', '9tap C256 N384 4x6'), ('conv_wgrad<1>', 'wgrad 1tap C512 N384 4x6'),
        ('conv_dma<1,32,1,4,4>', '1tap C384 N512 4x6'), ('conv_wgrad_group<1>', 'wgrad 1tap C384 N256 + C384 N256 + C384 N256 4x6'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C384 N256 + C384 N256 + C384 N256 4x6'), ('maxpool_bwd', 'poolbwd C512 8x12'),
        ('conv_dma<1,32,1,6,4>', '1tap C256 N384 8x12'), ('conv_dma<9,16,1,4,4>', '9tap C256 N384 8x12'),
        ('conv_wgrad<1>', 'wgrad 1tap C384 N384 8x12'), ('conv_dma<1,32,1,6,4>', '1tap C192 N288 8x12'),
        ('conv_dma<9,16,1,3,4>', '9tap C192 N288 8x12'), ('conv_wgrad<1>', 'wgrad 1tap C384 N288 8x12'),
        ('conv_dma<1,32,1,6,4>', '1tap C288 N384 8x12'), ('conv_wgrad_group<1>', 'wgrad 1tap C384 N256 + C288 N192 + C288 N192 8x12'),
        ('conv_wgrad<1>', 'wgrad 1tap C256 N288 8x12'), ('conv_dma<1,32,1,4,4>', '1tap C288 N256 8x12'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C384 N256 + C288 N192 + C288 N192 + C192 N128 8x12'), ('squeeze_bwd', 'sqbwd C192 N128 8x12'),
        ('conv_dma<9,16,1,4,4>', '9tap C128 N192 8x12'), ('conv_wgrad<1>', 'wgrad 1tap C256 N192 8x12'),
        ('conv_dma<1,32,1,4,4>', '1tap C192 N256 8x12'), ('maxpool_bwd', 'poolbwd C256 17x25'), ('squeeze_bwd', 'sqbwd C192 N128 17x25'),
        ('conv_dma<9,16,1,4,4>', '9tap C128 N192 17x25'), ('conv_wgrad<1>', 'wgrad 1tap C128 N192 17x25'),
        ('squeeze_bwd', 'sqbwd C96 N64 17x25'), ('conv_dma<9,16,1,3,4>', '9tap C64 N96 17x25'), ('squeeze_bwd', 'sqbwd C128 N96 17x25'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C192 N128 + C96 N64 + C96 N64 17x25'), ('squeeze_bwd', 'sqbwd C96 N96 17x25'),
        ('stem_wgrad_pooled<7>', 'stem wgrad (pooled) 70x100'), ('wgrad_reduce_batched', '31 layers'),
    ],
    ('squeezedet', 2, (186, 310)): [
        ('stem_pool<3>', 'stem+pool 186x310'), ('conv_dma<1,32,1,1,4>', '1tap C64 N16 46x77'),
        ('conv_dma<1,16,1,4,4>', '1tap C16 N64 46x77'), ('conv_dma<9,16,1,4,4>', '9tap C16 N64 46x77'),
        ('conv_dma<1,32,1,1,4>', '1tap C128 N16 46x77'), ('maxpool_fwd', 'pool C128 46x77'),
        ('conv_dma<1,32,1,2,4>', '1tap C128 N32 23x38'), ('conv_dma<1,16,1,4,4>', '1tap C32 N128 23x38'),
        ('conv_dma<9,16,1,4,4>', '9tap C32 N128 23x38'), ('conv_dma<1,32,1,2,4>', '1tap C256 N32 23x38'),
        ('maxpool_fwd', 'pool C256 23x38'), ('conv_dma<1,32,1,3,4>', '1tap C256 N48 11x19'),
        ('conv_dma<1,16,1,4,4>', '1tap C48 N192 11x19'), ('conv_dma<9,16,1,4,4>', '9tap C48 N192 11x19'),
        ('conv_dma<1,32,1,3,4>', '1tap C384 N48 11x19'), ('conv_dma<1,32,1,4,4>', '1tap C384 N64 11x19'),
        ('conv_dma<1,32,1,4,4>', '1tap C64 N256 11x19'), ('conv_dma<9,16,1,4,4>', '9tap C64 N256 11x19'),
        ('conv_dma<1,32,1,4,4>', '1tap C512 N64 11x19'), ('conv_dma<1,32,1,6,4>', '1tap C512 N96 11x19'),
        ('conv_dma<1,32,1,6,4>', '1tap C96 N384 11x19'), ('conv_dma<9,16,1,4,4>', '9tap C96 N384 11x19'),
        ('conv_dma<1,32,1,6,4>', '1tap C768 N96 11x19'), ('conv_dma<9,16,1,1,4>', '9tap C768 N72 11x19'),
        ('conv_ws<6,8>', '1tap C96 N384 11x19'), ('conv_wino_sk', '9tap C96 N384 11x19'), ('loss_fwd', 'loss A1881'),
        ('loss_bwd', 'lossbwd A1881'), ('conv_wgrad_wino', 'wgrad 9tap C768 N72 11x19'), ('conv_wino_sk', '9tap C72 N768 11x19'),
        ('conv_dma<1,32,1,6,4>', '1tap C384 N96 11x19'), ('conv_dma<9,16,1,3,4>', '9tap C384 N96 11x19'),
        ('squeeze_bwd', 'sqbwd C768 N96 11x19'), ('squeeze_bwd', 'sqbwd C512 N96 11x19'), ('conv_dma<1,32,1,4,4>', '1tap C256 N64 11x19'),
        ('conv_dma<9,16,1,4,4>', '9tap C256 N64 11x19'), ('squeeze_bwd', 'sqbwd C512 N64 11x19'),
        ('conv_wgrad_group<1>', 'wgrad 1tap C96 N384 + C96 N384 + C64 N256 + C64 N256 11x19'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C96 N384 + C96 N384 + C64 N256 + C64 N256 11x19'), ('squeeze_bwd', 'sqbwd C384 N64 11x19'),
        ('conv_dma<1,32,1,3,4>', '1tap C192 N48 11x19'), ('conv_dma<9,16,1,3,4>', '9tap C192 N48 11x19'),
        ('squeeze_bwd', 'sqbwd C384 N48 11x19'), ('conv_wgrad_group<1>', 'wgrad 1tap C48 N192 + C48 N192 11x19'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C48 N192 + C48 N192 11x19'), ('squeeze_bwd', 'sqbwd C256 N48 11x19'),
        ('maxpool_bwd', 'poolbwd C256 23x38'), ('squeeze_bwd', 'sqbwd C32 N128 23x38'), ('conv_dma<9,16,1,2,4>', '9tap C128 N32 23x38'),
        ('squeeze_bwd', 'sqbwd C256 N32 23x38'), ('conv_wgrad_wino_group', 'wgrad 9tap C32 N128 + C32 N128 23x38'),
        ('squeeze_bwd', 'sqbwd C128 N32 23x38'), ('maxpool_bwd', 'poolbwd C128 46x77'), ('squeeze_bwd', 'sqbwd C16 N64 46x77'),
        ('conv_dma<9,16,1,1,4>', '9tap C64 N16 46x77'), ('squeeze_bwd', 'sqbwd C128 N16 46x77'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C16 N64 + C16 N64 46x77'), ('squeeze_bwd', 'sqbwd C64 N16 46x77'),
        ('stem_wgrad_pooled<3>', 'stem wgrad (pooled) 186x310'), ('wgrad_reduce_batched', '31 layers'),
    ],
    ('squeezedet', 1, (48, 48)): [
        ('stem_pool_sq<3>', 'stem+pool+squeeze 48x48 S16'), ('conv_dma<1,16,1,4,4>', '1tap C16 N64 12x12'),
        ('conv_dma<9,16,1,4,4>', '9tap C16 N64 12x12'), ('conv_dma<1,32,1,1,4>', '1tap C128 N16 12x12'), ('maxpool_fwd', 'pool C128 12x12'),
        ('conv_dma<1,32,1,2,4>', '1tap C128 N32 6x6'), ('conv_dma<1,16,1,4,4>', '1tap C32 N128 6x6'),
        ('conv_dma<9,16,1,4,4>', '9tap C32 N128 6x6'), ('conv_dma<1,32,1,2,4>', '1tap C256 N32 6x6'), ('maxpool_fwd', 'pool C256 6x6'),
        ('conv_dma<1,32,1,3,4>', '1tap C256 N48 3x3'), ('conv_dma<1,16,1,4,4>', '1tap C48 N192 3x3'),
        ('conv_dma<9,16,1,4,4>', '9tap C48 N192 3x3'), ('conv_dma<1,32,1,3,4>', '1tap C384 N48 3x3'),
        ('conv_dma<1,32,1,4,4>', '1tap C384 N64 3x3'), ('conv_dma<1,32,1,4,4>', '1tap C64 N256 3x3'),
        ('conv_dma<9,16,1,4,4>', '9tap C64 N256 3x3'), ('conv_dma<1,32,1,4,4>', '1tap C512 N64 3x3'),
        ('conv_dma<1,32,1,6,4>', '1tap C512 N96 3x3'), ('conv_dma<1,32,1,6,4>', '1tap C96 N384 3x3'),
        ('conv_dma<9,16,1,4,4>', '9tap C96 N384 3x3'), ('conv_dma<1,32,1,6,4>', '1tap C768 N96 3x3'),
        ('conv_dma<9,16,1,1,4>', '9tap C768 N72 3x3'), ('stem_pool_sq_train<3>', 'stem+pool+squeeze 48x48 S16'),
        ('conv_ws<6,8>', '1tap C96 N384 3x3'), ('conv_wino_sk', '9tap C96 N384 3x3'), ('loss_fwd', 'loss A81'), ('loss_bwd', 'lossbwd A81'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N72 3x3'), ('conv_wino_sk', '9tap C72 N768 3x3'),
        ('conv_dma<1,32,1,6,4>', '1tap C384 N96 3x3'), ('conv_dma<9,16,1,3,4>', '9tap C384 N96 3x3'), ('squeeze_bwd', 'sqbwd C768 N96 3x3'),
        ('squeeze_bwd', 'sqbwd C512 N96 3x3'), ('conv_dma<1,32,1,4,4>', '1tap C256 N64 3x3'), ('conv_dma<9,16,1,4,4>', '9tap C256 N64 3x3'),
        ('squeeze_bwd', 'sqbwd C512 N64 3x3'), ('conv_wgrad_group<1>', 'wgrad 1tap C96 N384 + C96 N384 + C64 N256 + C64 N256 3x3'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C96 N384 + C96 N384 + C64 N256 + C64 N256 3x3'), ('squeeze_bwd', 'sqbwd C384 N64 3x3'),
        ('conv_dma<1,32,1,3,4>', '1tap C192 N48 3x3'), ('conv_dma<9,16,1,3,4>', '9tap C192 N48 3x3'), ('squeeze_bwd', 'sqbwd C384 N48 3x3'),
        ('conv_wgrad_group<1>', 'wgrad 1tap C48 N192 + C48 N192 3x3'), ('conv_wgrad_wino_group', 'wgrad 9tap C48 N192 + C48 N192 3x3'),
        ('squeeze_bwd', 'sqbwd C256 N48 3x3'), ('maxpool_bwd', 'poolbwd C256 6x6'), ('squeeze_bwd', 'sqbwd C32 N128 6x6'),
        ('conv_dma<9,16,1,2,4>', '9tap C128 N32 6x6'), ('squeeze_bwd', 'sqbwd C256 N32 6x6'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C32 N128 + C32 N128 6x6'), ('squeeze_bwd', 'sqbwd C128 N32 6x6'),
        ('maxpool_bwd', 'poolbwd C128 12x12'), ('squeeze_bwd', 'sqbwd C16 N64 12x12'), ('conv_dma<9,16,1,1,4>', '9tap C64 N16 12x12'),
        ('squeeze_bwd', 'sqbwd C128 N16 12x12'), ('conv_wgrad_wino_group', 'wgrad 9tap C16 N64 + C16 N64 12x12'),
        ('squeeze_bwd', 'sqbwd C64 N16 12x12'), ('stem_wgrad_pooled<3>', 'stem wgrad (pooled) 48x48'),
        ('wgrad_reduce_batched', '31 layers'),
    ],
}
_FORCED = {
    ('squeezedet', 3, (70, 100)): [
        ('stem_pool_sq<3>', 'stem+pool+squeeze 70x100 S16'), ('fire_bridge', 'fire C16 E64+64 -> S16 17x25'),
        ('fire_pool_bridge', 'fire C16 E64+64 -> pool -> S32 17x25'), ('conv_dma<1,16,1,4,4>', '1tap C32 N128 8x12'),
        ('conv_wino_us<2,4>', '9tap C32 N128 8x12'), ('conv_dma<1,32,1,2,4>', '1tap C256 N32 8x12'), ('maxpool_fwd', 'pool C256 8x12'),
        ('conv_dma<1,32,1,3,4>', '1tap C256 N48 4x6'), ('conv_dma<1,16,1,4,4>', '1tap C48 N192 4x6'),
        ('conv_wino_us<1,4>', '9tap C48 N192 4x6'), ('conv_dma<1,32,1,3,4>', '1tap C384 N48 4x6'),
        ('conv_dma<1,32,1,4,4>', '1tap C384 N64 4x6'), ('conv_dma<1,32,1,4,4>', '1tap C64 N256 4x6'),
        ('conv_wino_us<2,4>', '9tap C64 N256 4x6'), ('conv_dma<1,32,1,4,4>', '1tap C512 N64 4x6'),
        ('conv_dma<1,32,1,6,4>', '1tap C512 N96 4x6'), ('conv_dma<1,32,1,6,4>', '1tap C96 N384 4x6'),
        ('conv_wino_us<1,8>', '9tap C96 N384 4x6'), ('conv_dma<1,32,1,6,4>', '1tap C768 N96 4x6'), ('conv_wino_vs', '9tap C768 N72 4x6'),
        ('stem_pool_sq_train<3>', 'stem+pool+squeeze 70x100 S16'), ('fire_bridge_save', 'fire C16 E64+64 -> S16 17x25'),
        ('fire_pool_bridge_save', 'fire C16 E64+64 -> pool -> S32 17x25'), ('conv_ws<6,8>', '1tap C96 N384 4x6'),
        ('conv_wino_sk', '9tap C96 N384 4x6'), ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N72 4x6'), ('conv_wino_sk', '9tap C72 N768 4x6'),
        ('conv_dma<1,32,1,6,4>', '1tap C384 N96 4x6'), ('conv_wino<2,4>', '9tap C384 N96 4x6'), ('squeeze_bwd', 'sqbwd C768 N96 4x6'),
        ('squeeze_bwd', 'sqbwd C512 N96 4x6'), ('conv_dma<1,32,1,4,4>', '1tap C256 N64 4x6'), ('conv_wino<2,4>', '9tap C256 N64 4x6'),
        ('squeeze_bwd', 'sqbwd C512 N64 4x6'), ('conv_wgrad_group<1>', 'wgrad 1tap C96 N384 + C96 N384 + C64 N256 + C64 N256 4x6'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C96 N384 + C96 N384 + C64 N256 + C64 N256 4x6'), ('squeeze_bwd', 'sqbwd C384 N64 4x6'),
        ('conv_dma<1,32,1,3,4>', '1tap C192 N48 4x6'), ('conv_wino<2,4>', '9tap C192 N48 4x6'), ('squeeze_bwd', 'sqbwd C384 N48 4x6'),
        ('conv_wgrad_group<1>', 'wgrad 1tap C48 N192 + C48 N192 4x6'), ('conv_wgrad_wino_group', 'wgrad 9tap C48 N192 + C48 N192 4x6'),
        ('squeeze_bwd', 'sqbwd C256 N48 4x6'), ('maxpool_bwd', 'poolbwd C256 8x12'), ('squeeze_bwd', 'sqbwd C32 N128 8x12'),
        ('conv_wino_us<1,4>', '9tap C128 N32 8x12'), ('squeeze_bwd', 'sqbwd C256 N32 8x12'),
        ('conv_wgrad_wino_group', 'wgrad 9tap C32 N128 + C32 N128 8x12'), ('squeeze_bwd', 'sqbwd C128 N32 8x12'),
        ('maxpool_bwd', 'poolbwd C128 17x25'), ('squeeze_bwd', 'sqbwd C16 N64 17x25'), ('conv_wino_us<2,4>', '9tap C64 N16 17x25'),
        ('squeeze_bwd', 'sqbwd C128 N16 17x25'), ('conv_wgrad_wino_group', 'wgrad 9tap C16 N64 + C16 N64 17x25'),
        ('squeeze_bwd', 'sqbwd C64 N16 17x25'), ('stem_wgrad_pooled<3>', 'stem wgrad (pooled) 70x100'),
        ('wgrad_reduce_batched', '31 layers'),
    ],
}


def _flat(d):
    return [pt + e for pt, lst in d.items() for e in lst]


OFFBENCH = _flat(_OFFBENCH)
FORCED = _flat(_FORCED)


def _results(arch, batch, size, swap=None):
    return L._step_results(arch, batch, size, swap=swap, gt_seed=GT_SEED.get((arch, batch, size), 1), teeth_for=NEW_FAMILIES)


def _case_id(c):
    return f'{c[0]}-b{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]}-{c[4]}'


def _assert_case(case, swap=None):
    arch, batch, size, kernel, tag = case
    rows, _ = _results(arch, batch, size, swap)
    entry = (arch, batch, kernel, tag)
    assert entry in rows, f'{case} did not run in the step (fallback or plan drift)'
    outs = rows[entry]
    print(_summary(case, outs))
    bad = [(name, b) for name, b in outs if not (b['l_ok'] and b['p_ok'])]
    assert not bad, bad


def _summary(case, outs):
    """One line per case: the number of outputs the launch wrote and the largest attained ratios over them (with the output that
    attains the largest block ratio); a failing case lists every failing output with all its figures in the assertion."""
    head = f'{case[2][0]}x{case[2][1]} {case[0]} b{case[1]} {case[3]} | {case[4]} | {len(outs)} out'
    num = [(n, b) for n, b in outs if 'exact' not in b]
    tail = ''.join(f'  {n} ' + (f'branch flips {b["flips"]} (at most 4)' if 'flips' in b else f'exact={b["exact"]}')
                   for n, b in outs if 'exact' in b)
    if not num:
        return head + tail
    worst = max(num, key=lambda nb: nb[1]['p_block'])
    k = worst[1]['k']
    return (head + f'  max err/M {max(b["l_ratio"] for _n, b in num):.2e}  P block {worst[1]["p_block"]:.2f} ({worst[0]})  '
            f'P tensor {max(b["p_tensor"] for _n, b in num):.2f}  (k {k}, 2k {2 * k})' + tail)


@pytest.mark.parametrize('case', OFFBENCH, ids=[_case_id(c) for c in OFFBENCH])
def test_offbench_launch_against_fp64(case):
    """The planned (kernel, tag) ran in the point's step, and every output it wrote holds bars L and P (or is bit-exact)."""
    _assert_case(case)


@pytest.mark.parametrize('case', FORCED, ids=['forced-' + _case_id(c) for c in FORCED])
def test_forced_form_against_fp64(case):
    """The same at the forced-forms point: the bridges, the U-stationary and the V-shared Winograd kernels on a ragged grid."""
    assert case[:3] == FORCED_POINT
    _assert_case(case, forced_forms)


@pytest.mark.parametrize('fam,emu', [(f, e) for f in NEW_FAMILIES for e in ('bf16', 'split3')])
def test_teeth_bar_p_rejects_degraded_emulations_new_families(fam, emu):
    """Bar P tells the fp32 kernels of the two families that only run off the benchmark from reduced-precision ones: their first launch at
    192x624, batch 1, recomputed with bf16-rounded operands and with the 3-product bf16 split instead of the kernel, fails it."""
    t = _results(*TEETH_POINT)[1].get(fam)
    assert t is not None, f'no launch of family {fam} at {TEETH_POINT}'
    b = t[emu]
    print(f'teeth {fam:24s} {emu:7s} P block {b["p_block"]:9.2f}  P tensor {b["p_tensor"]:9.2f}  (k {b["k"]})')
    assert not b['p_ok'], (fam, emu, b)


# ---- every compiled tiling on one small ragged shape per tap count ----

# (taps, C, N, B, H, W): 1 tap: 231 pixels, no multiple of any pixel tile, N no multiple of any slice width; 9 tap and Winograd: rows % 4
# != 0, columns % 16 != 0, N <= 80 so that the V-shared kernel applies
TILING_SHAPES = {1: (96, 72, 3, 7, 11), 9: (48, 72, 2, 5, 17)}
WINDOW_OFF, WINDOW_PAD = 8, 16             # the output goes to channels [8, 8 + N) of a buffer N + 16 wide
CAP = 2000                                 # + 1000 k: at most k workgroups per CU


def _operands(taps):
    C, N, B, H, W = TILING_SHAPES[taps]
    k = 3 if taps == 9 else 1
    g = torch.Generator().manual_seed(100 + taps)
    x = torch.randn(B, H, W, C, generator=g).clamp_min(0).cuda()
    w = (torch.randn(N, C, k, k, generator=g) * (2.0 / (C * taps)) ** 0.5).cuda()
    b = (torch.randn(N, generator=g) * 0.1).cuda()
    return x, w, b


_TILING_REFS = {}


def _tiling_ref(taps, chain_kc):
    """``chain_kc``: the chunk width of a direct configuration (its float32 chain restates the kernels' single accumulator); None:
    the plain chain (the Winograd kernels)."""
    if (taps, chain_kc) not in _TILING_REFS:
        x, w, b = _operands(taps)
        _TILING_REFS[taps, chain_kc] = (x, w, b, R.conv(x, w, b, relu=True, chain_kc=chain_kc))
    return _TILING_REFS[taps, chain_kc]


def _run_tiling(launch, taps, name, k, chain_kc=None):
    x, w, b, ref = _tiling_ref(taps, chain_kc)
    N = w.shape[0]
    y = torch.full(tuple(x.shape[:3]) + (N + WINDOW_PAD,), float('nan'), device='cuda')
    launch(x, w, b, y)
    torch.cuda.synchronize()
    outside = torch.cat([y[..., :WINDOW_OFF], y[..., WINDOW_OFF + N:]], -1)
    assert bool(torch.isnan(outside).all()), f'{name}: wrote outside its channel window'
    got = y[..., WINDOW_OFF:WINDOW_OFF + N]
    assert not bool(torch.isnan(got).any()), f'{name}: left part of its channel window unwritten'
    bars = R.bars(got, ref, 'act', k)
    return bars['l_ok'] and bars['p_ok'], f'err/M {bars["l_ratio"]:.2e} P block {bars["p_block"]:.2f} P tensor {bars["p_tensor"]:.2f}'


def test_every_compiled_tiling():
    """Every configuration id the library compiles runs a ragged layer right, inside its channel window: the direct families through
    ``ops.conv`` (k = 2), the Winograd ones through ``ops.conv_wino`` (k = 4), each once more under a workgroup cap."""
    from squeezedet_pytorch_amd import ops
    bad, ran = [], set()

    def both(cid, name, taps, k, chain_kc, launch):
        res = [_run_tiling(lambda x, w, b, y: launch(cfg, x, w, b, y), taps, f'{name} cfg {cfg}', k, chain_kc) for cfg in (cid, cid + CAP)]
        print(f'cfg {cid:2d} {name:22s} {res[0][1]} | capped: {res[1][1]}  (k {k})')
        ran.add(name)
        if not (res[0][0] and res[1][0]):
            bad.append((cid, name))
    for cid, (taps, kc, _px, _bn) in sorted(ops.cfg_table().items()):
        if ops.conv_cfg_ok(cid, TILING_SHAPES[taps][0]):
            both(cid, ops.cfg_kernel_name(cid), taps, 2, kc,
                 lambda cfg, x, w, b, y: ops.conv(x, 0, ops.ConvPlan(w, b, cfg), y, WINDOW_OFF, relu=True))
    C, N = TILING_SHAPES[9][:2]
    for cid in sorted(ops.wino_cfgs()):
        if ops.wino_cfg_ok(cid, C, N):
            both(cid, ops.wino_kernel_name(cid), 9, 4, None,
                 lambda cfg, x, w, b, y: ops.conv_wino(x, 0, ops.WinoPlan(w, b, cfg), y, WINDOW_OFF, relu=True))
    assert not bad, bad
    assert set(LARGE_PIXEL_TILINGS) <= ran and {'conv_wino_sk', 'conv_wino_vs'} <= ran


# the tilings the planners name only above about 2.4 M pixels (no point of OFFBENCH reaches them): test_every_compiled_tiling runs them
LARGE_PIXEL_TILINGS = ['conv_dma<1,16,2,4,4>', 'conv_dma<1,32,2,1,4>', 'conv_dma<1,32,2,2,4>', 'conv_dma<9,16,2,2,4>',
                       'conv_dma<9,16,2,3,4>', 'conv_dma<9,16,2,4,4>']
