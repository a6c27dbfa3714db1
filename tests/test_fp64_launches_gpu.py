"""GPU tier: every GEMM-type launch of the four benchmarked steps (inference and training of SqueezeDet at bs=20 and SqueezeDet+ at
bs=16, 384x1248, shipped tuning table) held to fp32 accuracy against a float64 reference, element by element.  (The harness takes any
batch and input size: tests/test_fp64_offbench_gpu.py runs it away from the benchmark; and any class count, anchor seed and ground-truth
form: tests/test_fp64_widths_gpu.py runs it over ConvDet's width classes and the head paths.)

Each case is one distinct (arch, batch, kernel, shape tag) entry of ``plan.inference_launch_plan`` / ``plan.training_launch_plan``
(``CASES``; tests/test_fp64_coverage.py keeps the list equal to the plans).  The cases run inside the real step: the model is built
with the benchmark's synthetic weights, images and targets (fixed seeds), and every ``ops`` entry point it calls is wrapped.  The
wrapper copies the launch's operands, runs the kernel, reads the (kernel, tag) its KernelTimer bracket recorded and compares every
output with tests/fp64_ref.py evaluated on those same operands -- so each launch is checked on its own inputs, at the plan's batch and
shape, on the kernel the plan names.  Weight gradients are checked after the slab reduction the step ships (``wgrad_reduce_batched``).
Dropout runs at p = 0 here: the planned epilogue kernels launch with an all-keep mask.  tests/test_fp64_dropout_gpu.py runs the harness
with a live rate (``_run_step(dropout_prob=...)``, ``check_from='dropout'``): a launch with ``drop`` is then held to its reference times
the step's mask, read through the stand-alone kernel before the launch.

Two bars per output (fp64_ref.bars):
* L: |got - ref64| <= 2^-18 * M for every element (exact where M = 0): no dropped, duplicated or misplaced term anywhere;
* P: per 64-channel block rms(err) <= k * max(rms(err32), 2^-24 rms(ref64)), per tensor max|err| <= 2k * max(max|err32|, ...), with
  err32 the plain fp32 chain's error: k = 2 for the direct-GEMM families, 4 for the Winograd ones (bridges included).
  The direct kernels (conv_igemm, conv_dma, conv_ws, fire_expand) keep ONE accumulator per output over chunk x tap x 4-channel step: their
  plain chain is restated that way (fp64_ref._conv_chain), as the weight gradients' is.  A library matmul per tap, summed afterwards,
  is 2-5x more accurate than that on a 3x3 layer, and picks other algorithms for a few pixels (3x3 grids, batch 1).
  Weight and bias gradients sum 37k-599k pixels: there the plain chain is restated as the kernels' own algorithm
  (fp64_ref.wgrad_split_k: the kernel's pixel blocks, its S slabs accumulated in order, the shipped
  slab reduction) -- a whole-axis fp32 GEMM is 2-20x less accurate than the kernels and could not tell a 3-product bf16 split from
  fp32.  k stays 2 for the direct weight gradients; the Winograd ones keep their family's 4 (the restatement is of the summation
  structure, in the direct form: it does not restate the transforms).  The Winograd weight gradient
  mixes every offset of its 4x4 input tile with its 2x2 output tile, so its bar L uses that form's magnitude
  (fp64_ref.wgrad_wino_magnitude); the per-tap ratio is logged beside it.
``maxpool_fwd`` does no arithmetic: bit-exact against the max of its own input.
The loss launches (``loss_fwd`` / ``loss_bwd``: the mean forms that bench.py's step differentiates) are held to fp64_ref.loss: losses
[4, B], mean4 and dpred at bars L (M: the chain's running error bound) and P (k = 2; dpred in class-logit / conf / delta blocks), nobj
exact, and at most 4 anchors of a launch on a branch where float64 and float32 disagree (either branch's reference is accepted there).

The head axis (``num_classes``, ``anchors_seed``, ``sparse_gt`` of ``_run_step`` / ``_run_both`` / ``_step_results``; the defaults give the
benchmark's 3 classes, KITTI's nine anchors and a dense gt, with the keys, plans and rows of before).  ConvDet's width
anchors_per_grid * (num_classes + 5) decides its launches; the entry points that only other widths and heads reach are wrapped too:
* ``loss_*_many`` (17 .. 256 classes) and ``loss_sparse_*`` (``cfg.sparse_gt``): the same checks against the same reference, a sparse gt
  through ``ops.sparse_gt_to_dense``;
* a padded ConvDet (a width that is no multiple of 4 runs zero-padded to a multiple of 64): its forward and data gradient are held to
  the MODULE's parameters, zero-extended here -- not to the stand-in's tensors, so a stand-in that did not follow the parameters fails;
  ``convdet_pack`` is bit-equal to the first N channels of the scratch, which is exactly 0.0 past them; ``convdet_unpack`` bit-equal to
  dpred and exactly 0.0 past N; ``wgrad_reduce_rows`` (its weight gradient's own slab reduction, the slabs added in ascending order) holds
  dW / db to float64 on the true dpred[..., :N], restated at the launch's own S in the blocking of the kernel that wrote the slabs.
``check_from='convdet'`` passes the backbone's launches through unchecked (the launches are still asserted equal to the plan): for
points whose backbone rows another sweep already checks, which tests/test_fp64_coverage.py asserts on the host.
``check_from='dropout'`` does the same but also checks the last Fire's two expand launches, which carry the dropout; with a live rate
ConvDet's data gradient gets a second, end-to-end reference (``_Harness._dgrad_end_to_end``).
"""
import re

import pytest
import torch

import fp64_ref as R
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import synthetic

pytestmark = pytest.mark.gpu

INPUT = (384, 1248)
STEPS = (('squeezedet', 20), ('squeezedetplus', 16))

CASES = [
    ('squeezedet', 20, 'stem_pool_sq<3>', 'stem+pool+squeeze 384x1248 S16'),
    ('squeezedet', 20, 'fire_bridge', 'fire C16 E64+64 -> S16 96x312'),
    ('squeezedet', 20, 'fire_pool_bridge', 'fire C16 E64+64 -> pool -> S32 96x312'),
    ('squeezedet', 20, 'conv_ws<4,8>', '1tap C32 N128 48x156'),
    ('squeezedet', 20, 'conv_wino_us<2,8>', '9tap C32 N128 48x156'),
    ('squeezedet', 20, 'conv_ws<2,8>', '1tap C256 N32 48x156'),
    ('squeezedet', 20, 'maxpool_fwd', 'pool C256 48x156'),
    ('squeezedet', 20, 'conv_dma<1,32,1,3,4>', '1tap C256 N48 24x78'),
    ('squeezedet', 20, 'conv_ws<4,8>', '1tap C48 N192 24x78'),
    ('squeezedet', 20, 'conv_wino<2,4>', '9tap C48 N192 24x78'),
    ('squeezedet', 20, 'conv_dma<1,32,1,3,4>', '1tap C384 N48 24x78'),
    ('squeezedet', 20, 'conv_dma<1,32,1,2,4>', '1tap C384 N64 24x78'),
    ('squeezedet', 20, 'conv_ws<4,8>', '1tap C64 N256 24x78'),
    ('squeezedet', 20, 'conv_wino_us<2,4>', '9tap C64 N256 24x78'),
    ('squeezedet', 20, 'conv_dma<1,32,1,2,4>', '1tap C512 N64 24x78'),
    ('squeezedet', 20, 'conv_ws<2,8>', '1tap C512 N96 24x78'),
    ('squeezedet', 20, 'conv_ws<6,8>', '1tap C96 N384 24x78'),
    ('squeezedet', 20, 'conv_wino<2,4>', '9tap C96 N384 24x78'),
    ('squeezedet', 20, 'conv_dma<1,32,1,6,4>', '1tap C768 N96 24x78'),
    ('squeezedet', 20, 'conv_wino_vs', '9tap C768 N72 24x78'),
    ('squeezedet', 20, 'stem_pool_sq_train<3>', 'stem+pool+squeeze 384x1248 S16'),
    ('squeezedet', 20, 'fire_bridge_save', 'fire C16 E64+64 -> S16 96x312'),
    ('squeezedet', 20, 'fire_pool_bridge_save', 'fire C16 E64+64 -> pool -> S32 96x312'),
    ('squeezedet', 20, 'conv_wino_sk', '9tap C96 N384 24x78'),
    ('squeezedet', 20, 'conv_wgrad_wino', 'wgrad 9tap C768 N72 24x78'),
    ('squeezedet', 20, 'conv_wino_sk', '9tap C72 N768 24x78'),
    ('squeezedet', 20, 'conv_dma<1,64,1,3,4>', '1tap C384 N96 24x78'),
    ('squeezedet', 20, 'conv_wino<2,4>', '9tap C384 N96 24x78'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C768 N96 24x78'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C512 N96 24x78'),
    ('squeezedet', 20, 'conv_dma<1,32,1,2,4>', '1tap C256 N64 24x78'),
    ('squeezedet', 20, 'conv_wino<2,4>', '9tap C256 N64 24x78'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C512 N64 24x78'),
    ('squeezedet', 20, 'conv_wgrad_group<1>', 'wgrad 1tap C96 N384 + C96 N384 + C64 N256 + C64 N256 24x78'),
    ('squeezedet', 20, 'conv_wgrad_wino_group', 'wgrad 9tap C96 N384 + C96 N384 + C64 N256 + C64 N256 24x78'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C384 N64 24x78'),
    ('squeezedet', 20, 'conv_dma<1,32,1,3,4>', '1tap C192 N48 24x78'),
    ('squeezedet', 20, 'conv_wino<1,4>', '9tap C192 N48 24x78'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C384 N48 24x78'),
    ('squeezedet', 20, 'conv_wgrad_group<1>', 'wgrad 1tap C48 N192 + C48 N192 24x78'),
    ('squeezedet', 20, 'conv_wgrad_wino_group', 'wgrad 9tap C48 N192 + C48 N192 24x78'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C256 N48 24x78'),
    ('squeezedet', 20, 'maxpool_bwd', 'poolbwd C256 48x156'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C32 N128 48x156'),
    ('squeezedet', 20, 'conv_wino_us<1,4>', '9tap C128 N32 48x156'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C256 N32 48x156'),
    ('squeezedet', 20, 'conv_wgrad_wino_group', 'wgrad 9tap C32 N128 + C32 N128 48x156'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C128 N32 48x156'),
    ('squeezedet', 20, 'maxpool_bwd', 'poolbwd C128 96x312'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C16 N64 96x312'),
    ('squeezedet', 20, 'conv_wino_us<1,4>', '9tap C64 N16 96x312'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C128 N16 96x312'),
    ('squeezedet', 20, 'conv_wgrad_wino_group', 'wgrad 9tap C16 N64 + C16 N64 96x312'),
    ('squeezedet', 20, 'squeeze_bwd', 'sqbwd C64 N16 96x312'),
    ('squeezedet', 20, 'stem_wgrad_pooled<3>', 'stem wgrad (pooled) 384x1248'),
    ('squeezedet', 20, 'wgrad_reduce_batched', '31 layers'),
    ('squeezedet', 20, 'loss_fwd', 'loss A16848'),
    ('squeezedet', 20, 'loss_bwd', 'lossbwd A16848'),
    ('squeezedetplus', 16, 'stem_pool<7>', 'stem+pool 384x1248'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C96 N96 96x312'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C96 N64 96x312'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C96 N64 96x312'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C128 N96 96x312'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C128 N192 96x312'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C192 N128 96x312'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C192 N128 96x312'),
    ('squeezedetplus', 16, 'maxpool_fwd', 'pool C256 96x312'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C256 N192 48x156'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C192 N128 48x156'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C192 N128 48x156'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C256 N288 48x156'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C288 N192 48x156'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C288 N192 48x156'),
    ('squeezedetplus', 16, 'conv_dma<1,32,1,6,4>', '1tap C384 N288 48x156'),
    ('squeezedetplus', 16, 'conv_dma<1,32,1,6,4>', '1tap C384 N384 48x156'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C384 N256 48x156'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C384 N256 48x156'),
    ('squeezedetplus', 16, 'maxpool_fwd', 'pool C512 48x156'),
    ('squeezedetplus', 16, 'conv_dma<1,64,1,3,4>', '1tap C512 N384 24x78'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C384 N256 24x78'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C384 N256 24x78'),
    ('squeezedetplus', 16, 'conv_wino_vs', '9tap C512 N72 24x78'),
    ('squeezedetplus', 16, 'conv_wino_sk', '9tap C384 N256 24x78'),
    ('squeezedetplus', 16, 'conv_wgrad_wino', 'wgrad 9tap C512 N72 24x78'),
    ('squeezedetplus', 16, 'conv_wino_sk', '9tap C72 N512 24x78'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C256 N384 24x78'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C256 N384 24x78'),
    ('squeezedetplus', 16, 'conv_wgrad<1>', 'wgrad 1tap C512 N384 24x78'),
    ('squeezedetplus', 16, 'conv_dma<1,64,1,4,4>', '1tap C384 N512 24x78'),
    ('squeezedetplus', 16, 'conv_wgrad_group<1>', 'wgrad 1tap C384 N256 + C384 N256 + C384 N256 24x78'),
    ('squeezedetplus', 16, 'conv_wgrad_wino_group', 'wgrad 9tap C384 N256 + C384 N256 + C384 N256 24x78'),
    ('squeezedetplus', 16, 'maxpool_bwd', 'poolbwd C512 48x156'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C256 N384 48x156'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C256 N384 48x156'),
    ('squeezedetplus', 16, 'conv_wgrad<1>', 'wgrad 1tap C384 N384 48x156'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C192 N288 48x156'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C192 N288 48x156'),
    ('squeezedetplus', 16, 'conv_wgrad<1>', 'wgrad 1tap C384 N288 48x156'),
    ('squeezedetplus', 16, 'conv_ws<6,8>', '1tap C288 N384 48x156'),
    ('squeezedetplus', 16, 'conv_wgrad_group<1>', 'wgrad 1tap C384 N256 + C288 N192 + C288 N192 48x156'),
    ('squeezedetplus', 16, 'conv_wgrad<1>', 'wgrad 1tap C256 N288 48x156'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C288 N256 48x156'),
    ('squeezedetplus', 16, 'conv_wgrad_wino_group', 'wgrad 9tap C384 N256 + C288 N192 + C288 N192 + C192 N128 48x156'),
    ('squeezedetplus', 16, 'squeeze_bwd', 'sqbwd C192 N128 48x156'),
    ('squeezedetplus', 16, 'conv_wino<2,8>', '9tap C128 N192 48x156'),
    ('squeezedetplus', 16, 'conv_wgrad<1>', 'wgrad 1tap C256 N192 48x156'),
    ('squeezedetplus', 16, 'conv_ws<4,8>', '1tap C192 N256 48x156'),
    ('squeezedetplus', 16, 'maxpool_bwd', 'poolbwd C256 96x312'),
    ('squeezedetplus', 16, 'squeeze_bwd', 'sqbwd C192 N128 96x312'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C128 N192 96x312'),
    ('squeezedetplus', 16, 'conv_wgrad<1>', 'wgrad 1tap C128 N192 96x312'),
    ('squeezedetplus', 16, 'squeeze_bwd', 'sqbwd C96 N64 96x312'),
    ('squeezedetplus', 16, 'conv_wino<2,4>', '9tap C64 N96 96x312'),
    ('squeezedetplus', 16, 'squeeze_bwd', 'sqbwd C128 N96 96x312'),
    ('squeezedetplus', 16, 'conv_wgrad_wino_group', 'wgrad 9tap C192 N128 + C96 N64 + C96 N64 96x312'),
    ('squeezedetplus', 16, 'squeeze_bwd', 'sqbwd C96 N96 96x312'),
    ('squeezedetplus', 16, 'stem_wgrad_pooled<7>', 'stem wgrad (pooled) 384x1248'),
    ('squeezedetplus', 16, 'wgrad_reduce_batched', '31 layers'),
    ('squeezedetplus', 16, 'loss_fwd', 'loss A16848'),
    ('squeezedetplus', 16, 'loss_bwd', 'lossbwd A16848'),
]

# the families the teeth test runs through the degraded emulations (first launch of each in the steps above)
FAMILIES = ['conv_ws', 'conv_dma', 'conv_wino', 'conv_wino_us', 'conv_wino_sk', 'conv_wino_vs', 'fire_bridge', 'fire_bridge_save',
            'fire_pool_bridge', 'fire_pool_bridge_save', 'stem_pool', 'stem_pool_sq', 'stem_pool_sq_train', 'maxpool_bwd', 'squeeze_bwd',
            'conv_wgrad', 'conv_wgrad_group', 'conv_wgrad_wino', 'conv_wgrad_wino_group', 'stem_wgrad_pooled']
# the loss families: their teeth are bf16-rounded pred / gt through the float32 oracle chain (there is no product split to emulate)
LOSS_FAMILIES = ['loss_fwd', 'loss_bwd']


def wgrad_blocking(fam, N, C, taps):
    """How the weight-gradient kernel that ran a (N, C, taps) layer cuts the pixel axis into the blocks its split-K slabs take in turn, and the
    pixels per fp32 accumulation -> (fp64_ref blocking, step).  Restated from the launchers (csrc/wgrad.hip sqd_conv_wgrad,
    sqd_conv_wgrad_group, sqd_squeeze_bwd; csrc/wino_wgrad.hip): the direct forms take runs of 16 * TH consecutive pixels, TH chosen
    from the out- / in-channel tiles (TN, TC) of the layer; the Winograd forms take 4x16-pixel groups whatever their channel tile
    (tc 1 or 2).  Step: 1 for the direct forms (their 16x16x4 matrix-core steps are not taken as one exact 4-product sum), 4 output
    tiles (16 pixels) for the Winograd form."""
    if 'wino' in fam:
        return 'tile', 16
    if fam == 'squeeze_bwd':                                    # launch_wgrad<1, TN, TC, 2, true>
        return ('px', 32), 1
    if fam == 'conv_wgrad_group':                               # launch_wgrad_group<4, tc, tc == 1 ? 4 : 2>
        tc = 8 if C >= 256 else (4 if C >= 64 else -(-C // 16))
        return ('px', 64 if tc == 1 else 32), 1
    assert fam == 'conv_wgrad', fam
    if taps == 9:                                               # launch_wgrad<9, ., ., 4>: 4x16-pixel tiles, image-major
        return 'tile', 1
    tn = 6 if 64 < N <= 96 else (4 if N >= 64 else -(-N // 16))
    tc = 8 if C >= 256 else (4 if C >= 64 else -(-C // 16))
    th = 2 if tn + tc >= 6 else (4 if tn + tc >= 3 else 8)
    return ('px', 16 * th), 1


def family(kernel):
    return re.sub(r'<.*>$', '', kernel)


def k_of(kernel):
    """Bar P's factor: 4 for the Winograd families (the F(2x2,3x3) transforms and the bridges built on them), 2 for direct GEMM."""
    f = family(kernel)
    return 4 if ('wino' in f or 'bridge' in f) else 2


class _Harness:
    """Wraps the ``ops`` entry points (and the slab reduction) for one step; collects per-(kernel, tag) output checks."""

    def __init__(self, base, arch, batch, timer, teeth_for=None, check_from=None, dropout_prob=0.0):
        self.base, self.arch, self.batch, self.timer = base, arch, batch, timer
        self.teeth_for = teeth_for     # the families whose first launch also runs the degraded emulations (None: every family)
        assert check_from in (None, 'convdet', 'dropout')
        # 'convdet': the backbone's launches run unchecked (``passes``); 'dropout': the same, but the last Fire's two expand launches
        # (which carry the dropout) are checked as well; None: every launch is checked
        self.check_from = check_from
        self.dropout_prob = float(dropout_prob)     # 0: the planned epilogues with an all-keep mask; > 0: a live mask (``_mask_of``)
        self.drop_ctx = {}             # live dropout: the last Fire's squeeze output and the whole mask, for ConvDet's data gradient
        self.rows = {}                 # (arch, batch, kernel, tag) -> [(output, bars dict)]
        self.teeth = {}                # family -> {emu: bars dict}
        self.pending = {}              # slab data_ptr -> (entry, dy, x, taps) until the slab reduction
        self.plan_map = self._plan_map()

    def _plan_map(self):
        """id(plan) -> what it was packed from (the model's plan cache, filled by the warm-up step)."""
        m = {}
        for e in self.base.plan_cache.entries():
            if e.kind in ('conv', 'wino'):
                m[id(e.plan)] = ('conv', e.mods[0], e.direction)
            elif e.kind == 'bridge':
                m[id(e.plan)] = ('bridge',) + e.mods
            elif e.kind == 'fused_expand':
                m[id(e.plan)] = ('expand',) + e.mods
        return m

    def _is_convdet(self, mod):
        """``mod`` is the model's ConvDet or the zero-padded stand-in the executors launch in its place (model._PaddedConvDet)."""
        return mod is self.base.convdet or getattr(mod, 'src', None) is self.base.convdet

    def passes(self, name, args):
        """With ``check_from='convdet'``: whether this call runs unchecked -- every launch of the backbone (the CPU tier asserts they
        are, name and tag, those of a point the off-benchmark sweep checks).  ConvDet's own launches, the pack / unpack / row-reduction
        launches and the loss launches are always checked."""
        if self.check_from is None:
            return False
        if name in ('conv', 'conv_wino'):
            _kind, mod, direction = self.plan_map[id(args[2])]
            if self.check_from == 'dropout' and direction == 'fwd' and self._last_expand(mod) is not None:
                return False
            return not self._is_convdet(mod)
        if name == 'conv_wgrad':
            return not (args[6] == 9 and args[5] == self.base.convdet.in_channels)
        return name in _BACKBONE_NAMES

    def _last_expand(self, mod):
        """0 / 1 if ``mod`` is the expand1x1 / expand3x3 of the last Fire (the two launches in front of ConvDet), else None."""
        fire = self.base.features[-1]
        return 0 if mod is fire.expand1x1 else 1 if mod is fire.expand3x3 else None

    def _mask_of(self, drop, y, y_coff, N):
        """The scaled keep mask a launch with ``drop`` applies to y[..., y_coff:y_coff + N]: this step's mask of the whole buffer, read
        through the stand-alone kernel BEFORE the launch (the step advances only behind ConvDet's forward), outside the timer.  At
        p = 0 the state must be the all-keep one, and there is no mask to apply."""
        if drop is None:
            return None
        if self.dropout_prob == 0.0:
            assert drop.keep16 == 65536 and drop.scale == 1.0
            return None
        assert drop.keep16 < 65536 and drop.p == self.dropout_prob
        from squeezedet_pytorch_amd import ops
        ops.set_timer(None)
        try:
            full = ops.dropout_mask(drop, tuple(y.shape))
        finally:
            ops.set_timer(self.timer)
        self.drop_ctx['mask'] = full
        return full[..., y_coff:y_coff + N].clone()

    @staticmethod
    def _dropped(r, mask):
        """A launch's Ref behind the fused dropout: ref64, M and the plain chain times the (non-negative) mask."""
        if mask is None:
            return r
        return R.Ref(r.ref64 * mask.double(), r.M * mask.double(), r.b32 * mask)

    def _note_last_fire(self, plan, x, x_coff, ymul):
        """Live dropout: keep what the end-to-end reference of ConvDet's data gradient needs -- the last Fire's squeeze output (the
        input of its expand launches) and, in the forms that multiply a mask tensor in, that tensor."""
        kind, mod, direction = self.plan_map[id(plan)]
        if self.dropout_prob > 0.0 and direction == 'fwd' and self._last_expand(mod) is not None:
            self.drop_ctx['sq'] = x[..., x_coff:x_coff + plan.C].clone()
            if ymul is not None:
                self.drop_ctx['mask'] = ymul.clone()

    def _dgrad_end_to_end(self, entry, plan, dpred, got, yscale, ymul):
        """Live dropout, ConvDet's data gradient: beside the per-launch check (on the launch's own operands, the dropped tensor as
        ReLU mask), the launch's output against fp64_ref.dropped_dgrad -- plain float64 gradient of the true dpred * the mask of the
        stand-alone kernel * (pre-dropout expand output > 0), the latter recomputed in float64 from the last Fire's squeeze output and
        the module's parameters.  Bar L with M / (1 - p); elements on the ReLU's edge excluded, at most 0.5 % of the tensor."""
        kind, mod, direction = self.plan_map[id(plan)]
        if self.dropout_prob == 0.0 or direction == 'fwd' or not self._is_convdet(mod):
            return
        scale = 1.0 / (1.0 - self.dropout_prob)
        assert ymul is not None or yscale == scale, 'the launch does not carry the dropout scale: its output is not the final gradient'
        cd, fire = self.base.convdet, self.base.features[-1]
        assert mod is cd, 'a padded ConvDet: dpred is not the true one here'
        sq, mask = self.drop_ctx['sq'], self.drop_ctx['mask']
        pre = R.cat([R.conv(sq, fire.expand1x1.weight.detach(), fire.expand1x1.bias.detach()),
                     R.conv(sq, fire.expand3x3.weight.detach(), fire.expand3x3.bias.detach())])
        r, exclude = R.dropped_dgrad(dpred, cd.weight.detach(), mask, pre, scale)
        b = R.bar_l_excluding(got, r, exclude)
        b.update(l_ok=b['l_ok'] and b['cap_ok'], p_ok=True, p_block=0.0, p_tensor=0.0, k=0, end_to_end=True)
        self.rows.setdefault(entry, []).append(('dA end to end', b))

    def _padded_params(self, pad):
        """The reference weights of a padded ConvDet: the module's own parameters, zero-extended here to the run width -- never the
        stand-in's tensors (a stand-in that did not follow the parameters must fail)."""
        src = pad.src
        assert src is self.base.convdet
        N, Npad = src.out_channels, pad.out_channels
        w0, b0 = src.weight.detach(), src.bias.detach()
        w = torch.zeros(Npad, *w0.shape[1:], device=w0.device, dtype=w0.dtype)
        b = torch.zeros(Npad, device=b0.device, dtype=b0.dtype)
        w[:N] = w0
        b[:N] = b0
        return w, b

    def _weights(self, plan):
        kind, mod, direction = self.plan_map[id(plan)]
        assert kind == 'conv'
        if getattr(mod, 'src', None) is not None:           # (the plan-cache entry of the stand-in, mapped back to base.convdet)
            w, b = self._padded_params(mod)
            return (R.dgrad_weight(w), None) if direction != 'fwd' else (w, b)
        w = mod.weight.detach()
        if direction != 'fwd':
            return R.dgrad_weight(w), None
        return w, mod.bias.detach()

    def _entry(self, n0):
        recs = self.timer.records[n0:]
        assert len(recs) == 1, [r[:2] for r in recs]
        return (self.arch, self.batch, recs[0][0], recs[0][1])

    def _check(self, entry, outs):
        """outs: [(name, got, ref_fn, kind)]; ref_fn(emu) -> Ref.  The first output of a family's first launch also goes through
        both degraded emulations (teeth)."""
        k = k_of(entry[2])
        rows = self.rows.setdefault(entry, [])
        fam = family(entry[2])
        for j, (name, got, ref_fn, kind) in enumerate(outs):
            r = ref_fn(None)
            rows.append((name, R.bars(got, r, kind, k)))
            if j == 0 and fam not in self.teeth and self._wants_teeth(fam):
                self.teeth[fam] = {emu: R.bars(ref_fn(emu).b32, r, kind, k) for emu in ('bf16', 'split3')}
            del r

    def _wants_teeth(self, fam):
        return self.teeth_for is None or fam in self.teeth_for

    def _wgrad_pending(self, entry, slab, dy, x, taps):
        """A weight-gradient launch wrote its slabs: keep its operands; the check runs after the reduction (``reduce``)."""
        self.pending[slab.data_ptr()] = (entry, dy.clone(), x.clone(), taps)

    # ---- wrapped entry points ----
    def conv(self, orig, x, x_coff, plan, y, y_coff, relu=False, accumulate=False, xmask=None, xmask_coff=0, ymask=None, ymask_coff=0,
             ymul=None, ymul_coff=0, drop=None):
        dm = self._mask_of(drop, y, y_coff, plan.N)
        self._note_last_fire(plan, x, x_coff, ymul)
        w, b = self._weights(plan)
        xw = x[..., x_coff:x_coff + plan.C]
        if xmask is not None:
            xw = xw * (xmask[..., xmask_coff:xmask_coff + plan.C] > 0)
        xw = xw.clone()
        prev = y[..., y_coff:y_coff + plan.N].clone() if accumulate else None
        ym = None if ymask is None else ymask[..., ymask_coff:ymask_coff + plan.N].clone()
        yl = None if ymul is None else ymul[..., ymul_coff:ymul_coff + plan.N].clone()
        n0 = len(self.timer.records)
        out = orig(x, x_coff, plan, y, y_coff, relu=relu, accumulate=accumulate, xmask=xmask, xmask_coff=xmask_coff, ymask=ymask,
                   ymask_coff=ymask_coff, ymul=ymul, ymul_coff=ymul_coff, drop=drop)
        got = y[..., y_coff:y_coff + plan.N]
        kc = plan.kc                                      # b32 restates the direct kernels' single accumulator (fp64_ref._conv_chain)
        entry = self._entry(n0)
        self._check(entry, [('y', got, lambda e: self._dropped(R.epilogue(R.conv(xw, w, b, emu=e, chain_kc=kc), prev, yl, 1.0, ym, relu), dm), 'act')])
        self._dgrad_end_to_end(entry, plan, xw, got, 1.0, yl)
        return out

    def conv_wino(self, orig, x, x_coff, plan, y, y_coff, relu=False, accumulate=False, ymask=None, ymul=None, yscale=1.0, drop=None,
                  drop_advance=None):
        dm = self._mask_of(drop, y, y_coff, plan.N)
        self._note_last_fire(plan, x, x_coff, ymul)
        w, b = self._weights(plan)
        xw = x[..., x_coff:x_coff + plan.C].clone()
        prev = y[..., y_coff:y_coff + plan.N].clone() if accumulate else None
        ym = None if ymask is None else ymask[..., y_coff:y_coff + plan.N].clone()
        yl = None if ymul is None else ymul[..., y_coff:y_coff + plan.N].clone()
        n0 = len(self.timer.records)
        out = orig(x, x_coff, plan, y, y_coff, relu=relu, accumulate=accumulate, ymask=ymask, ymul=ymul, yscale=yscale, drop=drop,
                   drop_advance=drop_advance)
        got = y[..., y_coff:y_coff + plan.N]
        entry = self._entry(n0)
        self._check(entry, [('y', got, lambda e: self._dropped(R.epilogue(R.conv(xw, w, b, emu=e), prev, yl, yscale, ym, relu), dm), 'act')])
        self._dgrad_end_to_end(entry, plan, xw, got, yscale, yl)
        return out

    def fire_expand(self, orig, x, x_coff, fplan, y, y_coff):
        kind, e1, e3 = self.plan_map[id(fplan)]
        assert kind == 'expand'
        ws = tuple(t.detach() for t in (e1.weight, e1.bias, e3.weight, e3.bias))
        xw = x[..., x_coff:x_coff + fplan.C].clone()
        n0 = len(self.timer.records)
        out = orig(x, x_coff, fplan, y, y_coff)
        self._check(self._entry(n0), [('y', y[..., y_coff:y_coff + 2 * fplan.E], lambda e: R.fire_expand(xw, *ws, emu=e, chain_kc=fplan.plan.kc), 'act')])
        return out

    def _bridge_weights(self, plan):
        kind, e1, e3, sq = self.plan_map[id(plan)]
        assert kind == 'bridge'
        return tuple(t.detach() for t in (e1.weight, e1.bias, e3.weight, e3.bias, sq.weight, sq.bias))

    def fire_bridge(self, orig, x, x_coff, plan, y, y_coff, save=None, save_coff1=0, save_coff3=None):
        ws = self._bridge_weights(plan)
        N1, N3 = ws[0].shape[0], ws[2].shape[0]
        xw = x[..., x_coff:x_coff + plan.C].clone()
        n0 = len(self.timer.records)
        out = orig(x, x_coff, plan, y, y_coff, save=save, save_coff1=save_coff1, save_coff3=save_coff3)
        outs = [('y', y[..., y_coff:y_coff + plan.Nsq], lambda e: R.fire_bridge(xw, *ws, emu=e)[0], 'act')]
        if save is not None:
            c3 = save_coff1 + N1 if save_coff3 is None else save_coff3
            got = torch.cat([save[..., save_coff1:save_coff1 + N1], save[..., c3:c3 + N3]], -1)
            outs.append(('save', got, lambda e: R.fire_bridge(xw, *ws, emu=e)[1], 'act'))
        self._check(self._entry(n0), outs)
        return out

    def fire_pool_bridge(self, orig, x, x_coff, plan, y, y_coff, nseg=4, save=None, codes=None, save_coff1=0, save_coff3=None):
        ws = self._bridge_weights(plan)
        N1, N3 = ws[0].shape[0], ws[2].shape[0]
        xw = x[..., x_coff:x_coff + plan.C].clone()
        n0 = len(self.timer.records)
        out = orig(x, x_coff, plan, y, y_coff, nseg=nseg, save=save, codes=codes, save_coff1=save_coff1, save_coff3=save_coff3)
        outs = [('y', y[..., y_coff:y_coff + plan.Nsq], lambda e: R.fire_pool_bridge(xw, *ws, emu=e)[0], 'act')]
        if save is not None:
            c3 = save_coff1 + N1 if save_coff3 is None else save_coff3
            got = torch.cat([save[..., save_coff1:save_coff1 + N1], save[..., c3:c3 + N3]], -1)
            outs.append(('pooled', got, lambda e: R.fire_pool_bridge(xw, *ws, emu=e)[1], 'act'))
        self._check(self._entry(n0), outs)
        return out

    def stem_pool(self, orig, image, weight, bias, argmax=None):
        n0 = len(self.timer.records)
        out = orig(image, weight, bias, argmax=argmax)
        img, w, b = image.detach(), weight.detach(), bias.detach()
        self._check(self._entry(n0), [('pooled', out, lambda e: R.stem_pool(img, w, b, emu=e), 'act')])
        return out

    def stem_pool_squeeze(self, orig, image, weight, bias, sq_weight, sq_bias, argmax=None):
        n0 = len(self.timer.records)
        res = orig(image, weight, bias, sq_weight, sq_bias, argmax=argmax)
        img, w, b, ws, bs = (t.detach() for t in (image, weight, bias, sq_weight, sq_bias))
        y = res[0] if argmax is not None else res
        outs = [('y', y, lambda e: R.stem_pool_squeeze(img, w, b, ws, bs, emu=e)[0], 'act')]
        if argmax is not None:
            outs.append(('pooled', res[1], lambda e: R.stem_pool_squeeze(img, w, b, ws, bs, emu=e)[1], 'act'))
        self._check(self._entry(n0), outs)
        return res

    def maxpool(self, orig, x, out=None, argmax=None, relu_codes=False):
        n0 = len(self.timer.records)
        y = orig(x, out=out, argmax=argmax, relu_codes=relu_codes)
        entry = self._entry(n0)
        exact = torch.equal(y, R.maxpool_exact(x))
        self.rows.setdefault(entry, []).append(('y', dict(exact=exact, l_ok=exact, p_ok=exact, l_ratio=0.0 if exact else float('inf'),
                                                          p_block=0.0, p_tensor=0.0, k=0)))
        return y

    def maxpool_bwd(self, orig, dy, argmax, in_hw, out=None, relu_src=None):
        assert relu_src is None
        d, am = dy.clone(), argmax.clone()
        n0 = len(self.timer.records)
        dx = orig(dy, argmax, in_hw, out=out, relu_src=relu_src)
        self._check(self._entry(n0), [('dx', dx, lambda e: R.maxpool_bwd(d, am, in_hw, emu=e), 'act')])
        return dx

    def conv_wgrad(self, orig, dy, dy_coff, N, x, x_coff, C, taps, slab=None, wino=None):
        assert slab is not None
        n0 = len(self.timer.records)
        res = orig(dy, dy_coff, N, x, x_coff, C, taps, slab=slab, wino=wino)
        self._wgrad_pending(self._entry(n0), slab, dy[..., dy_coff:dy_coff + N], x[..., x_coff:x_coff + C], taps)
        return res

    def _group(self, orig, taps, items, *args):
        n0 = len(self.timer.records)
        res = orig(items, *args)
        entry = self._entry(n0)
        for dy, dy_coff, N, x, x_coff, C, slab in items:
            self._wgrad_pending(entry, slab, dy[..., dy_coff:dy_coff + N], x[..., x_coff:x_coff + C], taps)
        return res

    def conv_wgrad_group(self, orig, items, S):
        return self._group(orig, 1, items, S)

    def conv_wgrad_wino_group(self, orig, items, S, tc):
        return self._group(orig, 9, items, S, tc)

    def squeeze_bwd(self, orig, dy, x, weight, slab, dx, relu_mask, dy_coff=0, N=None):
        Nn = dy.shape[3] - dy_coff if N is None else int(N)
        dyw, xc = dy[..., dy_coff:dy_coff + Nn].clone(), x.clone()
        w = R.dgrad_weight(weight.detach())
        n0 = len(self.timer.records)
        res = orig(dy, x, weight, slab, dx, relu_mask, dy_coff=dy_coff, N=N)
        entry = self._entry(n0)
        self._check(entry, [('dx', dx, lambda e: R.epilogue(R.conv(dyw, w, emu=e), ymask=xc if relu_mask else None), 'act')])
        self._wgrad_pending(entry, slab, dyw, xc, 1)
        return res

    @staticmethod
    def _exact(ok):
        return dict(exact=ok, l_ok=ok, p_ok=ok, l_ratio=0.0 if ok else float('inf'), p_block=0.0, p_tensor=0.0, k=0)

    def convdet_pack(self, orig, y_pad, N, out=None):
        """No arithmetic: the packed pred is bit-equal to the first N channels of the padded scratch, and the scratch is exactly 0.0
        past them (a zero weight row with a zero bias is exact in every kernel form)."""
        src = y_pad.clone()
        n0 = len(self.timer.records)
        res = orig(y_pad, N, out=out)
        entry = self._entry(n0)
        same = tuple(res.shape) == tuple(src.shape[:3]) + (N,) and res.is_contiguous() and bool(torch.equal(res, src[..., :N]))
        zero = bool((src[..., N:] == 0).all()) and not bool(torch.signbit(src[..., N:]).any())
        self.rows.setdefault(entry, []).extend([('pred', self._exact(same)), ('scratch past N', self._exact(zero))])
        return res

    def convdet_unpack(self, orig, dy, Npad):
        src = dy.clone()
        N = dy.shape[3]
        n0 = len(self.timer.records)
        res = orig(dy, Npad)
        entry = self._entry(n0)
        same = tuple(res.shape) == tuple(src.shape[:3]) + (Npad,) and bool(torch.equal(res[..., :N], src))
        zero = bool((res[..., N:] == 0).all()) and not bool(torch.signbit(res[..., N:]).any())
        self.rows.setdefault(entry, []).extend([('dpred', self._exact(same)), ('past N', self._exact(zero))])
        return res

    def wgrad_reduce_rows(self, orig, slab, S, N, Npad, C, taps, dw, db, scale=1.0):
        """The padded ConvDet's own slab reduction: dw / db (the parameter-shaped views) against float64 on the TRUE dpred[..., :N],
        b32 = the split-K restatement at the launch's own S, in the blocking of the kernel that wrote the slabs, the slabs added in
        ascending order (csrc/convdet_pad.hip)."""
        assert scale == 1.0
        src, dy, x, taps_ = self.pending.pop(slab.data_ptr())
        assert taps_ == taps and dy.shape[3] == Npad and x.shape[3] == C and tuple(dw.shape) == (N, C, 3 if taps == 9 else 1, 3 if taps == 9 else 1)
        n0 = len(self.timer.records)
        res = orig(slab, S, N, Npad, C, taps, dw, db, scale=scale)
        entry = self._entry(n0)
        checks = self._wgrad_checks(src, dy[..., :N].contiguous(), x, taps, S, N, C, Npad, dw, db, 'ascending')
        for e in (src, entry):
            self.rows.setdefault(e, []).extend(checks)
        return res

    def _wgrad_checks(self, src, dy, x, taps, S, N, C, Nrun, gw, gb, order):
        """[(name, bars)] of one layer's reduced (dW, db) against float64 on (dy, x); ``Nrun``: the width the launch ran at (its tiles)."""
        fam = family(src[2])
        blocking, step = wgrad_blocking(fam, Nrun, C, taps)
        kk = k_of(src[2])
        dW, db = R.wgrad(dy, x, taps)
        w32, b32 = R.wgrad_split_k(dy, x, taps, S, blocking, step, order=order)
        dW, db = R.Ref(dW.ref64, dW.M, w32), R.Ref(db.ref64, db.M, b32)
        if 'wino' in fam:
            # bar L on the Winograd form's own magnitude (R.wgrad_wino_magnitude); the per-tap ratio is logged next to it
            tap = R.bars(gw, dW, 'wgrad', kk)['l_ratio']
            dW = R.Ref(dW.ref64, R.wgrad_wino_magnitude(dy, x), dW.b32)
            bw = R.bars(gw, dW, 'wgrad', kk)
            bw['l_ratio_tap'] = tap
        else:
            bw = R.bars(gw, dW, 'wgrad', kk)
        if fam not in self.teeth and self._wants_teeth(fam):
            self.teeth[fam] = {emu: R.bars(R.wgrad_split_k(dy, x, taps, S, blocking, step, emu, order=order)[0], dW, 'wgrad', kk)
                               for emu in ('bf16', 'split3')}
        return [(f'dW C{C} N{N} S{S}', bw), (f'db N{N} S{S}', R.bars(gb, db, 'vec', kk))]

    def stem_wgrad_pooled(self, orig, dpool, pooled, argmax, image, N, ksize, out=None):
        d, am, img = dpool.clone(), argmax.clone(), image.clone()
        n0 = len(self.timer.records)
        dw, db = orig(dpool, pooled, argmax, image, N, ksize, out=out)
        self._check(self._entry(n0), [('dW', dw, lambda e: R.stem_wgrad_pooled(d, am, img, N, ksize, emu=e)[0], 'wgrad'),
                                      ('db', db, lambda e: R.stem_wgrad_pooled(d, am, img, N, ksize, emu=e)[1], 'vec')])
        return dw, db

    # ---- the loss launches: every output against fp64_ref.loss on the launch's own operands (bar P at k = 2) ----
    def _loss_rows(self, entry, outs):
        rows = self.rows.setdefault(entry, [])
        for name, got, r, kind in outs:
            rows.append((name, R.bars_nan(got.cpu(), r, kind, 2)))

    @staticmethod
    def _dense_gt(gt, A, C):
        """The launch's ground truth as the dense [B, A, C+9] tensor the reference reads (a sparse one: ``ops.sparse_gt_to_dense``)."""
        from squeezedet_pytorch_amd import ops
        if isinstance(gt, ops.SparseGT):
            return ops.sparse_gt_to_dense(ops.SparseGT(*(t.detach().clone() for t in gt)), A, C)
        return gt.detach().clone()

    def _loss_fwd(self, orig, pred, gt, anchors, input_size, num_classes, weights, mean, teeth='loss_fwd'):
        p, a = pred.detach().clone(), anchors.detach().clone()
        g = self._dense_gt(gt, p.shape[1], num_classes)
        n0 = len(self.timer.records)
        res = orig(pred, gt, anchors, input_size, num_classes, weights)
        entry = self._entry(n0)
        ref = R.loss(p, g, a, input_size, num_classes, weights)
        nobj_exact = bool(torch.equal(res[1].cpu().double(), ref['nobj']))
        outs = [('losses', res[0], ref['losses'], 'vec')] + ([('mean4', res[2], ref['mean4'], 'vec')] if mean else [])
        self._loss_rows(entry, outs)
        self.rows[entry].append(('nobj', dict(exact=nobj_exact, l_ok=nobj_exact, p_ok=nobj_exact, l_ratio=0.0, p_block=0.0,
                                               p_tensor=0.0, k=0)))
        if teeth not in self.teeth and self._wants_teeth(teeth):
            l16 = R.loss_bf16(p, g, a, input_size, num_classes, weights)[0]
            self.teeth[teeth] = {'bf16': R.bars(l16, ref['losses'], 'vec', 2)}
        return res

    def loss_fwd(self, orig, pred, gt, anchors, input_size, num_classes, weights):
        return self._loss_fwd(orig, pred, gt, anchors, input_size, num_classes, weights, False)

    def loss_mean_fwd(self, orig, pred, gt, anchors, input_size, num_classes, weights):
        return self._loss_fwd(orig, pred, gt, anchors, input_size, num_classes, weights, True)

    def _loss_bwd(self, orig, args, input_size, num_classes, weights, gmean=None, coef=None, teeth='loss_bwd'):
        p, a = args[0].detach().clone(), args[2].detach().clone()
        g = self._dense_gt(args[1], p.shape[1], num_classes)
        n0 = len(self.timer.records)
        dpred = orig(*args, input_size, num_classes, weights)
        entry = self._entry(n0)
        ref = R.loss(p, g, a, input_size, num_classes, weights, gmean=gmean, coef=coef)
        name = 'dmean' if gmean is not None else 'dcoef'
        got = dpred.cpu()
        self._loss_rows(entry, [('dpred', got, R.pick(got, ref[name], ref[name + '_alt'], ref['flips']), 'dpred')])
        flips = int(ref['flips'].sum())
        print(f'{entry[2]} {entry[3]}: {flips} anchors where float64 and float32 take different branches')
        self.rows[entry].append(('flips', dict(exact=flips <= 4, l_ok=flips <= 4, p_ok=True, l_ratio=0.0, p_block=0.0, p_tensor=0.0,
                                                k=0, flips=flips)))
        if teeth not in self.teeth and self._wants_teeth(teeth):
            d16 = R.loss_bf16(p, g, a, input_size, num_classes, weights, gmean=gmean, coef=coef)[1 if gmean is not None else 2]
            self.teeth[teeth] = {'bf16': R.bars(d16, ref[name], 'dpred', 2)}
        return dpred

    def loss_mean_bwd(self, orig, pred, gt, anchors, nobj, gmean, input_size, num_classes, weights):
        return self._loss_bwd(orig, (pred, gt, anchors, nobj, gmean), input_size, num_classes, weights, gmean=float(gmean.reshape(-1)[0]))

    def loss_bwd(self, orig, pred, gt, anchors, nobj, coef, input_size, num_classes, weights):
        return self._loss_bwd(orig, (pred, gt, anchors, nobj, coef), input_size, num_classes, weights, coef=coef.detach().cpu())

    # the many-class (17 .. 256 classes: ``ops.loss_fns``) and the sparse-ground-truth launches: the same checks on the same reference
    # (a sparse gt through ``ops.sparse_gt_to_dense``); their teeth are kept under their own names
    def loss_fwd_many(self, orig, pred, gt, anchors, input_size, num_classes, weights):
        return self._loss_fwd(orig, pred, gt, anchors, input_size, num_classes, weights, False, 'loss_fwd_many')

    def loss_mean_fwd_many(self, orig, pred, gt, anchors, input_size, num_classes, weights):
        return self._loss_fwd(orig, pred, gt, anchors, input_size, num_classes, weights, True, 'loss_fwd_many')

    def loss_mean_bwd_many(self, orig, pred, gt, anchors, nobj, gmean, input_size, num_classes, weights):
        return self._loss_bwd(orig, (pred, gt, anchors, nobj, gmean), input_size, num_classes, weights, gmean=float(gmean.reshape(-1)[0]),
                              teeth='loss_bwd_many')

    def loss_bwd_many(self, orig, pred, gt, anchors, nobj, coef, input_size, num_classes, weights):
        return self._loss_bwd(orig, (pred, gt, anchors, nobj, coef), input_size, num_classes, weights, coef=coef.detach().cpu(),
                              teeth='loss_bwd_many')

    def loss_sparse_fwd(self, orig, pred, sgt, anchors, input_size, num_classes, weights):
        return self._loss_fwd(orig, pred, sgt, anchors, input_size, num_classes, weights, False, 'loss_sparse_fwd')

    def loss_sparse_mean_fwd(self, orig, pred, sgt, anchors, input_size, num_classes, weights):
        return self._loss_fwd(orig, pred, sgt, anchors, input_size, num_classes, weights, True, 'loss_sparse_fwd')

    def loss_sparse_mean_bwd(self, orig, pred, sgt, anchors, nobj, gmean, input_size, num_classes, weights):
        return self._loss_bwd(orig, (pred, sgt, anchors, nobj, gmean), input_size, num_classes, weights, gmean=float(gmean.reshape(-1)[0]),
                              teeth='loss_sparse_bwd')

    def loss_sparse_bwd(self, orig, pred, sgt, anchors, nobj, coef, input_size, num_classes, weights):
        return self._loss_bwd(orig, (pred, sgt, anchors, nobj, coef), input_size, num_classes, weights, coef=coef.detach().cpu(),
                              teeth='loss_sparse_bwd')

    def reduce(self, orig, wb, grad_flat, row_lo=0, row_hi=None, scale=1.0):
        """After the slab reduction: every layer's (dW, db) against float64, b32 = the split-K restatement with the layer's own S."""
        assert scale == 1.0
        n0 = len(self.timer.records)
        res = orig(wb, grad_flat, row_lo, row_hi, scale)
        entry = self._entry(n0)
        rows = wb.table.cpu().tolist()
        row_hi = wb.nrows if row_hi is None else row_hi
        base_ptr = wb.workspace.data_ptr()
        for slab_off, dw_off, db_off, S, _stride, N, C, taps, _blk in rows[row_lo:row_hi]:
            k = 3 if taps == 9 else 1
            if self.check_from is not None and base_ptr + 4 * slab_off not in self.pending:
                continue                                     # (a backbone layer, passed through unchecked)
            src, dy, x, taps_ = self.pending.pop(base_ptr + 4 * slab_off)
            assert taps_ == taps and tuple(dy.shape[3:]) == (N,) and x.shape[3] == C
            gw = grad_flat[dw_off:dw_off + N * C * taps].view(N, C, k, k)
            gb = grad_flat[db_off:db_off + N]
            checks = self._wgrad_checks(src, dy, x, taps, S, N, C, N, gw, gb, 'batched')
            for e in (src, entry):
                self.rows.setdefault(e, []).extend(checks)
            del dy, x
        return res


_NAMES = ('conv', 'conv_wino', 'fire_expand', 'fire_bridge', 'fire_pool_bridge', 'stem_pool', 'stem_pool_squeeze', 'maxpool', 'maxpool_bwd',
          'conv_wgrad', 'conv_wgrad_group', 'conv_wgrad_wino_group', 'squeeze_bwd', 'stem_wgrad_pooled',
          'loss_fwd', 'loss_mean_fwd', 'loss_bwd', 'loss_mean_bwd',
          'convdet_pack', 'convdet_unpack', 'wgrad_reduce_rows', 'loss_fwd_many', 'loss_mean_fwd_many', 'loss_bwd_many', 'loss_mean_bwd_many',
          'loss_sparse_fwd', 'loss_sparse_mean_fwd', 'loss_sparse_bwd', 'loss_sparse_mean_bwd')
# what ``check_from='convdet'`` passes through unchecked whatever its operands (``_Harness.passes``): the backbone alone calls these
_BACKBONE_NAMES = ('fire_expand', 'fire_bridge', 'fire_pool_bridge', 'stem_pool', 'stem_pool_squeeze', 'maxpool', 'maxpool_bwd',
                   'conv_wgrad_group', 'conv_wgrad_wino_group', 'squeeze_bwd', 'stem_wgrad_pooled')


def anchors_seed(k):
    """An anchor seed of k shapes: the first k rows of the KITTI nine; past nine, the nine again times 2, 3, ... (distinct shapes)."""
    import numpy as np
    from squeezedet_pytorch_amd.boxes import KITTI_ANCHORS_SEED
    base = np.asarray(KITTI_ANCHORS_SEED)
    return np.concatenate([base * (1 + j) for j in range(-(-k // len(base)))])[:k]


def _head_kwargs(num_classes, seed, sparse_gt):
    """The keyword arguments of the class / anchor / gt axis for ``make_cfg``, ``make_state_dict``, ``make_gt`` and the planners: all
    empty at the defaults (3 classes, the KITTI nine, dense gt), so that a default point calls everything exactly as before."""
    import numpy as np
    cfg_kw, sd_kw, gt_kw, plan_kw = {}, {}, {}, {}
    if num_classes != 3:
        cfg_kw['num_classes'] = sd_kw['num_classes'] = gt_kw['num_classes'] = plan_kw['num_classes'] = int(num_classes)
    if seed is not None:
        cfg_kw['anchors_seed'] = np.asarray(seed)
        sd_kw['anchors_per_grid'] = plan_kw['anchors_per_grid'] = int(np.asarray(seed).shape[0])
    if sparse_gt:
        cfg_kw['sparse_gt'] = True
    return cfg_kw, sd_kw, gt_kw, plan_kw


DROP_FORMS = ('fused', 'standalone', 'injected')


def _run_step(arch, batch, mode, size=INPUT, gt_seed=1, teeth_for=None, num_classes=3, anchors_seed=None, sparse_gt=False, check_from=None,
              dropout_prob=0.0, drop_form='fused'):
    """One step at ``size`` (the benchmarked one by default; the same seeds as bench.py) with every GEMM-type launch checked.
    ``num_classes`` / ``anchors_seed`` (None: the KITTI nine) / ``sparse_gt``: the head axis, which decides ConvDet's width
    anchors_per_grid * (num_classes + 5) and the loss launches; ``check_from``: ``_Harness.passes``.
    ``dropout_prob``: 0 (default) runs the planned dropout epilogues with an all-keep mask, as every sweep did; > 0 (training) builds
    the module with that rate and leaves it live, in one of ``DROP_FORMS``: the fused epilogues, ``base.fused_dropout = False`` (the
    stand-alone ``dropout_mask`` launch, a mask tensor multiplied in), or ``base._forced_drop_mask`` set to the stream's current mask.
    The harness then holds (seed, step) of the stream before and after the checked step in ``drop_rng``.
    -> (harness, [(kernel, tag)] recorded)."""
    from squeezedet_pytorch_amd import ops, plans as plans_mod
    from squeezedet_pytorch_amd.detector import Detector
    from squeezedet_pytorch_amd.model import SqueezeDet, SqueezeDetWithLoss
    torch.manual_seed(0)
    cfg_kw, sd_kw, gt_kw, _ = _head_kwargs(num_classes, anchors_seed, sparse_gt)
    assert drop_form in DROP_FORMS and (dropout_prob == 0.0 or mode == 'train')
    if dropout_prob > 0.0:
        cfg_kw['dropout_prob'] = float(dropout_prob)
    cfg = sqd.make_cfg(arch=arch, input_size=size, device='cuda', **cfg_kw)
    sd = synthetic.make_state_dict(arch, seed=1234, **sd_kw)
    x = synthetic.make_images(batch, size, seed=0).cuda()
    if mode == 'train':
        m = SqueezeDetWithLoss(cfg)
        m.load_state_dict(sd)
        m = m.cuda().train()
        base = m.base
        if dropout_prob == 0.0:
            base.dropout_prob = 0.0      # the planned dropout epilogues with an all-keep mask
        else:
            assert base.dropout_prob == dropout_prob and base.dropout is not None
            dev = torch.device('cuda', torch.cuda.current_device())
            if drop_form == 'standalone':
                base.fused_dropout = False
            elif drop_form == 'injected':        # the mask the stream would draw now, as the NCHW tensor the tests inject
                from squeezedet_pytorch_amd import autograd, plan
                last = plan.forward_schedule(arch, batch, size, autograd._flags(base), True, 'mask')[-1]
                fh, fw = last.H, last.W
                full = ops.dropout_mask(base.drop_state(dev), (batch, fh, fw, base.convdet.in_channels))
                base._forced_drop_mask = full.permute(0, 3, 1, 2).contiguous()
        batch_d = {'image': x, 'gt': synthetic.make_gt(batch, cfg.anchors, size, seed=gt_seed, **gt_kw).cuda()}
        if sparse_gt:                    # the positives as a list: the sparse loss launches, no dense gt in the step
            batch_d = {'image': x, 'gt_sparse': ops.sparse_gt_from_dense(batch_d['gt'])}

        def step():                      # bench.py's form (trainer.make_train_step): the mean and its backward in the loss launches
            loss, _ = m.forward_mean(batch_d)
            m.zero_grad()
            loss.backward()
    else:
        m = SqueezeDet(cfg)
        m.load_state_dict(sd)
        det = Detector(m, cfg)
        base = det.model.base

        def step():
            det.detect_device(x)
    step()                                # plans are packed here, outside the checked pass
    torch.cuda.synchronize()
    timer = ops.KernelTimer()
    h = _Harness(base, arch, batch, timer, teeth_for, check_from, dropout_prob)
    rng_before = base.get_dropout_rng() if mode == 'train' else None
    saved = {n: getattr(ops, n) for n in _NAMES}
    red = plans_mod.WgradBatch.reduce
    for n in _NAMES:
        setattr(ops, n, (lambda n, meth, orig: lambda *a, **kw: orig(*a, **kw) if h.passes(n, a) else meth(orig, *a, **kw))(n, getattr(h, n), saved[n]))
    plans_mod.WgradBatch.reduce = lambda wb, *a, **kw: h.reduce(red, wb, *a, **kw)
    ops.set_timer(timer)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        ops.set_timer(None)
        for n in _NAMES:
            setattr(ops, n, saved[n])
        plans_mod.WgradBatch.reduce = red
    assert not h.pending, 'weight-gradient slabs that no reduction consumed'
    h.drop_rng = (rng_before, base.get_dropout_rng() if mode == 'train' else None)
    h.drop_ctx.clear()
    return h, [(r[0], r[1]) for r in timer.records]


_STATE = {}


def _step_results(arch, batch, size=INPUT, swap=None, gt_seed=1, teeth_for=None, num_classes=3, anchors_seed=None, sparse_gt=False,
                  check_from=None):
    """{(arch, batch, kernel, tag): rows} of the inference and the training step of ``arch`` at ``size`` (run once per process; a failure
    is kept and raised again for every case of that point instead of re-running the steps).  ``swap``: a context manager factory that
    replaces look-ups of ``ops`` for the two steps and the plans they are compared with (forced kernel forms); ``gt_seed``: the
    ground-truth seed of the training step; ``teeth_for``: the families that also run the degraded emulations (None: all);
    ``num_classes`` / ``anchors_seed`` / ``sparse_gt`` / ``check_from``: ``_run_step`` (a default point keeps its key)."""
    key = (arch, batch, tuple(size)) if swap is None else (arch, batch, tuple(size), swap.__name__)
    if (num_classes, anchors_seed is None, bool(sparse_gt), check_from) != (3, True, False, None):
        seed_key = None if anchors_seed is None else tuple(map(tuple, anchors_seed))
        key += (int(num_classes), seed_key, bool(sparse_gt), check_from)
    if key not in _STATE:
        try:
            _STATE[key] = _run_both(arch, batch, tuple(size), swap, gt_seed, teeth_for, num_classes, anchors_seed, sparse_gt, check_from)
        except Exception as exc:            # noqa: BLE001 -- re-raised below, and by every later case of this arch
            _STATE[key] = exc
    res = _STATE[key]
    if isinstance(res, Exception):
        raise res
    return res


def _run_both(arch, batch, size=INPUT, swap=None, gt_seed=1, teeth_for=None, num_classes=3, anchors_seed=None, sparse_gt=False,
              check_from=None):
    if swap is not None:
        with swap():
            return _run_both(arch, batch, size, None, gt_seed, teeth_for, num_classes, anchors_seed, sparse_gt, check_from)
    from squeezedet_pytorch_amd import plan
    rows, teeth = {}, {}
    plan_kw = _head_kwargs(num_classes, anchors_seed, sparse_gt)[3]
    for mode, planner in (('infer', plan.inference_launch_plan), ('train', plan.training_launch_plan)):
        h, got = _run_step(arch, batch, mode, size, gt_seed, teeth_for, num_classes, anchors_seed, sparse_gt, check_from)
        want = planner(arch, batch, size, **plan_kw, **({'sparse_gt': True} if (sparse_gt and mode == 'train') else {}))
        assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:4] + [len(got), len(want)]
        for e, r in h.rows.items():
            rows.setdefault(e, []).extend(r)
        for f, t in h.teeth.items():
            teeth.setdefault(f, t)
        del h
        torch.cuda.empty_cache()
    return rows, teeth


def _fmt(case, name, b):
    if 'flips' in b:
        return f'{case[0]:14s} b{case[1]:<3d} {case[2]:24s} {case[3]:56s} {name:20s} branch flips {b["flips"]} (at most 4)'
    if 'exact' in b:
        return f'{case[0]:14s} b{case[1]:<3d} {case[2]:24s} {case[3]:56s} {name:20s} bit-exact={b["exact"]}'
    tap = f'  (per-tap M: {b["l_ratio_tap"]:.2e})' if 'l_ratio_tap' in b else ''
    return (f'{case[0]:14s} b{case[1]:<3d} {case[2]:24s} {case[3]:56s} {name:20s} max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e})  '
            f'P block {b["p_block"]:5.2f} (k {b["k"]})  P tensor {b["p_tensor"]:5.2f} (2k {2 * b["k"]}){tap}')


@pytest.mark.parametrize('case', CASES, ids=[f'{a}-b{b}-{k}-{t}' for a, b, k, t in CASES])
def test_launch_against_fp64(case):
    """The planned (kernel, tag) ran in the benchmarked step, and every output it wrote holds bars L and P (or is bit-exact)."""
    rows, _ = _step_results(case[0], case[1])
    assert case in rows, f'{case} did not run in the step (fallback or plan drift)'
    bad = []
    for name, b in rows[case]:
        print(_fmt(case, name, b))
        if not (b['l_ok'] and b['p_ok']):
            bad.append((name, b))
    assert not bad, bad


@pytest.mark.parametrize('fam,emu', [(f, e) for f in FAMILIES for e in ('bf16', 'split3')] + [(f, 'bf16') for f in LOSS_FAMILIES])
def test_teeth_bar_p_rejects_degraded_emulations(fam, emu):
    """Bar P tells an fp32 kernel from reduced-precision ones: the first launch of each family, recomputed with bf16-rounded operands and
    with the 3-product bf16 split instead of the kernel (the weight gradients: inside the same split-K slab structure), fails it.  The
    loss launches: the float32 oracle chain on bf16-rounded pred and gt fails it, for the losses and for dpred."""
    found = None
    for arch, batch in STEPS:
        t = _step_results(arch, batch)[1].get(fam)
        if t is not None:
            found = t
            break
    assert found is not None, f'no launch of family {fam} in the benchmarked steps'
    b = found[emu]
    print(f'teeth {fam:24s} {emu:7s} P block {b["p_block"]:9.2f}  P tensor {b["p_tensor"]:9.2f}  (k {b["k"]})')
    assert not b['p_ok'], (fam, emu, b)
