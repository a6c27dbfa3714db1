"""CPU tier: tests/test_fp64_launches_gpu.py has one case per (arch, batch, kernel, shape tag) entry of the four benchmarked launch plans
(recomputed here on the host with the shipped tuning table), and no case that the plans no longer contain.  A new kernel, tuning row
or fusion that changes a plan fails here until it has a float64 case.  The plain references of tests/fp64_ref.py are checked against
torch's own convolution, pooling and autograd on small shapes; the loss reference against float64 autograd, its bound against the
float32 oracle chain (attainability), and each wrong branch convention against the loss edge cases (teeth); the clip + SGD reference
against torch.optim.SGD + clip_grad_norm_, and the norm bar against a norm that drops the tail or a part.
The off-benchmark sweep (tests/test_fp64_offbench_gpu.py) is held the same way: its two lists equal the planners' output at its points
(the forced-forms point recomputed under the same swap of look-ups), and every kernel name the planners produce over a grid of batches
and input sizes has a float64 case in one of the lists.
The sweep along the head axis (tests/test_fp64_widths_gpu.py: class counts, anchors per cell, sparse ground truth) likewise: ``WIDTHS``
equals the planners' ConvDet-side rows at its points, the backbone rows of those points are the ones the off-benchmark sweep checks,
every kernel name and every ConvDet signature the planners produce over 1..20 anchors x 1..256 classes x dense / sparse occurs at a
point, and a numpy restatement of ``wgrad_reduce_rows`` with a wrong row stride, a wrong bias offset or a dropped slab fails bar L.
The sweep with a live dropout (tests/test_fp64_dropout_gpu.py): its cases equal the planners' rows from the last Fire's expand launches
through ConvDet's data gradient, for the fused and the stand-alone form; ``dropout_mask`` itself is bit-exact elsewhere (``ALLOWED``)."""
import contextlib
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ref as R  # noqa: E402
import test_fp64_launches_gpu as L  # noqa: E402
import test_fp64_loss_gpu as LG  # noqa: E402
import test_fp64_offbench_gpu as OB  # noqa: E402
import test_fp64_optim_gpu as OG  # noqa: E402
import test_fp64_widths_gpu as WD  # noqa: E402
import test_fp64_dropout_gpu as DR  # noqa: E402

# launches outside the float64 sweep, each with the test that covers it
ALLOWED = {
    'detect': 'tests/test_detect_sweep_gpu.py (exact against oracle.filter_detections)',
    'dropout_mask': 'bit-exact against `ops.dropout_mask_reference`, tests/test_dropout_gpu.py',
}


def plan_entries():
    from squeezedet_pytorch_amd import plan
    out = []
    for arch, batch in L.STEPS:
        for planner in (plan.inference_launch_plan, plan.training_launch_plan):
            for kernel, tag in planner(arch, batch, L.INPUT):
                e = (arch, batch, kernel, tag)
                if e not in out:
                    out.append(e)
    return out


def test_every_plan_entry_has_a_case():
    entries = plan_entries()
    cases = set(L.CASES)
    assert len(cases) == len(L.CASES), 'duplicate cases'
    missing = [e for e in entries if e not in cases and e[2] not in ALLOWED]
    assert not missing, f'launches of the benchmarked steps without a float64 case: {missing}'
    stale = [c for c in L.CASES if c not in entries]
    assert not stale, f'cases the benchmarked plans no longer launch: {stale}'
    assert all(c[2] not in ALLOWED for c in L.CASES)


def test_every_case_family_has_a_bar():
    for c in L.CASES:
        f = L.family(c[2])
        assert f == 'maxpool_fwd' or f == 'wgrad_reduce_batched' or f in L.FAMILIES or f in L.LOSS_FAMILIES, c


def offbench_entries(points):
    from squeezedet_pytorch_amd import plan
    out = []
    for arch, batch, size in points:
        for planner in (plan.inference_launch_plan, plan.training_launch_plan):
            for kernel, tag in planner(arch, batch, size):
                e = (arch, batch, size, kernel, tag)
                if e not in out:
                    out.append(e)
    return out


def _same_as_plans(cases, entries, what, name_at=3):
    """``name_at``: where a case holds its kernel name."""
    assert len(set(cases)) == len(cases), 'duplicate cases'
    missing = [e for e in entries if e not in set(cases) and e[name_at] not in ALLOWED]
    assert not missing, f'launches of {what} without a float64 case: {missing}'
    stale = [c for c in cases if c not in entries]
    assert not stale, f'cases the plans of {what} no longer launch: {stale}'
    assert all(c[name_at] not in ALLOWED for c in cases)


def test_every_offbench_plan_entry_has_a_case():
    assert OB.POINTS == [('squeezedet', 1, (192, 624)), ('squeezedetplus', 1, (192, 624)), ('squeezedet', 3, (70, 100)),
                         ('squeezedetplus', 3, (70, 100)), ('squeezedet', 2, (186, 310)), ('squeezedet', 1, (48, 48))]
    _same_as_plans(OB.OFFBENCH, offbench_entries(OB.POINTS), 'the off-benchmark points')


def test_every_forced_form_entry_has_a_case():
    """The forced-forms point, recomputed under the same swap of look-ups the GPU test runs with; the swap reaches the forms it is for,
    and leaves the look-ups and the schedule memo as it found them."""
    from squeezedet_pytorch_amd import ops, plan
    assert OB.FORCED_POINT == ('squeezedet', 3, (70, 100))
    before = (ops.choose_fire_bridge_cfg, ops.choose_fire_pool_bridge, ops.choose_wino_cfg)
    plain = plan.training_launch_plan(*OB.FORCED_POINT)
    with OB.forced_forms():
        entries = offbench_entries([OB.FORCED_POINT])
    assert (ops.choose_fire_bridge_cfg, ops.choose_fire_pool_bridge, ops.choose_wino_cfg) == before
    assert plan.training_launch_plan(*OB.FORCED_POINT) == plain
    _same_as_plans(OB.FORCED, entries, 'the forced-forms point')
    fams = {L.family(c[3]) for c in OB.FORCED}
    assert {'conv_wino_us', 'conv_wino_vs', 'fire_bridge', 'fire_bridge_save', 'fire_pool_bridge', 'fire_pool_bridge_save'} <= fams


def test_every_offbench_case_family_has_a_bar():
    known = set(L.FAMILIES) | set(L.LOSS_FAMILIES) | set(OB.NEW_FAMILIES) | {'maxpool_fwd', 'wgrad_reduce_batched'}
    for c in OB.OFFBENCH + OB.FORCED:
        assert L.family(c[3]) in known, c
    # the new families launch at the point their teeth are taken from
    for f in OB.NEW_FAMILIES:
        assert f not in L.FAMILIES and any(c[:3] == OB.TEETH_POINT and L.family(c[3]) == f for c in OB.OFFBENCH), f


# the grid of the reachability check: both architectures at these batches and input sizes
GRID_BATCHES = (1, 2, 3, 4, 5, 8, 16, 20, 32, 64)
GRID_SIZES = ((384, 1248), (192, 624), (256, 832), (512, 1664), (64, 96), (70, 100))


def test_every_reachable_kernel_has_a_case():
    """Every kernel name either planner produces over the grid has a float64 case, in the benchmarked sweep or the off-benchmark one.
    The only exceptions are the six tilings the planners name above about 2.4 M pixels alone; they are compiled configurations, which
    test_every_compiled_tiling runs.  A tuning row or a heuristic change that makes another instance reachable fails here until it
    has a case."""
    from squeezedet_pytorch_amd import ops, plan
    names = set()
    for arch in ('squeezedet', 'squeezedetplus'):
        for batch in GRID_BATCHES:
            for size in GRID_SIZES:
                for planner in (plan.inference_launch_plan, plan.training_launch_plan):
                    names |= {kernel for kernel, _tag in planner(arch, batch, size)}
    covered = {c[2] for c in L.CASES} | {c[3] for c in OB.OFFBENCH} | set(ALLOWED)
    large = ['conv_dma<1,16,2,4,4>', 'conv_dma<1,32,2,1,4>', 'conv_dma<1,32,2,2,4>', 'conv_dma<9,16,2,2,4>', 'conv_dma<9,16,2,3,4>',
             'conv_dma<9,16,2,4,4>']
    assert OB.LARGE_PIXEL_TILINGS == large
    assert not set(large) & covered, 'a large-pixel tiling has a case now: take it off the exception list'
    missing = sorted(names - covered - set(large))
    assert not missing, f'kernel instances the planners can name without a float64 case: {missing}'
    compiled = {ops.cfg_kernel_name(cid) for cid, (taps, _kc, _px, _bn) in ops.cfg_table().items()
                if ops.conv_cfg_ok(cid, OB.TILING_SHAPES[taps][0])}
    assert set(large) <= compiled, sorted(set(large) - compiled)


# ---- the head axis: class counts, anchors per cell, sparse ground truth (tests/test_fp64_widths_gpu.py) ----

def _width_plans(arch, apg, C, sparse=False):
    from squeezedet_pytorch_amd import plan
    return (plan.inference_launch_plan(arch, WD.BATCH, WD.SIZE, anchors_per_grid=apg, num_classes=C),
            plan.training_launch_plan(arch, WD.BATCH, WD.SIZE, anchors_per_grid=apg, num_classes=C, sparse_gt=sparse))


def width_entries(points):
    """The ConvDet-side rows of both plans of every point, as WIDTHS cases."""
    out = []
    for pt in points:
        arch, apg, C, _sparse = pt
        for rows, train in zip(_width_plans(*pt), (False, True)):
            i0, i1 = WD.convdet_side(rows, arch, apg, C, train)
            for e in rows[i0:i1]:
                if pt + e not in out:
                    out.append(pt + e)
    return out


def test_every_width_plan_entry_has_a_case():
    """WIDTHS equals the planners' ConvDet-side rows at POINTS: nothing missing, nothing stale (``detect`` stays with its own sweep)."""
    assert WD.POINTS == [('squeezedet', 9, 7, False), ('squeezedet', 9, 255, True), ('squeezedet', 20, 7, False),
                         ('squeezedet', 4, 6, False), ('squeezedet', 3, 7, False), ('squeezedet', 4, 3, False),
                         ('squeezedet', 1, 3, False), ('squeezedet', 16, 3, False), ('squeezedet', 9, 1, False),
                         ('squeezedet', 9, 20, False), ('squeezedet', 9, 256, True), ('squeezedetplus', 9, 20, True)]
    assert (WD.BATCH, WD.SIZE) == (3, (70, 100))
    _same_as_plans(WD.WIDTHS, width_entries(WD.POINTS), 'the head-axis points', name_at=4)
    assert set(WD.TEETH_POINTS) <= set(WD.POINTS) and all(pt in WD.POINTS for pt in WD.GT_SEED)
    # every case family has a bar: a GEMM family of the older sweeps (k from ``L.k_of``), a loss launch, or one of the exact launches
    known = set(L.FAMILIES) | set(L.LOSS_FAMILIES) | set(OB.NEW_FAMILIES) | {'loss_sparse_fwd', 'loss_sparse_bwd', 'convdet_pack',
                                                                             'convdet_unpack', 'wgrad_reduce_rows'}
    assert all(L.family(c[4]) in known for c in WD.WIDTHS)
    # the teeth points launch what their teeth are taken from
    for pt, fams in WD.TEETH_POINTS.items():
        kernels = {c[4] for c in WD.WIDTHS if c[:4] == pt}
        for f in fams:
            if f == 'conv_wgrad':
                assert 'conv_wgrad<9>' in kernels, pt
            elif 'sparse' in f:
                assert f in kernels and pt[3], (pt, f)
            else:
                from squeezedet_pytorch_amd import ops
                assert ops.head_path(pt[2]) == 'many' and not pt[3] and f.replace('_many', '') in kernels, (pt, f)


def test_width_points_run_a_checked_backbone():
    """Why the head-axis sweep may pass the backbone through unchecked: outside the ConvDet side the launches of every point are, name and
    tag, those of the off-benchmark sweep's point of the same architecture at batch 3, 70x100 (all of which have float64 cases there).
    The one row that differs is the batched slab reduction of a padded point: ConvDet's slabs are reduced on their own
    (``wgrad_reduce_rows``), which leaves it 30 layers instead of 31."""
    from squeezedet_pytorch_amd import ops
    for pt in WD.POINTS:
        arch, apg, C, sparse = pt
        assert (arch, WD.BATCH, WD.SIZE) in OB.POINTS
        checked = {c[3:] for c in OB.OFFBENCH if c[:3] == (arch, WD.BATCH, WD.SIZE)} | {(k, None) for k in ALLOWED}
        for rows, base, train in zip(_width_plans(*pt), _width_plans(arch, 9, 3), (False, True)):
            i0, i1 = WD.convdet_side(rows, arch, apg, C, train)
            j0, j1 = WD.convdet_side(base, arch, 9, 3, train)
            assert rows[:i0] == base[:j0], pt
            tail, want = rows[i1:], base[j1:]
            if train and ops.convdet_padded(apg, C):
                assert tail[-1] == ('wgrad_reduce_batched', '30 layers') and want[-1] == ('wgrad_reduce_batched', '31 layers'), pt
                tail, want = tail[:-1], want[:-1]
            if train:
                assert tail == want, pt
            assert all(e in checked or (e[0], None) in checked for e in rows[:i0] + tail), pt


# ---- the step with a live dropout (tests/test_fp64_dropout_gpu.py) ----

def test_every_dropout_plan_entry_has_a_case():
    """``DR.CASES`` equals the planners' rows from the last Fire's expand launches through ConvDet's data gradient at its points, for
    both values of ``fused_dropout`` (the injected form runs the stand-alone form's launches without the ``dropout_mask`` row, which has
    its own bit-exact test); the rest of those plans -- the backbone, passed through unchecked -- is, name and tag, what the
    off-benchmark sweep checks at batch 3, 70x100."""
    assert DR.POINTS == [('squeezedet', 0.5), ('squeezedetplus', 0.5), ('squeezedet', 0.2)]
    assert (DR.BATCH, DR.SIZE) == (3, (70, 100)) and DR.FORMS == ('fused', 'standalone', 'injected')
    entries = []
    for arch, p in DR.POINTS:
        assert (arch, DR.BATCH, DR.SIZE) in OB.POINTS
        checked = {c[3:] for c in OB.OFFBENCH if c[:3] == (arch, DR.BATCH, DR.SIZE)}
        for form in DR.FORMS:
            rows = DR.planned(arch, form)
            i0, i1 = DR.dropout_side(rows, arch)
            masks = [r for r in rows[:i0] if r[0] == 'dropout_mask']
            assert len(masks) == (1 if form == 'standalone' else 0), (arch, form, masks)
            entries += [(arch, p, form) + e for e in masks + rows[i0:i1]]
            assert all(e in checked or e[0] in ALLOWED for e in rows[:i0] + rows[i1:]), (arch, form)
    _same_as_plans(DR.CASES, entries, 'the live-dropout points', name_at=3)
    known = set(L.FAMILIES) | set(L.LOSS_FAMILIES) | set(OB.NEW_FAMILIES)
    assert all(L.family(c[3]) in known for c in DR.CASES)
    # the fused form is the one the planners choose by default, and it needs no mask launch
    from squeezedet_pytorch_amd import plan
    for arch, _p in DR.POINTS:
        assert DR.planned(arch, 'fused') == plan.training_launch_plan(arch, DR.BATCH, DR.SIZE)


@contextlib.contextmanager
def _memoized_lookups():
    """The two table look-ups every 3x3 and 1x1 row goes through, memoized for the grid walk below (they are pure functions of their
    arguments and the loaded table; the planners read them through ``ops``).  Restored afterwards, schedule memos cleared, as
    ``OB.forced_forms`` does."""
    from squeezedet_pytorch_amd import ops, plan
    saved = {n: getattr(ops, n) for n in ('choose_cfg', 'choose_wino_cfg')}
    plan.forward_schedule.cache_clear(); plan.backward_schedule.cache_clear()
    for n, f in saved.items():
        setattr(ops, n, functools.lru_cache(maxsize=None)(f))
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        plan.forward_schedule.cache_clear(); plan.backward_schedule.cache_clear()


HEAD_GRID_ANCHORS = range(1, 21)
HEAD_GRID_CLASSES = range(1, 257)


def convdet_signature(arch, apg, C):
    """What decides ConvDet's launches at (anchors per cell, classes): (padded or not, the forward kernel family, the weight-gradient
    kernel name, the data-gradient kernel family, the run width mod 16 if it is <= 80 else whether it is a multiple of 64, the run
    width mod 16 where the data gradient is a direct kernel)."""
    from squeezedet_pytorch_amd import ops
    rows = _width_plans(arch, apg, C)[1]
    i0, i1 = WD.convdet_side(rows, arch, apg, C, True)
    side = rows[i0:i1]
    n, nrun = ops.convdet_width(apg, C)
    wg, = [k for k, t in side if t.startswith('wgrad ')]
    dg = L.family(side[-1][0])
    return (n != nrun, L.family(side[0][0]), wg, dg, nrun % 16 if nrun <= 80 else nrun % 64 == 0, None if 'wino' in dg else nrun % 16)


def test_every_reachable_head_kernel_and_convdet_signature_has_a_case():
    """Over 1..20 anchors per cell x 1..256 classes x dense / sparse ground truth at batch 3, 70x100, for both architectures: every
    kernel name either planner produces has a float64 case (``CASES``, ``OFFBENCH`` or ``WIDTHS``), and every ConvDet signature
    (``convdet_signature``) occurs at a point of the head-axis sweep.  Both head paths and both kinds of loss launch occur there too."""
    from squeezedet_pytorch_amd import ops
    covered = {c[2] for c in L.CASES} | {c[3] for c in OB.OFFBENCH} | {c[4] for c in WD.WIDTHS} | set(ALLOWED)
    at_points = {convdet_signature(*pt[:3]) for pt in WD.POINTS}
    with _memoized_lookups():
        for arch in ('squeezedet', 'squeezedetplus'):
            names, sigs = set(), {}
            for apg in HEAD_GRID_ANCHORS:
                for C in HEAD_GRID_CLASSES:
                    for sparse in (False, True):
                        for rows in _width_plans(arch, apg, C, sparse):
                            names |= {kernel for kernel, _tag in rows}
                    sigs.setdefault(convdet_signature(arch, apg, C), (apg, C))
            missing = sorted(names - covered)
            assert not missing, f'{arch}: kernel instances the planners can name along the head axis without a float64 case: {missing}'
            new = {s: at for s, at in sigs.items() if s not in at_points}
            assert not new, f'{arch}: ConvDet signatures (first at anchors, classes) that no point of the head-axis sweep runs: {new}'
            print(f'{arch}: {len(names)} kernel names, {len(sigs)} ConvDet signatures over the head grid')
    assert {ops.head_path(pt[2]) for pt in WD.POINTS} == {'narrow', 'many'}
    kernels = {c[4] for c in WD.WIDTHS}
    assert {'loss_fwd', 'loss_bwd', 'loss_sparse_fwd', 'loss_sparse_bwd'} <= kernels
    # the many-class launches are bracketed under the dense names: a dense point past 16 classes runs them
    assert any(ops.head_path(pt[2]) == 'many' and not pt[3] for pt in WD.POINTS)


def _reduce_rows_numpy(slab, S, N, Npad, C, taps, stride_rows=None, bias_off=None, slabs=None):
    """csrc/convdet_pad.hip's wgrad_reduce_rows restated in numpy (float32, the slabs added in ascending order): slab s starts at
    s * (Npad * taps * C + Npad) and holds [Npad][taps][C] weight sums, then [Npad] bias sums.  -> (dw [N,C,k,k], db [N]).  The keyword
    arguments are the wrong variants of the teeth: the slab stride from another row count, another bias offset, a subset of the slabs."""
    import numpy as np
    k = 3 if taps == 9 else 1
    stride_rows = Npad if stride_rows is None else stride_rows
    stride = stride_rows * taps * C + stride_rows
    bias_off = Npad * taps * C if bias_off is None else bias_off
    dw = np.zeros((N, taps, C), np.float32)
    db = np.zeros(N, np.float32)
    for s in (range(S) if slabs is None else slabs):
        dw += slab[s * stride:s * stride + N * taps * C].reshape(N, taps, C)
        db += slab[s * stride + bias_off:s * stride + bias_off + N]
    return dw.transpose(0, 2, 1).reshape(N, C, k, k), db


def test_reduce_rows_restatement_and_its_teeth():
    """The numpy restatement of ``wgrad_reduce_rows`` holds bar L against the float64 sum of the true rows on the (54 of 64, C768) layout;
    reading the slabs at the stride of N instead of Npad rows, taking the bias from offset N * taps * C, or dropping one slab fails it."""
    import numpy as np
    S, N, Npad, C, taps = 3, 54, 64, 768, 9
    rs = np.random.RandomState(54)
    stride = Npad * taps * C + Npad
    slab = rs.standard_normal(S * stride).astype(np.float32)
    s64 = slab.astype(np.float64).reshape(S, stride)
    w64 = s64[:, :Npad * taps * C].reshape(S, Npad, taps, C)[:, :N]
    b64 = s64[:, Npad * taps * C:][:, :N]
    ref_w, M_w = w64.sum(0).transpose(0, 2, 1).reshape(N, C, 3, 3), np.abs(w64).sum(0).transpose(0, 2, 1).reshape(N, C, 3, 3)
    ref_b, M_b = b64.sum(0), np.abs(b64).sum(0)

    def holds(dw, db):
        return bool((np.abs(dw - ref_w) <= R.BAR_L * M_w).all()), bool((np.abs(db - ref_b) <= R.BAR_L * M_b).all())
    assert holds(*_reduce_rows_numpy(slab, S, N, Npad, C, taps)) == (True, True)
    # rows at stride N: the slabs are taken N * taps * C + N floats apart (slab 0 still lines up, the later ones do not)
    assert holds(*_reduce_rows_numpy(slab, S, N, Npad, C, taps, stride_rows=N)) == (False, False)
    # the bias from offset N * taps * C: weight sums of row N land in db
    assert holds(*_reduce_rows_numpy(slab, S, N, Npad, C, taps, bias_off=N * taps * C)) == (True, False)
    # one slab dropped
    for drop in range(S):
        assert holds(*_reduce_rows_numpy(slab, S, N, Npad, C, taps, slabs=[s for s in range(S) if s != drop])) == (False, False), drop


def test_wgrad_blocking_restates_the_launchers():
    """L.wgrad_blocking against the host's own split rule: the launchers refuse S above their number of pixel blocks, so the blocks of the
    restatement must be at least as many as the S ``tiles.wgrad_split`` hands out; and the tile forms at the widths of both models."""
    from squeezedet_pytorch_amd import ops
    assert L.wgrad_blocking('squeeze_bwd', 64, 16, 1) == (('px', 32), 1)
    assert L.wgrad_blocking('conv_wgrad_group', 64, 16, 1) == (('px', 64), 1)           # tc 1: launch_wgrad_group<4, 1, 4>
    assert L.wgrad_blocking('conv_wgrad_group', 192, 48, 1) == (('px', 32), 1)          # tc 3
    assert L.wgrad_blocking('conv_wgrad_group', 256, 384, 1) == (('px', 32), 1)         # tc 8
    assert L.wgrad_blocking('conv_wgrad', 384, 512, 1) == (('px', 32), 1)               # launch_wgrad<1, 4, 8, 2>
    assert L.wgrad_blocking('conv_wgrad', 16, 16, 1) == (('px', 128), 1)                # launch_wgrad<1, 1, 1, 8>
    assert L.wgrad_blocking('conv_wgrad', 32, 32, 1) == (('px', 64), 1)                 # launch_wgrad<1, 2, 2, 4>
    assert L.wgrad_blocking('conv_wgrad_wino', 72, 768, 9) == ('tile', 16)
    assert L.wgrad_blocking('conv_wgrad_wino_group', 64, 16, 9) == ('tile', 16)
    # the 9-tap rows of the head-axis sweep: the direct 3x3 form takes 4x16-pixel tiles one pixel per accumulation whatever its
    # out-channel tiling (N 108: a partial tile; 2340: 147 tiles), the N <= 80 Winograd form 4x16 groups, 16 pixels per step
    for N in (108, 240, 2340):
        assert not ops.wgrad_uses_wino(N, 768, 9, 3, 4, 6)
        assert L.wgrad_blocking('conv_wgrad', N, 768, 9) == ('tile', 1)
    for N in (8, 36, 44):
        assert ops.wgrad_uses_wino(N, 768, 9, 3, 4, 6)
        assert L.wgrad_blocking('conv_wgrad_wino', N, 768, 9) == ('tile', 16)
    for N in (108, 240, 2340, 8, 36, 44, 64, 256, 2368):                # S never exceeds the 4x16 tile groups of the 3 x 4x6 grid
        assert ops.wgrad_split(N, 768, 9, 3, 4, 6)[0] <= 3
    for B, H, W in ((1, 3, 3), (3, 4, 6), (2, 11, 19), (1, 12, 39), (20, 24, 78)):
        for N, C in ((192, 128), (384, 512), (288, 256), (16, 16), (96, 64)):
            S, _ = ops.wgrad_split(N, C, 1, B, H, W)
            (_px, P), _step = L.wgrad_blocking('conv_wgrad', N, C, 1)
            assert S <= -(-(B * H * W) // P), (B, H, W, N, C, S, P)


def test_wgrad_tile_form_agrees_with_the_restatement():
    """The library's own tile-form rule (``sqd_wgrad_tile_form``, the one the host sizes its splits from) against the independent
    restatement ``L.wgrad_blocking`` on pixels per block, over every width the rule branches on (N up to 128 in steps of 4, the wide
    and ConvDet widths; C likewise) for the plain entry at 1 and 9 taps and the grouped and fused entries where they accept the shape;
    and ``tiles.wgrad_split``'s S within the library's own block count on the grids of the test above."""
    from squeezedet_pytorch_amd import ops, tiles
    Ns = list(range(4, 129, 4)) + [192, 256, 288, 384, 2340]
    Cs = list(range(4, 65, 4)) + [96, 128, 256, 384, 512, 768]
    grids = ((1, 3, 3), (3, 4, 6), (2, 11, 19), (1, 12, 39), (20, 24, 78))
    seen = {tiles.WGRAD_GROUP: 0, tiles.WGRAD_FUSED: 0}
    for N in Ns:
        for C in Cs:
            tn, tc, px = tiles.wgrad_tile_form(tiles.WGRAD_PLAIN, 1, N, C)
            assert L.wgrad_blocking('conv_wgrad', N, C, 1) == (('px', px), 1), (N, C, px)
            assert tn * 16 >= min(N, 64) and tc * 16 >= min(C, 64), (N, C, tn, tc)
            tn9, tc9, px9 = tiles.wgrad_tile_form(tiles.WGRAD_PLAIN, 9, N, C)
            assert L.wgrad_blocking('conv_wgrad', N, C, 9) == ('tile', 1) and px9 == 4 * 16, (N, C, px9)      # 'tile': 4x16-pixel windows
            forms = {(1, False): (tn, tc, px), (9, False): (tn9, tc9, px9)}
            grp = tiles.wgrad_tile_form(tiles.WGRAD_GROUP, 1, N, C)
            assert (grp is not None) == (N >= 64 and not 64 < N <= 96), (N, C)
            if grp is not None:
                assert L.wgrad_blocking('conv_wgrad_group', N, C, 1) == (('px', grp[2]), 1), (N, C, grp)
                assert grp == (tn, tc, px), (N, C, grp)                # bitwise the slabs of sqd_conv_wgrad: the same form
                seen[tiles.WGRAD_GROUP] += 1
            fus = tiles.wgrad_tile_form(tiles.WGRAD_FUSED, 1, N, C)
            assert (fus is not None) == (N <= 128), (N, C)
            if fus is not None:
                assert L.wgrad_blocking('squeeze_bwd', N, C, 1) == (('px', fus[2]), 1), (N, C, fus)
                assert fus[0] * 16 >= N, (N, C, fus)                   # all of N in one out-channel group
                forms[(1, True)] = fus
                seen[tiles.WGRAD_FUSED] += 1
            for (taps, fused), (_tn, _tc, p) in forms.items():
                for B, H, W in grids:
                    S, stride = ops.wgrad_split(N, C, taps, B, H, W, wino=False, fused_dgrad=fused)
                    blocks = B * -(-H // (p // 16)) * -(-W // 16) if taps == 9 else -(-(B * H * W) // p)
                    assert 1 <= S <= blocks and stride == N * taps * C + N, (N, C, taps, fused, B, H, W, S, blocks)
    assert seen[tiles.WGRAD_GROUP] == 14 * len(Cs) and seen[tiles.WGRAD_FUSED] == 32 * len(Cs)
    for kind in (tiles.WGRAD_GROUP, tiles.WGRAD_FUSED):                # 1x1 entries only
        assert tiles.wgrad_tile_form(kind, 9, 64, 64) is None


def _rand(*shape, seed, relu=False):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g, dtype=torch.float64)
    return t.clamp_min(0) if relu else t


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('k', [1, 3])
def test_reference_conv_dgrad_wgrad(k):
    x = _rand(2, 5, 6, 7, seed=1, relu=True)
    w = _rand(8, 5, k, k, seed=2)
    b = _rand(8, seed=3)
    want = F.conv2d(x, w, b, padding=k // 2)
    r = R.conv(_nhwc(x), w, b)
    assert torch.allclose(r.ref64, _nhwc(want), atol=1e-12)
    assert (r.M >= r.ref64.abs() - 1e-12).all()
    assert torch.allclose(r.b32.double(), r.ref64, atol=1e-5)
    xg = x.clone().requires_grad_(True); wg = w.clone().requires_grad_(True); bg = b.clone().requires_grad_(True)
    dy = _rand(*want.shape, seed=4)
    F.conv2d(xg, wg, bg, padding=k // 2).backward(dy)
    assert torch.allclose(R.conv(_nhwc(dy), R.dgrad_weight(w)).ref64, _nhwc(xg.grad), atol=1e-12)
    dW, db = R.wgrad(_nhwc(dy), _nhwc(x), k * k)
    assert torch.allclose(dW.ref64, wg.grad, atol=1e-12) and torch.allclose(db.ref64, bg.grad, atol=1e-12)


def test_reference_fire_expand():
    """R.fire_expand (the reference of the ``ops.fire_expand`` wrapper) against torch's own conv2d in float64: relu(expand1x1) next to
    relu(expand3x3) in the channel window, magnitude above |ref64|, the float32 chain inside bar L."""
    x = _rand(2, 6, 5, 7, seed=41, relu=True)
    w1, b1 = _rand(8, 6, 1, 1, seed=42), _rand(8, seed=43)
    w3, b3 = _rand(8, 6, 3, 3, seed=44), _rand(8, seed=45)
    want = torch.cat([F.relu(F.conv2d(x, w1, b1)), F.relu(F.conv2d(x, w3, b3, padding=1))], 1)
    r = R.fire_expand(_nhwc(x), w1, b1, w3, b3)
    assert tuple(r.ref64.shape) == (2, 5, 7, 16)
    assert torch.allclose(r.ref64, _nhwc(want), atol=1e-12)
    assert (r.M >= r.ref64.abs() - 1e-12).all()
    assert ((r.b32.double() - r.ref64).abs() <= R.BAR_L * r.M).all()
    assert R.bars(r.b32, r, 'act', 2)['p_ok']
    for emu in ('bf16', 'split3'):
        assert not R.bars(R.fire_expand(_nhwc(x), w1, b1, w3, b3, emu=emu).b32, r, 'act', 2)['p_ok'], emu


def test_reference_direct3x3_chain():
    """The restated float32 chain of the direct kernels (one accumulator over chunk x tap x 4-channel step) is the same
    convolution: inside bar L of float64 and bar P of itself; ref64 and M are those of the plain reference; and the plain per-tap chain
    is the more accurate one on a long reduction (why the restatement exists), so a kernel of that structure cannot be held to it."""
    x = _rand(1, 5, 7, 200, seed=61, relu=True).float()
    w = (_rand(12, 200, 3, 3, seed=62) * (2.0 / 1800) ** 0.5).float()
    b = _rand(12, seed=63).float()
    plain, chain = R.conv(x, w, b, relu=True), R.conv(x, w, b, relu=True, chain_kc=16)
    assert torch.equal(plain.ref64, chain.ref64) and torch.equal(plain.M, chain.M)
    assert ((chain.b32.double() - chain.ref64).abs() <= R.BAR_L * chain.M).all()
    assert R.bars(chain.b32, chain, 'act', 2)['p_ok']
    e_plain = (plain.b32.double() - plain.ref64).pow(2).mean().sqrt()
    e_chain = (chain.b32.double() - chain.ref64).pow(2).mean().sqrt()
    assert e_chain > e_plain
    for emu in ('bf16', 'split3'):
        assert not R.bars(R.conv(x, w, b, relu=True, emu=emu, chain_kc=16).b32, chain, 'act', 2)['p_ok'], emu
    # a 1x1 layer has one tap: the chain is the plain one up to what the matmul does inside a step
    w1 = w[:, :, 1:2, 1:2].contiguous()
    assert R.bars(R.conv(x, w1, b, chain_kc=16).b32, R.conv(x, w1, b), 'act', 2)['p_ok']


@pytest.mark.parametrize('H,W', [(35, 50), (50, 35), (12, 12), (11, 19)])
def test_reference_pool_at_mixed_parity(H, W):
    """R.maxpool_exact against torch's ceil-mode pool where rows and columns differ in parity (the padding of each axis is its own)."""
    x = _rand(2, 3, H, W, seed=64)
    want = F.max_pool2d(x, 3, 2, ceil_mode=True)
    assert torch.equal(R.maxpool_exact(_nhwc(x)), _nhwc(want))


@pytest.mark.parametrize('k,H,W', [(3, 13, 18), (7, 14, 17)])
def test_reference_stem_pool_and_backward(k, H, W):
    img = _rand(2, 3, H, W, seed=5)
    w = _rand(6, 3, k, k, seed=6).requires_grad_(True)
    b = _rand(6, seed=7).requires_grad_(True)
    s = F.relu(F.conv2d(img, w, b, stride=2, padding=k // 2))
    p, idx = F.max_pool2d(s, 3, 2, ceil_mode=True, return_indices=True)
    r = R.stem_pool(img, w.detach(), b.detach())
    assert torch.allclose(r.ref64, _nhwc(p.detach()), atol=1e-12)
    # the kernel's codes: tap of the window (15 where the pooled value is not > 0, the ReLU mask)
    Ho, Wo = p.shape[2:]
    Ws = s.shape[3]
    oy = torch.arange(Ho).view(1, 1, Ho, 1) * 2
    ox = torch.arange(Wo).view(1, 1, 1, Wo) * 2
    codes = (idx // Ws - oy) * 3 + (idx % Ws - ox)
    codes = torch.where(p > 0, codes, torch.full_like(codes, 15)).to(torch.uint8)
    dp = _rand(*p.shape, seed=8)
    p.backward(dp)
    dW, db = R.stem_wgrad_pooled(_nhwc(dp), _nhwc(codes), img, 6, k)
    assert torch.allclose(dW.ref64, w.grad, atol=1e-10) and torch.allclose(db.ref64, b.grad, atol=1e-10)
    sp = _nhwc(s.detach())
    dx = R.maxpool_bwd(_nhwc(dp), _nhwc(codes), sp.shape[1:3])
    sg = s.detach().clone().requires_grad_(True)
    F.max_pool2d(sg, 3, 2, ceil_mode=True).backward(dp * (p > 0))
    assert torch.allclose(dx.ref64, _nhwc(sg.grad), atol=1e-12)


def test_reference_bridge_magnitude_bounds_the_fp32_chain():
    x = _rand(2, 9, 11, 8, seed=9, relu=True).float()
    ws = [_rand(*s, seed=10 + i).float() * 0.3 for i, s in enumerate([(4, 8, 1, 1), (4,), (4, 8, 3, 3), (4,), (8, 8, 1, 1), (8,)])]
    for y, mid in (R.fire_bridge(x, *ws), R.fire_pool_bridge(x, *ws)):
        for r in (y, mid):
            assert ((r.b32.double() - r.ref64).abs() <= R.BAR_L * r.M).all()
            assert R.bars(r.b32, r, 'act', 2)['p_ok']


def test_bars_reject_a_misplaced_term_and_the_emulations():
    x = _rand(4, 12, 12, 64, seed=20).abs().float()
    w = _rand(64, 64, 3, 3, seed=21).float() * 0.05
    b = _rand(64, seed=22).float()
    r = R.conv(x, w, b)
    got = r.b32.clone()
    assert R.bars(got, r, 'act', 2)['l_ok']
    got[1, 5, 7, 3] += float(w[3, 7, 1, 1] * x[1, 5, 7, 7])          # one duplicated product
    assert not R.bars(got, r, 'act', 2)['l_ok']
    for emu in ('bf16', 'split3'):
        assert not R.bars(R.conv(x, w, b, emu=emu).b32, r, 'act', 4)['p_ok'], emu


@pytest.mark.parametrize('taps,S,blocking,step', [(1, 3, ('px', 32), 4), (1, 5, ('px', 128), 4), (9, 4, 'tile', 16), (9, 1, 'tile', 16)])
def test_reference_split_k_restatement(taps, S, blocking, step):
    dy = _rand(2, 9, 37, 8, seed=30, relu=True)
    x = _rand(2, 9, 37, 12, seed=31, relu=True)
    dW, db = R.wgrad(dy, x, taps)
    w32, b32 = R.wgrad_split_k(dy, x, taps, S, blocking, step)
    assert w32.dtype == torch.float32 and tuple(w32.shape) == tuple(dW.ref64.shape)
    assert ((w32.double() - dW.ref64).abs() <= R.BAR_L * dW.M).all()
    assert ((b32.double() - db.ref64).abs() <= R.BAR_L * db.M).all()
    assert R.bars(w32, R.Ref(dW.ref64, dW.M, w32), 'wgrad', 2)['p_ok']


# ---- the loss ----

def _bench_like(B=4, seed=11):
    """Operands shaped like the benchmarked loss launch: the KITTI anchors (A = 16848), the synthetic head's scales, synthetic gt."""
    import numpy as np
    import squeezedet_pytorch_amd as sqd
    from squeezedet_pytorch_amd import synthetic
    cfg = sqd.make_cfg()
    rs = np.random.RandomState(seed)
    pred = (rs.standard_normal((B, cfg.num_anchors, 8)) * np.array([2, 2, 2, 1.5, .4, .4, .4, .4])).astype(np.float32)
    pred[..., 3] -= 2.0
    gt = synthetic.make_gt(B, cfg.anchors, cfg.input_size, seed=1)
    return torch.from_numpy(pred), gt, torch.from_numpy(cfg.anchors).float(), cfg.input_size


def _loss_cases():
    yield 'bench', _bench_like(), 3
    for C in (1, 3, 16):
        yield f'edges C{C}', LG.edge_case(C=C) + (LG.SIZE,), C
    yield 'saturated', LG.saturated_case() + (LG.SIZE,), 3
    yield 'n_obj 0 and A', LG.random_case(4, 500, 3, seed=300, nobj=[37, 0, 500, 11]) + (LG.SIZE,), 3
    yield 'A1', LG.random_case(2, 1, 3, seed=101) + (LG.SIZE,), 3


_LOSS_REFS = {}


def _loss_ref(name, ops, C, mutant=None):
    key = (name, mutant)
    if key not in _LOSS_REFS:
        pred, gt, anchors, size = ops
        _LOSS_REFS[key] = R.loss(pred, gt, anchors, size, C, LG.WEIGHTS, gmean=LG.GMEAN, coef=LG.make_coef(pred.shape[0], 3), mutant=mutant)
    return _LOSS_REFS[key]


@pytest.mark.parametrize('name,ops,C', list(_loss_cases()), ids=[c[0] for c in _loss_cases()])
def test_loss_reference_attainable(name, ops, C):
    """The float32 oracle chain (torch autograd in float32 on the host) holds bar L with 4x headroom on every output of every edge case
    and on bench-shaped operands, and bar P trivially; nobj is exact; no exact construction flips a branch."""
    ref = _loss_ref(name, ops, C)
    for out in ('losses', 'mean4', 'dmean', 'dcoef'):
        r = ref[out]
        b = R.bars_nan(r.b32, r, 'dpred' if out[0] == 'd' else 'vec', 2)
        print(f'{name:16s} {out:7s} float32 chain max err/M {b["l_ratio"]:.2e}')
        assert b['nan_ok'] and b['l_ratio'] <= R.BAR_L / 4, (name, out, b)
    assert torch.equal(ref['nobj'], ops[1][..., 0].double().sum(1))
    assert int(ref['flips'].sum()) <= (4 if name == 'bench' else 0)


def test_loss_reference_matches_autograd():
    """The analytic chain (which M and the flipped-branch and mutant references come from) equals float64 autograd of the oracle, and
    torch 2.10's conventions are the ones it pins: clamp inclusive, ties split, clamp_min inclusive."""
    x = torch.tensor([0.0, 1.0, 5.0], dtype=torch.float64, requires_grad=True)
    x.clamp(0, 5).sum().backward()
    assert x.grad.tolist() == [1.0, 1.0, 1.0]
    a = torch.tensor([1.0, 2.0], dtype=torch.float64, requires_grad=True)
    torch.min(a, torch.ones(2, dtype=torch.float64)).sum().backward()
    assert a.grad.tolist() == [0.5, 0.0]
    y = torch.tensor([0.0, -1.0], dtype=torch.float64, requires_grad=True)
    torch.clamp_min(y, 0).sum().backward()
    assert y.grad.tolist() == [1.0, 0.0]
    for name, ops, C in _loss_cases():
        pred, gt, anchors, size = ops
        B = pred.shape[0]
        ref = _loss_ref(name, ops, C)
        br = R._branches(*R._box64(pred, anchors, C), gt, size[1] - 1, size[0] - 1)
        for out, u in (('dmean', torch.full((3, B), float(torch.tensor(LG.GMEAN, dtype=torch.float32)) / B, dtype=torch.float64)),
                       ('dcoef', LG.make_coef(B, 3).double())):
            losses, _n, dp, _ = R._loss_chain(pred, gt, anchors, size, C, LG.WEIGHTS, u, br)
            r = ref[out].ref64
            fin = ~torch.isnan(r)
            assert torch.equal(torch.isnan(dp.v), ~fin), name
            assert bool(((dp.v[fin] - r[fin]).abs() <= 1e-12 * (dp.m[fin] + r[fin].abs())).all()), (name, out)
        lr = ref['losses'].ref64
        fin = ~torch.isnan(lr)
        assert torch.equal(torch.isnan(losses.v), ~fin)
        assert bool(((losses.v[fin] - lr[fin]).abs() <= 1e-12 * lr[fin].abs()).all()), name


@pytest.mark.parametrize('mutant', R.LOSS_MUTANTS)
def test_loss_mutants_fail_the_edge_cases(mutant):
    """Teeth of the GPU edge tests: a kernel that implemented a wrong convention (exclusive clamp, no tie split, clamp_min passing only
    above 0, a detached IoU path, A as the negative term's denominator) would move at least one element of the edge cases beyond bar
    L.  The reference under that convention stands in for the kernel."""
    moved = []
    for name, ops, C in _loss_cases():
        if name == 'bench':
            continue
        ref, mut = _loss_ref(name, ops, C), _loss_ref(name, ops, C, mutant)
        for out in ('losses', 'dmean', 'dcoef'):
            r = ref[out]
            if not R.bars_nan(mut[out].ref64, r, 'dpred' if out[0] == 'd' else 'vec', 2)['l_ok']:
                moved.append((name, out))
    print(mutant, moved)
    assert moved, f'{mutant}: no edge case tells it from the pinned convention'
    if mutant in ('clamp_exclusive', 'no_tie_split', 'clamp_min_strict'):
        assert ('edges C3', 'dmean') in moved


def test_loss_bar_p_rejects_bf16_operands():
    pred, gt, anchors, size = _bench_like(B=2)
    ref = R.loss(pred, gt, anchors, size, 3, LG.WEIGHTS, gmean=1.0)
    l16, d16, _ = R.loss_bf16(pred, gt, anchors, size, 3, LG.WEIGHTS, gmean=1.0)
    assert not R.bars(l16, ref['losses'], 'vec', 2)['p_ok']
    assert not R.bars(d16, ref['dmean'], 'dpred', 2)['p_ok']


# ---- clip + SGD ----

@pytest.mark.parametrize('max_norm,momentum,wd', [(5.0, 0.875, 2.0 ** -13), (0.5, 0.875, 0.0), (0.0, 0.0, 2.0 ** -13), (1e3, 0.875, 2.0 ** -13)])
def test_clip_sgd_reference_matches_torch(max_norm, momentum, wd):
    """R.clip_sgd against torch's own clip_grad_norm_ + SGD (float64), over two steps (zero buffer, then a carried one); the
    hyper-parameters are float32 values (the reference rounds them as the kernel receives them)."""
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 3), (5,), (2, 3, 3, 3), (1,)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    mine = [p.detach().clone() for p in ps]
    bufs = [torch.zeros_like(p) for p in mine]
    lr = 2.0 ** -7
    opt = torch.optim.SGD(ps, lr=lr, momentum=momentum, weight_decay=wd)
    for _ in range(2):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        tn = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm > 0 else None
        opt.step()
        tn64, _coef, newp, newb = R.clip_sgd(mine, grads, bufs, lr, momentum, wd, max_norm)
        if tn is not None:
            assert abs(float(tn) - tn64) <= 1e-12 * tn64
        for p, r in zip(ps, newp):
            assert torch.allclose(p.detach(), r.ref64, rtol=1e-12, atol=1e-15)
            assert (r.M >= r.ref64.abs() - 1e-12).all()
        mine = [r.ref64 for r in newp]
        bufs = [r.ref64 for r in newb]
        if momentum > 0:
            for p, b in zip(ps, bufs):
                assert torch.allclose(opt.state[p]['momentum_buffer'], b, rtol=1e-12, atol=1e-15)


def test_norm_bar_rejects_dropped_tail_and_parts():
    """Teeth of the norm bar (2^-18 relative): a norm without the n & 3 tail fails it on the layout of total 3 and on one whose tail
    holds large values; a norm without one of the 256 partial sums fails it on the [1021] layout."""
    for sizes, big in (([3], False), (OG.TAIL_BIG, True), ([1021], False)):
        flat = OG.flat_values(sum(sizes), seed=1, big_tail=big)
        tn64 = float(flat.double().norm())
        n = flat.numel()
        nq = n >> 2
        no_tail = float(flat[:4 * nq].double().norm())
        assert abs(no_tail - tn64) > 2.0 ** -18 * tn64, sizes
        if sizes == [1021]:
            per = -(-nq // 256)
            for k in range(256):
                lo, hi = k * per, min(nq, (k + 1) * per)
                if hi <= lo:
                    continue
                keep = torch.ones(n, dtype=torch.bool)
                keep[4 * lo:4 * hi] = False
                assert abs(float(flat[keep].double().norm()) - tn64) > 2.0 ** -18 * tn64, k
