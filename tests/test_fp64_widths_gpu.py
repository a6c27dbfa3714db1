"""GPU tier: the float64 sweep of tests/test_fp64_launches_gpu.py along the head axis -- every ConvDet width class, both head paths, dense
and sparse ground truth.

ConvDet's width N = anchors_per_grid * (num_classes + 5) selects its launches (``ops.convdet_width``, ``tiles.wgrad_uses_wino``,
``plan.backward_schedule``); the two older sweeps run 9 anchors x 3 classes (N = 72) only.  Every point here is batch 3 at 70x100 (final
grid 4x6: 72 pixels, A = 24 * anchors_per_grid), one inference and one training step through the same harness (same seeds, dropout at
p = 0), with the launches asserted equal to the plan and every output of ConvDet's side held to bars L and P of tests/fp64_ref.py
(k = 2 direct, 4 Winograd), ``convdet_pack`` / ``convdet_unpack`` bit-exact, ``nobj`` exact, at most 4 branch-flip anchors.

| anchors, classes | N -> run width | what it reaches |
|---|---|---|
| 9, 7 | 108 | the direct 3x3 weight gradient ``conv_wgrad<9>``; a direct data gradient whose last K chunk holds 12 of 16 channels |
| 9, 255 (sparse) | 2340 | ``conv_wgrad<9>`` at 147 out-channel tiles, a direct data gradient with C % 16 = 4, the sparse loss at 255 classes |
| 20, 7 | 240 | ``conv_wgrad<9>`` with the balanced Winograd data gradient, A = 480 |
| 4, 6 | 44 | the N <= 80 Winograd weight gradient at N % 16 = 12, direct data gradient at C = 44 |
| 3, 7 | 36 | the same at N % 16 = 4 |
| 4, 3 | 32 | the N <= 80 form at two full 16-blocks, Winograd data gradient at C = 32 |
| 1, 3 | 8 | one anchor per cell: N = 8, A = 24 (fewer anchors than keep_top_k) |
| 16, 3 | 128 | the 64-block Winograd weight gradient on an unpadded width |
| 9, 1 | 54 -> 64 | the smallest padded ConvDet: ``convdet_pack``, ``convdet_unpack``, ``wgrad_reduce_rows``; one class |
| 9, 20 | 225 -> 256 | the padded ConvDet under the many-class loss launches |
| 9, 256 (sparse) | 2349 -> 2368 | the widest ConvDet, padded, under the sparse loss |
| squeezedetplus 9, 20 (sparse) | 225 -> 256 | the padded ConvDet on 512 input channels |

The backbone's launches are, name and tag, those of the off-benchmark sweep's 70x100 points, which checks them
(tests/test_fp64_coverage.py asserts it on the host), so the harness passes them through unchecked here (``check_from='convdet'``) and a
point costs seconds.  ``WIDTHS`` has one case per point and ConvDet-side plan row: from the inference plan ConvDet's forward and
``convdet_pack`` (``detect`` is covered elsewhere: ``ALLOWED`` of the coverage test); from the training plan every row from ConvDet's
forward through its data gradient.  The coverage test keeps ``WIDTHS`` equal to the planners and checks that every ConvDet signature the
planners produce over 1..20 anchors x 1..256 classes occurs at a point.

A padded ConvDet is held to the module's own parameters, zero-extended in the harness: a stand-in that did not follow them fails.  Its
weight gradient is held, after ``wgrad_reduce_rows``, to float64 on the true ``dpred[..., :N]``.

Attained: every ConvDet-side launch of the twelve points holds both bars (the figures: profiles/fp64_widths.log).  The first run had
one miss, which changed the kernel: ``loss_bwd`` at 16 anchors x 3 classes (A = 384) held bar L at 1.66e-8 M and missed bar P in the
delta block (P block 2.14 of 2, P tensor 4.43 of 4, no branch flip).  One positive anchor carried it, a 34x30 anchor whose decoded box
is clamped on two sides: its delta gradients were 1.0e-7 .. 5.1e-7 relative (8 ulp) from float64 where the float32 oracle chain lands
within 1 ulp.  A float32 restatement of the kernel's own formula on the host gives the kernel's figures (4.8e-7, 2.2e-7, 1.4e-7,
0.7e-7), and moves to -2.9e-7 .. +9.3e-7 when the decoded width or height changes by one ulp: the IoU gradient cancels about 3:1 between
its intersection and area paths, so every float32 evaluation lands a few ulp to either side, and with 3 to 8 positives per image one
anchor decides the block's rms.  csrc/loss.hip ``anchor_geom_grad`` now takes the rows with a box (about 0.1 % of a batch) through the
decode, the IoU and its gradient in float64 and rounds once; the other rows run the float32 chain as before.

``test_convdet_pad_entries``: the three entry points of csrc/convdet_pad.hip away from the model, into NaN-filled buffers.
"""
import gc

import pytest
import torch

import fp64_ref as R
import test_fp64_launches_gpu as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    """The models, plans and operand copies of the twelve points are finalised here, with the device idle, not by a garbage
    collection in the middle of a later module's stream capture."""
    yield
    gc.collect()
    torch.cuda.synchronize()

BATCH, SIZE = 3, (70, 100)
POINTS = [  # arch, anchors_per_grid, num_classes, sparse_gt
    ('squeezedet', 9, 7, False), ('squeezedet', 9, 255, True), ('squeezedet', 20, 7, False),
    ('squeezedet', 4, 6, False), ('squeezedet', 3, 7, False), ('squeezedet', 4, 3, False),
    ('squeezedet', 1, 3, False), ('squeezedet', 16, 3, False), ('squeezedet', 9, 1, False),
    ('squeezedet', 9, 20, False), ('squeezedet', 9, 256, True), ('squeezedetplus', 9, 20, True),
]
# the training step's ground-truth seed per point (1 = the benchmark's; another one only where the float32 oracle chain alone exceeds
# the branch-flip cap on the point's operands)
GT_SEED = {}
# the points whose first launch of a family also runs the degraded emulations, and the teeth taken from them: the 9-tap direct weight
# gradient (the benchmark's conv_wgrad teeth come from a 1-tap launch), the first sparse and the first many-class loss launches
TEETH_POINTS = {
    ('squeezedet', 9, 7, False): ['conv_wgrad'],
    ('squeezedet', 9, 255, True): ['loss_sparse_fwd', 'loss_sparse_bwd'],
    ('squeezedet', 9, 20, False): ['loss_fwd_many', 'loss_bwd_many'],
}
TEETH = [(pt, fam, emu) for pt, fams in TEETH_POINTS.items() for fam in fams for emu in (('bf16', 'split3') if fam == 'conv_wgrad' else ('bf16',))]


def convdet_side(rows, arch, anchors_per_grid, num_classes, train):
    """The ConvDet side of a launch plan of a point: from ConvDet's forward row to the end (inference) or through ConvDet's data-gradient
    row (training).  -> (first index, one past the last index)."""
    from squeezedet_pytorch_amd import ops
    from squeezedet_pytorch_amd.synthetic import convdet_in_channels
    ccd, nrun = convdet_in_channels(arch), ops.convdet_width(anchors_per_grid, num_classes)[1]
    tags = [t for _k, t in rows]
    i0 = tags.index(f'9tap C{ccd} N{nrun} 4x6')
    return (i0, tags.index(f'9tap C{nrun} N{ccd} 4x6', i0 + 1) + 1) if train else (i0, len(rows))


# one (kernel, tag) per distinct ConvDet-side launch of the two plans of each point, in plan order; WIDTHS below: point + (kernel, tag)
_WIDTHS = {
    ('squeezedet', 9, 7, False): [
        ('conv_dma<9,16,1,1,4>', '9tap C768 N108 4x6'), ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'),
        ('conv_wgrad<9>', 'wgrad 9tap C768 N108 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C108 N768 4x6'),
    ],
    ('squeezedet', 9, 255, True): [
        ('conv_dma<9,16,1,4,4>', '9tap C768 N2340 4x6'), ('loss_sparse_fwd', 'loss A216'), ('loss_sparse_bwd', 'lossbwd A216'),
        ('conv_wgrad<9>', 'wgrad 9tap C768 N2340 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C2340 N768 4x6'),
    ],
    ('squeezedet', 20, 7, False): [
        ('conv_dma<9,16,1,3,4>', '9tap C768 N240 4x6'), ('loss_fwd', 'loss A480'), ('loss_bwd', 'lossbwd A480'),
        ('conv_wgrad<9>', 'wgrad 9tap C768 N240 4x6'), ('conv_wino_sk', '9tap C240 N768 4x6'),
    ],
    ('squeezedet', 4, 6, False): [
        ('conv_dma<9,16,1,3,4>', '9tap C768 N44 4x6'), ('loss_fwd', 'loss A96'), ('loss_bwd', 'lossbwd A96'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N44 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C44 N768 4x6'),
    ],
    ('squeezedet', 3, 7, False): [
        ('conv_dma<9,16,1,3,4>', '9tap C768 N36 4x6'), ('loss_fwd', 'loss A72'), ('loss_bwd', 'lossbwd A72'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N36 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C36 N768 4x6'),
    ],
    ('squeezedet', 4, 3, False): [
        ('conv_dma<9,16,1,2,4>', '9tap C768 N32 4x6'), ('loss_fwd', 'loss A96'), ('loss_bwd', 'lossbwd A96'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N32 4x6'), ('conv_wino_sk', '9tap C32 N768 4x6'),
    ],
    ('squeezedet', 1, 3, False): [
        ('conv_dma<9,16,1,1,4>', '9tap C768 N8 4x6'), ('loss_fwd', 'loss A24'), ('loss_bwd', 'lossbwd A24'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N8 4x6'), ('conv_wino_sk', '9tap C8 N768 4x6'),
    ],
    ('squeezedet', 16, 3, False): [
        ('conv_dma<9,16,1,4,4>', '9tap C768 N128 4x6'), ('loss_fwd', 'loss A384'), ('loss_bwd', 'lossbwd A384'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N128 4x6'), ('conv_wino_sk', '9tap C128 N768 4x6'),
    ],
    ('squeezedet', 9, 1, False): [
        ('conv_dma<9,16,1,4,4>', '9tap C768 N64 4x6'), ('convdet_pack', 'pack N54 <- 64 4x6'), ('loss_fwd', 'loss A216'),
        ('loss_bwd', 'lossbwd A216'), ('convdet_unpack', 'unpack N54 -> 64 4x6'), ('conv_wgrad_wino', 'wgrad 9tap C768 N64 4x6'),
        ('wgrad_reduce_rows', 'N54 of 64 C768'), ('conv_wino_sk', '9tap C64 N768 4x6'),
    ],
    ('squeezedet', 9, 20, False): [
        ('conv_dma<9,16,1,4,4>', '9tap C768 N256 4x6'), ('convdet_pack', 'pack N225 <- 256 4x6'), ('loss_fwd', 'loss A216'),
        ('loss_bwd', 'lossbwd A216'), ('convdet_unpack', 'unpack N225 -> 256 4x6'), ('conv_wgrad_wino', 'wgrad 9tap C768 N256 4x6'),
        ('wgrad_reduce_rows', 'N225 of 256 C768'), ('conv_wino_sk', '9tap C256 N768 4x6'),
    ],
    ('squeezedet', 9, 256, True): [
        ('conv_dma<9,16,1,4,4>', '9tap C768 N2368 4x6'), ('convdet_pack', 'pack N2349 <- 2368 4x6'), ('loss_sparse_fwd', 'loss A216'),
        ('loss_sparse_bwd', 'lossbwd A216'), ('convdet_unpack', 'unpack N2349 -> 2368 4x6'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N2368 4x6'), ('wgrad_reduce_rows', 'N2349 of 2368 C768'),
        ('conv_wino_sk', '9tap C2368 N768 4x6'),
    ],
    ('squeezedetplus', 9, 20, True): [
        ('conv_dma<9,16,1,4,4>', '9tap C512 N256 4x6'), ('convdet_pack', 'pack N225 <- 256 4x6'), ('loss_sparse_fwd', 'loss A216'),
        ('loss_sparse_bwd', 'lossbwd A216'), ('convdet_unpack', 'unpack N225 -> 256 4x6'),
        ('conv_wgrad_wino', 'wgrad 9tap C512 N256 4x6'), ('wgrad_reduce_rows', 'N225 of 256 C512'),
        ('conv_wino_sk', '9tap C256 N512 4x6'),
    ],
}
WIDTHS = [pt + e for pt, lst in _WIDTHS.items() for e in lst]


def _results(point):
    arch, apg, C, sparse = point
    return L._step_results(arch, BATCH, SIZE, gt_seed=GT_SEED.get(point, 1), teeth_for=TEETH_POINTS.get(point, []), num_classes=C,
                           anchors_seed=None if apg == 9 else L.anchors_seed(apg), sparse_gt=sparse, check_from='convdet')


def _case_id(c):
    return f'{c[0]}-a{c[1]}-c{c[2]}-{"sparse" if c[3] else "dense"}-{c[4]}-{c[5]}'


def _summary(case, outs):
    """One line per case: the outputs the launch wrote and the largest attained ratios over them (``test_fp64_offbench_gpu._summary``)."""
    head = f'{case[0]} a{case[1]} c{case[2]} {"sparse" if case[3] else "dense"} {case[4]} | {case[5]} | {len(outs)} out'
    num = [(n, b) for n, b in outs if 'exact' not in b]
    tail = ''.join(f'  {n} ' + (f'branch flips {b["flips"]} (at most 4)' if 'flips' in b else f'exact={b["exact"]}')
                   for n, b in outs if 'exact' in b)
    if not num:
        return head + tail
    worst = max(num, key=lambda nb: nb[1]['p_block'])
    k = worst[1]['k']
    tap = max((b['l_ratio_tap'] for _n, b in num if 'l_ratio_tap' in b), default=None)
    return (head + f'  max err/M {max(b["l_ratio"] for _n, b in num):.2e}' + (f' (per-tap M: {tap:.2e})' if tap is not None else '')
            + f'  P block {worst[1]["p_block"]:.2f} ({worst[0]})  P tensor {max(b["p_tensor"] for _n, b in num):.2f}  (k {k}, 2k {2 * k})' + tail)


@pytest.mark.parametrize('case', WIDTHS, ids=[_case_id(c) for c in WIDTHS])
def test_width_launch_against_fp64(case):
    """The planned (kernel, tag) ran in the point's step (the launches equal the plan: ``L._run_both``), and every output it wrote holds
    bars L and P, or is bit-exact; at most 4 branch-flip anchors per loss launch."""
    rows, _ = _results(case[:4])
    entry = (case[0], BATCH, case[4], case[5])
    assert entry in rows, f'{case} did not run in the step (fallback or plan drift)'
    outs = rows[entry]
    assert outs, case
    print(_summary(case, outs))
    bad = [(name, b) for name, b in outs if not (b['l_ok'] and b['p_ok'])]
    assert not bad, bad


@pytest.mark.parametrize('point,fam,emu', TEETH, ids=[f'a{p[1]}-c{p[2]}-{f}-{e}' for p, f, e in TEETH])
def test_teeth_bar_p_rejects_degraded_emulations_widths(point, fam, emu):
    """Bar P tells the fp32 kernels of this axis from reduced-precision ones: the 9-tap ``conv_wgrad<9>`` launch of (9, 7) recomputed
    with bf16-rounded operands and with the 3-product bf16 split inside the same slab structure, and the first sparse and the first
    many-class loss launch on bf16-rounded pred and gt, fail it."""
    rows, teeth = _results(point)
    t = teeth.get(fam)
    assert t is not None, f'no launch of family {fam} at {point}'
    if fam == 'conv_wgrad':         # the only launch of the family at this point is the 9-tap one: the teeth are its own
        assert [e[2] for e in rows if L.family(e[2]) == 'conv_wgrad'] == ['conv_wgrad<9>']
    b = t[emu]
    print(f'teeth {fam:24s} {emu:7s} P block {b["p_block"]:9.2f}  P tensor {b["p_tensor"]:9.2f}  (k {b["k"]})')
    assert not b['p_ok'], (fam, emu, b)


# ---- the three entry points of csrc/convdet_pad.hip away from the model ----

PAD_SHAPES = [(1, 1, 64), (72, 54, 64), (5, 2349, 2368), (257, 225, 256), (72, 64, 64)]      # (rows, N, Npad); the last: N == Npad
REDUCE_C = 12
GUARD = 7               # NaN elements in front of and behind every output view


def _in_nan_buffer(shape):
    """A contiguous view of ``shape`` inside a larger NaN-filled buffer -> (view, buffer, offset)."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), float('nan'), device='cuda')
    return buf[GUARD:GUARD + n].view(shape), buf, n


def _guards_intact(buf, n):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all())


def test_convdet_pad_entries():
    """``convdet_pack`` / ``convdet_unpack`` bit-exact (zero past N) and ``wgrad_reduce_rows`` against the float64 sum of the slabs (bar
    L: 2^-18 of the sum of magnitudes; S = 1 exact), with outputs that are views inside NaN buffers whose other elements stay NaN; malformed
    arguments give the wrappers' ValueError."""
    from squeezedet_pytorch_amd import ops
    g = torch.Generator().manual_seed(77)
    for rows, N, Npad in PAD_SHAPES:
        y_pad = torch.randn(1, rows, 1, Npad, generator=g).cuda()
        out, buf, n = _in_nan_buffer((1, rows, 1, N))
        res = ops.convdet_pack(y_pad, N, out=out)
        torch.cuda.synchronize()
        assert res is out and torch.equal(out, y_pad[..., :N]) and _guards_intact(buf, n), (rows, N, Npad)
        assert torch.equal(ops.convdet_pack(y_pad, N), y_pad[..., :N])
        dy = torch.randn(1, rows, 1, N, generator=g).cuda()
        up = ops.convdet_unpack(dy, Npad)
        assert tuple(up.shape) == (1, rows, 1, Npad) and torch.equal(up[..., :N], dy), (rows, N, Npad)
        assert bool((up[..., N:] == 0).all()) and not bool(torch.signbit(up[..., N:]).any())
        for S in (1, 3):
            for taps in (1, 9):
                k = 3 if taps == 9 else 1
                C = REDUCE_C
                stride = Npad * taps * C + Npad
                slab = torch.randn(S * stride, generator=g).cuda()
                dw, bw, nw = _in_nan_buffer((N, C, k, k))
                db, bb, nb = _in_nan_buffer((N,))
                ops.wgrad_reduce_rows(slab, S, N, Npad, C, taps, dw, db)
                torch.cuda.synchronize()
                s64 = slab.double().view(S, stride)
                w64 = s64[:, :Npad * taps * C].view(S, Npad, taps, C)[:, :N]
                b64 = s64[:, Npad * taps * C:][:, :N]
                ref_w = w64.sum(0).permute(0, 2, 1).reshape(N, C, k, k)
                M_w = w64.abs().sum(0).permute(0, 2, 1).reshape(N, C, k, k)
                what = (rows, N, Npad, S, taps)
                assert _guards_intact(bw, nw) and _guards_intact(bb, nb), what
                assert not bool(torch.isnan(dw).any()) and not bool(torch.isnan(db).any()), what
                lim = 0.0 if S == 1 else R.BAR_L
                assert bool(((dw.double() - ref_w).abs() <= lim * M_w).all()), what
                assert bool(((db.double() - b64.sum(0)).abs() <= lim * b64.abs().sum(0)).all()), what
    # malformed arguments: the wrappers refuse before the library is touched
    y = torch.zeros(1, 4, 1, 64, device='cuda')
    for bad in (lambda: ops.convdet_pack(y, 0), lambda: ops.convdet_pack(y, 65), lambda: ops.convdet_pack(y[..., :32], 8),
                lambda: ops.convdet_pack(y, 8, out=torch.empty(1, 4, 1, 9, device='cuda')),
                lambda: ops.convdet_pack(y, 8, out=torch.empty(1, 4, 1, 16, device='cuda')[..., :8]),
                lambda: ops.convdet_unpack(y, 63), lambda: ops.convdet_unpack(y[0], 64)):
        with pytest.raises(ValueError):
            bad()
    slab = torch.zeros(2 * (64 * 9 * 4 + 64), device='cuda')
    dw, db = torch.empty(54, 4, 3, 3, device='cuda'), torch.empty(54, device='cuda')
    for bad in (lambda: ops.wgrad_reduce_rows(slab, 3, 54, 64, 4, 9, dw, db),                  # S does not match the workspace
                lambda: ops.wgrad_reduce_rows(slab, 2, 54, 64, 4, 1, dw, db),                  # taps does not match
                lambda: ops.wgrad_reduce_rows(slab.double(), 2, 54, 64, 4, 9, dw, db),
                lambda: ops.wgrad_reduce_rows(slab, 2, 54, 64, 4, 9, dw.permute(0, 1, 3, 2), db),
                lambda: ops.wgrad_reduce_rows(slab, 2, 54, 64, 4, 9, dw, db[:53]),
                lambda: ops.wgrad_reduce_rows(slab[:2 * (48 * 9 * 4 + 48)], 2, 54, 48, 4, 9, dw, db)):   # N > Npad
        with pytest.raises(ValueError):
            bad()
