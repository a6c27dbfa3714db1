"""GPU tier: the training step with a LIVE dropout in front of ConvDet, held to float64 from the last Fire's expand launches through
ConvDet's data gradient.  Every other float64 sweep runs the step at p = 0 (an all-keep mask); this one keeps the rate (p = 0.5, the
default of every real training run, and p = 0.2: scale 1.25, keep16 52429) through the harness of tests/test_fp64_launches_gpu.py
(``_run_step(dropout_prob=p, check_from='dropout')``).

Points: batch 3 at 70x100 (final grid 4x6: 72 pixels x 768 / 512 channels), in the three forms the dropout can take:
* ``fused``: the mask is evaluated in the epilogues of the last Fire's expand1x1 (weight-stationary 1x1) and expand3x3 (balanced
  Winograd), no mask tensor; ConvDet's data gradient masks by its own input and scales by 1 / (1 - p);
* ``standalone``: ``base.fused_dropout = False`` -- the ``dropout_mask`` launch draws the mask tensor (bit-exact against the host
  restatement: tests/test_dropout_gpu.py), the expand launches and the data gradient multiply it in (``ymul``);
* ``injected``: ``base._forced_drop_mask`` set to that same mask; the stream is not consumed.

Per form: the launches equal ``plan.training_launch_plan(..., dropout=True, fused_dropout=...)`` (the injected form: the stand-alone
plan without its ``dropout_mask`` row); every output of the checked launches -- the two expand launches (reference times the step's mask,
read through the stand-alone kernel before the launch), ConvDet's forward, the loss launches, ConvDet's weight gradient after the slab
reduction (against ``fp64_ref.wgrad`` on the dropped input) and its data gradient -- holds bars L and P with its family's k; the step
counter advanced exactly once (not at all with an injected mask).  The backbone's other launches are those of the off-benchmark
sweep's 70x100 points (tests/test_fp64_coverage.py) and pass through unchecked.

ConvDet's data gradient gets a second reference beside the per-launch one, because the per-launch one takes the launch's own ReLU mask
(the dropped tensor) on trust: ``fp64_ref.dropped_dgrad`` -- the plain float64 gradient of the true dpred, times the stand-alone
kernel's mask, times (pre-dropout expand output > 0) recomputed in float64 from the last Fire's squeeze output and the module's
parameters.  Bar L with M / (1 - p); elements whose float64 pre-activation is within 2^-18 M of zero (where a correct fp32 forward may
land on either side of the ReLU) are excluded, at most 0.5 % of the tensor.  A gradient masked by the mask alone fails it
(tests/test_dropout_host.py).

The figures of a run: profiles/dropout_fp64_tests.log.
"""
import gc

import pytest
import torch

import fp64_ref as R
import test_fp64_launches_gpu as L

pytestmark = pytest.mark.gpu

BATCH, SIZE = 3, (70, 100)
POINTS = [('squeezedet', 0.5), ('squeezedetplus', 0.5), ('squeezedet', 0.2)]        # arch, p
FORMS = L.DROP_FORMS
GT_SEED = {}            # per (arch, p): the ground-truth seed where 1 (the benchmark's) exceeds a cap on the point's operands

# the checked launches of a point, in plan order, per form ('injected' runs the stand-alone form's launches)
_SIDE = {
    ('squeezedet', True): [
        ('conv_ws<6,8>', '1tap C96 N384 4x6'), ('conv_wino_sk', '9tap C96 N384 4x6'), ('conv_dma<9,16,1,1,4>', '9tap C768 N72 4x6'),
        ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'), ('conv_wgrad_wino', 'wgrad 9tap C768 N72 4x6'),
        ('conv_wino_sk', '9tap C72 N768 4x6'),
    ],
    ('squeezedet', False): [
        ('conv_dma<1,32,1,6,4>', '1tap C96 N384 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C96 N384 4x6'),
        ('conv_dma<9,16,1,1,4>', '9tap C768 N72 4x6'), ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'),
        ('conv_wgrad_wino', 'wgrad 9tap C768 N72 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C72 N768 4x6'),
    ],
    ('squeezedetplus', True): [
        ('conv_ws<4,8>', '1tap C384 N256 4x6'), ('conv_wino_sk', '9tap C384 N256 4x6'), ('conv_dma<9,16,1,1,4>', '9tap C512 N72 4x6'),
        ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'), ('conv_wgrad_wino', 'wgrad 9tap C512 N72 4x6'),
        ('conv_wino_sk', '9tap C72 N512 4x6'),
    ],
    ('squeezedetplus', False): [
        ('conv_dma<1,32,1,4,4>', '1tap C384 N256 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C384 N256 4x6'),
        ('conv_dma<9,16,1,1,4>', '9tap C512 N72 4x6'), ('loss_fwd', 'loss A216'), ('loss_bwd', 'lossbwd A216'),
        ('conv_wgrad_wino', 'wgrad 9tap C512 N72 4x6'), ('conv_dma<9,16,1,4,4>', '9tap C72 N512 4x6'),
    ],
}
# arch, p, form, kernel, tag
CASES = [(arch, p, form) + e for arch, p in POINTS for form in FORMS for e in _SIDE[(arch, form == 'fused')]]


def dropout_side(rows, arch):
    """Where a training plan's checked rows lie: from the last Fire's expand1x1 (two rows in front of ConvDet's forward) through
    ConvDet's data gradient.  -> (first index, one past the last index)."""
    from squeezedet_pytorch_amd.synthetic import convdet_in_channels
    ccd = convdet_in_channels(arch)
    tags = [t for _k, t in rows]
    i0 = tags.index(f'9tap C{ccd} N72 4x6')
    return i0 - 2, tags.index(f'9tap C72 N{ccd} 4x6', i0 + 1) + 1


def planned(arch, form):
    """The launches of the point's step in ``form``."""
    from squeezedet_pytorch_amd import plan
    rows = plan.training_launch_plan(arch, BATCH, SIZE, dropout=True, fused_dropout=form == 'fused')
    return [r for r in rows if not (form == 'injected' and r[0] == 'dropout_mask')]


@pytest.fixture(scope='module', autouse=True)
def _leave_nothing_behind():
    yield
    _STATE.clear()
    gc.collect()
    torch.cuda.synchronize()


_STATE = {}


def _results(arch, p, form):
    """(rows, launches, (rng before, rng after)) of the point's checked training step (run once per process; a failure is kept and
    raised again for every case of the point)."""
    key = (arch, p, form)
    if key not in _STATE:
        try:
            h, got = L._run_step(arch, BATCH, 'train', SIZE, GT_SEED.get((arch, p), 1), [], check_from='dropout', dropout_prob=p,
                                 drop_form=form)
            _STATE[key] = (h.rows, got, h.drop_rng)
            del h
            torch.cuda.empty_cache()
        except Exception as exc:            # noqa: BLE001 -- re-raised below
            _STATE[key] = exc
    res = _STATE[key]
    if isinstance(res, Exception):
        raise res
    return res


def _fmt(case, name, b):
    head = f'{case[0]:14s} p{case[1]} {case[2]:10s} {case[3]:22s} {case[4]:30s} {name:20s}'
    if b.get('end_to_end'):
        return head + f' max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e})  excluded {b["excluded"]} (cap ok: {b["cap_ok"]})'
    if 'flips' in b:
        return head + f' branch flips {b["flips"]} (at most 4)'
    if 'exact' in b:
        return head + f' bit-exact={b["exact"]}'
    return head + (f' max err/M {b["l_ratio"]:.2e} (bar {R.BAR_L:.2e})  P block {b["p_block"]:5.2f} (k {b["k"]})  '
                   f'P tensor {b["p_tensor"]:5.2f} (2k {2 * b["k"]})')


@pytest.mark.parametrize('arch,p,form', [(a, p, f) for a, p in POINTS for f in FORMS], ids=lambda v: str(v))
def test_launches_equal_the_plan_and_the_step_advances_once(arch, p, form):
    _rows, got, (before, after) = _results(arch, p, form)
    want = planned(arch, form)
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:4] + [len(got), len(want)]
    assert ('dropout_mask' in [k for k, _t in got]) == (form == 'standalone')
    assert before is not None and after is not None
    print(f'{arch} p{p} {form}: dropout stream {before} -> {after}')
    assert after == (before[0], before[1] + (0 if form == 'injected' else 1))


@pytest.mark.parametrize('case', CASES, ids=[f'{a}-p{p}-{f}-{k}-{t}' for a, p, f, k, t in CASES])
def test_dropout_launch_against_fp64(case):
    """The planned (kernel, tag) ran in the step with a live dropout, and every output it wrote holds bars L and P."""
    arch, p, form, kernel, tag = case
    rows, _got, _rng = _results(arch, p, form)
    entry = (arch, BATCH, kernel, tag)
    assert entry in rows and rows[entry], f'{case} did not run checked in the step (fallback or plan drift)'
    names = [n for n, _b in rows[entry]]
    if kernel == 'conv_wgrad_wino':                         # ConvDet's dW / db, after the slab reduction, on the dropped input
        assert any(n.startswith('dW ') for n in names) and any(n.startswith('db ') for n in names), names
    if tag.startswith('9tap C72 '):                         # ConvDet's data gradient: the per-launch and the end-to-end reference
        assert names == ['y', 'dA end to end'], names
    bad = []
    for name, b in rows[entry]:
        print(_fmt(case, name, b))
        if not (b['l_ok'] and b['p_ok']):
            bad.append((name, b))
    assert not bad, bad
