"""GT encoding away from the KITTI grid, CPU tier.

1. tests/golden/gt_encode_grids.npz (the reference's ``compute_deltas`` on six other grids, tests/golden/make_golden_gt_grids.py)
   against ``oracle.compute_deltas`` with both tie rules and ``boxes.compute_deltas``, by the rules of tests/test_gt_encode.py:
   indices and deltas bit-equal on the determined prefix and on the whole fully determined set, a valid assignment everywhere,
   deltas bit-equal wherever the same anchor was picked.
2. tests/gt_encode_ref.py, the restatement the device sweep (tests/test_gt_encode_sweep_gpu.py) is held to, equals
   ``oracle.compute_deltas(ties='lowest')`` bit for bit on every sweep geometry and on both fixture files, and every one of its
   mutants moves an index, or a delta by more than 1 ulp, on some sweep case.
"""
import os

import numpy as np
import pytest

import gt_encode_ref as R
import oracle
import squeezedet_pytorch_amd as sqd
from squeezedet_pytorch_amd import boxes as host_boxes
from test_gt_encode import _check_valid_assignment, _overlaps, _prefix


@pytest.fixture(scope="module")
def grids(golden_dir):
    g = np.load(os.path.join(golden_dir, "gt_encode_grids.npz"))
    kinds = [str(k) for k in g["kinds"]]
    out = []
    for n, name in enumerate(g["grids"]):
        k = f"g{n}_"
        cfg = sqd.make_cfg(arch=str(g[k + "arch"]), input_size=tuple(int(v) for v in g[k + "input_size"]), anchors_seed=g[k + "seed"],
                           device="cpu")
        assert cfg.anchors.shape[0] == int(g[k + "num_anchors"][0])
        sets = [(kinds[s], g[k + f"boxes{s}"], g[k + f"cls{s}"], g[k + f"idx{s}"], g[k + f"deltas{s}"], g[k + f"unique{s}"])
                for s in range(len(kinds))]
        out.append((str(name), cfg.anchors, sets))
    return out


def test_fixture_grids_are_the_sweep_grids(grids):
    assert [n for n, _, _ in grids] == list(R.GRIDS)
    assert [a.shape[0] for _, a, _ in grids] == [216, 135, 32400, 4212, 60, 700]
    for name, anchors, _ in grids:
        assert np.array_equal(anchors, R.grid_anchors(name)), name            # make_cfg's anchors, as the product builds them


def test_fixture_conditions(grids):
    """what the generator asserted about its inputs, read back from the file"""
    for name, anchors, sets in grids:
        det = [s for s in sets if s[0] == "determined"]
        assert len(det) == 1 and det[0][1].shape[0] >= 12 and det[0][5].all(), name
        assert len(set(det[0][3].tolist())) == det[0][1].shape[0]
        far = [s for s in sets if s[0] == "far"][0]
        assert all(not _overlaps(anchors, b).max() > 0 for b in far[1]), name          # the zero-overlap fallback
        assert any(not s[5].all() for s in sets), f"{name}: no exact tie"


@pytest.mark.parametrize("ties", ["argsort", "lowest"])
def test_oracle_vs_reference_grids(grids, ties):
    for name, anchors, sets in grids:
        for s, (kind, bx, cls, idx_ref, deltas_ref, unique) in enumerate(sets):
            deltas, idx = oracle.compute_deltas(bx, anchors, ties=ties)
            p = _prefix(unique)
            assert p == bx.shape[0] or kind != "determined"
            assert np.array_equal(idx[:p], idx_ref[:p]), f"{name} set {s}"
            assert np.array_equal(deltas[:p], deltas_ref[:p]), f"{name} set {s}"
            _check_valid_assignment(anchors, bx, idx)
            same = idx == idx_ref
            assert np.array_equal(deltas[same], deltas_ref[same]), f"{name} set {s}"


def test_host_compute_deltas_vs_reference_grids(grids):
    for name, anchors, sets in grids:
        for s, (kind, bx, cls, idx_ref, deltas_ref, unique) in enumerate(sets):
            deltas, idx = host_boxes.compute_deltas(bx, anchors)
            p = _prefix(unique)
            assert np.array_equal(idx[:p], idx_ref[:p]) and np.array_equal(deltas[:p], deltas_ref[:p]), f"{name} set {s}"
            _check_valid_assignment(anchors, bx, idx)
            same = idx == idx_ref
            assert np.array_equal(deltas[same], deltas_ref[same]), f"{name} set {s}"


# ------------------------------------------------------------------------------------------- the restatement and its teeth
def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


_GEOMS = {c["geom"]: c for c in R.geometries()}
_REF = {}


def _ref(geom, mutant=None):
    """(deltas, idx) of every image of a geometry (computed once per (geometry, mutant))"""
    key = (geom, mutant)
    if key not in _REF:
        c = _GEOMS[geom]
        _REF[key] = [R.compute_deltas(bx, c["anchors"], mutant) for bx in c["boxes"]]
    return _REF[key]


@pytest.mark.parametrize("geom", list(_GEOMS))
def test_restatement_equals_oracle_on_the_sweep(geom):
    c = _GEOMS[geom]
    for (d, i), bx in zip(_ref(geom), c["boxes"]):
        d_or, i_or = oracle.compute_deltas(bx, c["anchors"], ties="lowest")
        assert _bits_equal(i, i_or) and _bits_equal(d, d_or), c["name"]


def test_restatement_equals_oracle_on_the_fixtures(grids, golden_dir):
    for name, anchors, sets in grids:
        for s, (kind, bx, cls, idx_ref, deltas_ref, unique) in enumerate(sets):
            d, i = R.compute_deltas(bx, anchors)
            d_or, i_or = oracle.compute_deltas(bx, anchors, ties="lowest")
            assert _bits_equal(i, i_or) and _bits_equal(d, d_or), f"{name} set {s}"
            if kind == "determined":                                           # and there the reference itself, bit for bit
                assert _bits_equal(i, idx_ref) and _bits_equal(d, deltas_ref), name
    kitti = np.load(os.path.join(golden_dir, "gt_encode.npz"))
    anchors = sqd.make_cfg(arch="squeezedet", device="cpu").anchors
    for s in range(int(kitti["num_sets"][0])):
        d, i = R.compute_deltas(kitti[f"boxes{s}"], anchors)
        d_or, i_or = oracle.compute_deltas(kitti[f"boxes{s}"], anchors, ties="lowest")
        assert _bits_equal(i, i_or) and _bits_equal(d, d_or), f"KITTI set {s}"


def test_restatement_dense_rows():
    """the dense form: one row per assigned box, a class id outside 0 .. C-1 leaves the one-hot part zero, an unassigned box no row"""
    c = [c for c in R.sweep_cases() if c["name"] == "overfull-A33"][0]
    bx, A = c["boxes"][0], 33
    cls = np.arange(bx.shape[0]) % 7 - 1                                       # -1 .. 5 with C = 5: -1 and 5 are outside
    gt, d, i = R.encode_gt(cls, bx, c["anchors"], 5)
    assert gt.shape == (A, 14) and int(gt[:, 0].sum()) == A and np.all(i[A:] == A) and sorted(i[:A].tolist()) == list(range(A))
    for k in range(A):
        assert np.array_equal(gt[i[k], 1:5], bx[k]) and np.array_equal(gt[i[k], 5:9], d[k])
        assert gt[i[k], 9:].sum() == (1. if 0 <= cls[k] < 5 else 0.)


def _moved(ref, mut):
    (d, i), (dm, im) = ref, mut
    ulps = np.abs(d.view(np.int32).astype(np.int64) - dm.view(np.int32).astype(np.int64))
    return (not np.array_equal(i, im)) or bool(np.any(ulps > 1))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_caught_by_the_sweep(mutant):
    caught = [g for g, c in _GEOMS.items() if c["group"] != "big"              # (the large clouds add nothing a small one lacks)
              and any(_moved(r, m) for r, m in zip(_ref(g), _ref(g, mutant)))]
    print(mutant, len(caught), caught[:6])
    assert caught, f"{mutant}: no sweep case tells it from the rule"


def test_sweep_reaches_the_listed_paths():
    """the host-side path counts the device sweep prints: each listed path is taken by some case"""
    pc = {c["name"]: R.path_counts(c) for c in R.geometries() if c["group"] in ("unaligned", "past256", "big")}
    assert pc["unaligned-A135-C4"]["unaligned_images"] == 3
    free, late, groups = pc["past256-free"], pc["past256-late-conflicts"], pc["past256-groups"]
    assert free["past_256"] >= 40 and free["conflicts"] == 0 and free["past_256_free"] == free["past_256"]
    assert late["conflicts"] > 0 and late["past_256_free"] > 0 and late["conflicts"] + late["past_256_free"] == late["past_256"]
    assert groups["conflicts"] > 256 and groups["past_256_free"] == 0
    big = [pc[f"big-A{A}"] for A in R.BIG_A]
    assert all(b["lds_attribute"] and b["conflicts"] >= 1 for b in big)
    assert big[0]["lds_dynamic"] == 48 * 1024 + 4 and big[1]["lds_dynamic"] == 128 * 1024 and big[1]["lds_total"] < 160 * 1024
