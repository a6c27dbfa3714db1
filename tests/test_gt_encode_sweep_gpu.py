"""The GT encoder (csrc/gt_encode.hip) on the MI355X against tests/gt_encode_ref.py, the numpy restatement of its rule that the CPU
tier (tests/test_gt_encode_grids.py) pins to the oracle and, through it, to the reference: other grids than KITTI's, 1 .. 256
classes, dense and sparse outputs, images of the dense tensor off 16-byte alignment, bitmap word edges, anchor counts below and
next to the 1024-thread stride, more than 256 boxes per image with free and with conflicting first choices, more boxes than
anchors, class ids outside 0 .. C-1, the dynamic-LDS branch up to the documented limit A = 2^20, stale output buffers, and the
product's own callers.

Bars (the project's existing ones for this kernel): anchor_idx exact; dx, dy bit-exact (a float64 divide rounded to float32); dw,
dh within 1 ulp (the device log against numpy's); dense gt bit-exact except columns 7:9 at 1 ulp; ``parallel=True`` and
``parallel=False`` bit-equal to each other.  Every test prints the path counts of its case (gt_encode_ref.path_counts), derived
from the inputs on the host."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gt_encode_ref as R
import squeezedet_pytorch_amd as sqd

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in R.sweep_cases()}
_ASSIGNED, _COUNTS = {}, {}


def _assigned(case):
    """[(deltas, idx)] per image by the restatement, once per geometry"""
    g = case["geom"]
    if g not in _ASSIGNED:
        _ASSIGNED[g] = [R.compute_deltas(bx, case["anchors"]) for bx in case["boxes"]]
    return _ASSIGNED[g]


def _counts(case, **kw):
    key = (case["geom"], case["C"], case["dense"], tuple(sorted(kw.items())))
    if key not in _COUNTS:
        _COUNTS[key] = R.path_counts(dict(case, **kw))
    print(f'{case["name"]}: A={case["anchors"].shape[0]} C={case["C"]} boxes={[b.shape[0] for b in case["boxes"]]} {_COUNTS[key]}')
    return _COUNTS[key]


def _reference(case):
    """(gt [B,A,C+9] or None, idx [total], deltas [total,4], assigned mask [total])"""
    A = case["anchors"].shape[0]
    per = _assigned(case)
    gt = None
    if case["dense"]:
        gt = np.stack([R.encode_gt(c, b, case["anchors"], case["C"], assigned=a)[0] for c, b, a in zip(case["cls"], case["boxes"], per)])
    idx = np.concatenate([i for _, i in per])
    deltas = np.concatenate([d for d, _ in per], 0)
    return gt, idx, deltas, (idx >= 0) & (idx < A)


def _pack(case):
    offs = np.zeros(len(case["boxes"]) + 1, np.int32)
    offs[1:] = np.cumsum([b.shape[0] for b in case["boxes"]])
    boxes = np.concatenate(case["boxes"], 0).astype(np.float32)
    cls = np.concatenate(case["cls"]).astype(np.int32)
    return [torch.from_numpy(v).cuda() for v in (boxes, cls, offs)] + [torch.from_numpy(case["anchors"]).cuda()]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _ulps(a, b):
    d = np.abs(_bits(a) - _bits(b))
    return int(d.max()) if d.size else 0


def _check(case, ref, gt, idx, deltas, tag):
    gt_r, idx_r, del_r, ok = ref
    assert np.array_equal(idx, idx_r), f"{tag}: anchor indices differ from the restatement"
    assert _same_bits(deltas[ok, :2], del_r[ok, :2]), f"{tag}: dx, dy"
    u = _ulps(deltas[ok, 2:], del_r[ok, 2:])
    print(f"{tag}: dw, dh max {u} ulp")
    assert u <= 1, f"{tag}: dw, dh {u} ulp"
    if gt_r is not None:
        assert gt.shape == gt_r.shape
        for lo, hi in ((0, 7), (9, gt_r.shape[2])):
            assert _same_bits(gt[..., lo:hi], gt_r[..., lo:hi]), f"{tag}: dense gt columns {lo}:{hi}"
        assert _ulps(gt[..., 7:9], gt_r[..., 7:9]) <= 1, f"{tag}: dense gt columns 7:9"
    else:
        assert gt is None


def _ops_run(case, d, parallel):
    from squeezedet_pytorch_amd import ops
    gt, idx, deltas = ops.encode_gt(d[0], d[1], d[2], d[3], case["C"], dense=case["dense"], parallel=parallel)
    torch.cuda.synchronize()
    return (None if gt is None else gt.cpu().numpy()), idx.cpu().numpy(), deltas.cpu().numpy()


def _sweep_ids(groups):
    return [n for n, c in CASES.items() if c["group"] in groups]


@pytest.mark.parametrize("name", _sweep_ids(("grid", "unaligned", "cloud", "past256", "big")))
def test_sweep_through_ops(name):
    """every case through ops.encode_gt, both parallel forms, against the restatement and against each other"""
    case = CASES[name]
    pc = _counts(case)
    if case["group"] == "big":
        assert pc["lds_attribute"] and not case["dense"]
    ref = _reference(case)
    d = _pack(case)
    out = {}
    for parallel in (True, False):
        out[parallel] = _ops_run(case, d, parallel)
        _check(case, ref, *out[parallel], f"{name} parallel={parallel}")
    (gp, ip, dp), (gs, is_, ds) = out[True], out[False]
    assert ip.tobytes() == is_.tobytes() and dp.tobytes() == ds.tobytes() and (gp is None or gp.tobytes() == gs.tobytes())
    if case["dense"]:
        assert int(gp[..., 0].sum()) == int(ref[3].sum())
        empty = [b for b, bx in enumerate(case["boxes"]) if bx.shape[0] == 0]
        assert empty or case["group"] == "cloud"
        assert all(not gp[b].any() for b in empty)


@pytest.mark.parametrize("g", range(len(R.GRIDS)), ids=list(R.GRIDS))
def test_fixture_sets_on_device(golden_dir, g):
    """the sets of tests/golden/gt_encode_grids.npz as one batch: the device against the restatement everywhere, and against the
    REFERENCE's own indices and deltas on every determined prefix (the whole determined set)"""
    gold = np.load(os.path.join(golden_dir, "gt_encode_grids.npz"))
    name = str(gold["grids"][g])
    kinds = [str(k) for k in gold["kinds"]]
    k = f"g{g}_"
    case = dict(name=f"fixture-{name}", anchors=R.grid_anchors(name), boxes=[gold[k + f"boxes{s}"] for s in range(len(kinds))],
                cls=[gold[k + f"cls{s}"] for s in range(len(kinds))], C=3, dense=True, geom=f"fixture-{name}", group="fixture")
    _counts(case)
    ref = _reference(case)
    d = _pack(case)
    for parallel in (True, False):
        gt, idx, deltas = _ops_run(case, d, parallel)
        _check(case, ref, gt, idx, deltas, f"fixture {name} parallel={parallel}")
        lo = 0
        for s, kind in enumerate(kinds):
            idx_ref, del_ref, unique = gold[k + f"idx{s}"], gold[k + f"deltas{s}"], gold[k + f"unique{s}"]
            nz = np.nonzero(~unique)[0]
            p = int(nz[0]) if nz.size else unique.shape[0]
            assert kind != "determined" or p == unique.shape[0] >= 12
            assert np.array_equal(idx[lo:lo + p], idx_ref[:p]), f"{name} set {s}: differs from the reference where it is determined"
            assert _same_bits(deltas[lo:lo + p, :2], del_ref[:p, :2]) and _ulps(deltas[lo:lo + p, 2:], del_ref[:p, 2:]) <= 1
            lo += unique.shape[0]
    assert lo == ref[1].shape[0]


# ------------------------------------------------------------------------------------------------------------ through the C entry
GUARD = 64                     # floats before and after a buffer (a multiple of 4: the band keeps the buffer's alignment)


def _entry(d, case, gt_ptr, idx, deltas, parallel):
    from squeezedet_pytorch_amd import _native as nat
    total = int(d[0].shape[0])
    ws = torch.empty(max(total, 1) * 2, device="cuda", dtype=torch.float64) if parallel else None
    rc = nat.lib().sqd_encode_gt_fwd(nat.ptr(d[0]), nat.ptr(d[1]), nat.ptr(d[2]), nat.ptr(d[3]), ctypes.c_void_p(gt_ptr),
                                     nat.ptr(idx), nat.ptr(deltas), nat.ptr(ws), total, len(case["boxes"]), case["anchors"].shape[0], case["C"],
                                     nat.stream_handle(torch.device("cuda")))
    torch.cuda.synchronize()
    return rc


def _guarded(n, shift):
    """a NaN-filled float buffer of GUARD + shift + n + GUARD floats; the n floats in the middle start ``shift`` floats past a
    16-byte boundary"""
    buf = torch.full((GUARD + shift + n + GUARD,), float("nan"), device="cuda", dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * (GUARD + shift)


def _split(buf, n, shift):
    h = buf.cpu().numpy()
    lo = GUARD + shift
    return h[:lo], h[lo:lo + n], h[lo + n:]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("parallel", [True, False])
def test_unaligned_images_scalar_zeroing(shift, parallel):
    """A = 135, C = 4: 1755 floats per image, so images 1 .. 3 of four start off a 16-byte boundary (and with the base pointer itself
    4 bytes off, images 0, 2 and 3).  gt starts as NaN: afterwards every float is 0 or a written row, and the bands around it are
    untouched."""
    case = CASES["unaligned-A135-C4"]
    pc = _counts(case, gt_byte_offset=4 * shift)
    assert pc["unaligned_images"] == 3
    gt_r, idx_r, del_r, ok = ref = _reference(case)
    d = _pack(case)
    buf, p = _guarded(gt_r.size, shift)
    assert p % 16 == 4 * shift
    idx = torch.full((idx_r.shape[0],), -7, device="cuda", dtype=torch.int32)
    deltas = torch.full((idx_r.shape[0], 4), float("nan"), device="cuda")
    assert _entry(d, case, p, idx, deltas, parallel) == 0
    before, gt, after = _split(buf, gt_r.size, shift)
    assert np.isnan(before).all() and np.isnan(after).all(), "the encoder wrote outside gt"
    assert not np.isnan(gt).any(), "a float of gt was neither zeroed nor written"
    _check(case, ref, gt.reshape(gt_r.shape), idx.cpu().numpy(), deltas.cpu().numpy(), f"unaligned shift={shift} parallel={parallel}")


@pytest.mark.parametrize("parallel", [True, False])
def test_class_id_guard(parallel):
    """class ids -1 and C: the row is written with an all-zero class part and no float outside the row changes"""
    A, C = 33, 4
    src = CASES["overfull-A33"]
    bx = src["boxes"][0][:6]
    cls = np.array([-1, C, 0, C - 1, -1, C], np.int32)
    case = dict(name="class-guard", anchors=src["anchors"], boxes=[bx[:3], bx[3:]], cls=[cls[:3], cls[3:]], C=C, dense=True, geom="class-guard",
                group="guard")
    _counts(case)
    gt_r, idx_r, del_r, ok = ref = _reference(case)
    assert ok.all() and int(gt_r[..., 9:].sum()) == 2 and int(gt_r[..., 0].sum()) == 6
    d = _pack(case)
    buf, p = _guarded(gt_r.size, 0)
    idx = torch.full((6,), -7, device="cuda", dtype=torch.int32)
    deltas = torch.full((6, 4), float("nan"), device="cuda")
    assert _entry(d, case, p, idx, deltas, parallel) == 0
    before, gt, after = _split(buf, gt_r.size, 0)
    assert np.isnan(before).all() and np.isnan(after).all(), "a class id outside 0 .. C-1 wrote outside gt"
    gt = gt.reshape(gt_r.shape)
    _check(case, ref, gt, idx.cpu().numpy(), deltas.cpu().numpy(), f"class guard parallel={parallel}")
    offs = [0, 3, 6]
    for b in range(2):
        for k in range(offs[b], offs[b + 1]):
            row = gt[b, idx_r[k]]
            assert row[0] == 1. and row[9:].sum() == (1. if 0 <= cls[k] < C else 0.)


@pytest.mark.parametrize("A", [1, 33])
def test_more_boxes_than_anchors(A):
    """what the kernel does today with more boxes than anchors: the first A boxes get distinct anchors, the rest report A, their
    deltas rows keep what the buffer held and they write no gt row"""
    from squeezedet_pytorch_amd import ops
    case = CASES[f"overfull-A{A}"]
    _counts(case)
    gt_r, idx_r, del_r, ok = ref = _reference(case)
    n0 = case["boxes"][0].shape[0]
    n1 = min(A, 2)                                  # (image 1 has two boxes: at A = 1 its second one stays unassigned too)
    assert n0 == A + 5 and ok[:A].all() and not ok[A:n0].any() and ok[n0:n0 + n1].all() and not ok[n0 + n1:].any()
    d = _pack(case)
    for parallel in (True, False):
        gt, idx, deltas = _ops_run(case, d, parallel)
        _check(case, ref, gt, idx, deltas, f"overfull A={A} parallel={parallel}")
        assert sorted(idx[:A].tolist()) == list(range(A)) and np.all(idx[A:n0] == A)
        assert int(gt[0, :, 0].sum()) == A and int(gt[1, :, 0].sum()) == n1 and np.all(idx[n0 + n1:] == A)
        # the same through the C entry into pre-filled buffers
        buf, p = _guarded(gt_r.size, 0)
        idx_t = torch.full((idx_r.shape[0],), -7, device="cuda", dtype=torch.int32)
        del_t = torch.full((idx_r.shape[0], 4), float("nan"), device="cuda")
        assert _entry(d, case, p, idx_t, del_t, parallel) == 0
        before, gt2, after = _split(buf, gt_r.size, 0)
        assert np.isnan(before).all() and np.isnan(after).all()
        del2 = del_t.cpu().numpy()
        assert np.isnan(del2[~ok]).all() and not np.isnan(del2[ok]).any()
        assert gt2.tobytes() == gt.tobytes() and idx_t.cpu().numpy().tobytes() == idx.tobytes() and del2[ok].tobytes() == deltas[ok].tobytes()
    # the product's own entry refuses such a batch before any launch
    from squeezedet_pytorch_amd.annotations import encode_annotations
    with pytest.raises(IndexError):
        encode_annotations(case["cls"], case["boxes"], case["anchors"], case["C"], device="cuda")


def test_anchor_count_past_the_limit_is_refused():
    """A = 2^20 + 1: status 1 (the entry's argument check), nothing launched, nothing written"""
    from squeezedet_pytorch_amd import _native as nat
    from squeezedet_pytorch_amd import ops
    big = CASES[f"big-A{1 << 20}"]
    A = (1 << 20) + 1
    anchors = np.concatenate([big["anchors"], big["anchors"][:1]], 0)
    case = dict(big, name="past-limit", anchors=anchors, geom="past-limit")
    print(f"past-limit: A={A} lds_dynamic={((A + 31) // 32) * 4} (not launched)")
    d = _pack(case)
    n = d[0].shape[0]
    for parallel in (True, False):
        idx = torch.full((n,), -7, device="cuda", dtype=torch.int32)
        deltas = torch.full((n, 4), float("nan"), device="cuda")
        assert _entry(d, case, 0, idx, deltas, parallel) == nat.ERR_BAD_ARG
        assert torch.all(idx == -7) and torch.isnan(deltas).all()
    with pytest.raises(RuntimeError, match="status 1"):
        ops.encode_gt(d[0], d[1], d[2], d[3], 3, dense=False)
    # and the limit itself is accepted (test_sweep_through_ops[big-A1048576] checks what it computes)
    assert big["anchors"].shape[0] == 1 << 20


@pytest.mark.parametrize("name", ["unaligned-A135-C4", "past256-groups", "past256-late-conflicts"])
def test_stale_buffers(name):
    """another batch goes into the same idx / deltas / gt buffers first; then the case three times: identical bytes every time,
    equal to the restatement"""
    case = CASES[name]
    _counts(case)
    other = dict(case, name=name + "-other", geom=name + "-other", boxes=[b[::-1].copy() for b in case["boxes"][::-1]],
                 cls=[(c[::-1] + 1) % case["C"] for c in case["cls"][::-1]])
    gt_r, idx_r, del_r, ok = ref = _reference(case)
    assert ok.all()
    n = idx_r.shape[0]
    buf, p = _guarded(gt_r.size, 0)
    idx = torch.full((n,), -7, device="cuda", dtype=torch.int32)
    deltas = torch.full((n, 4), float("nan"), device="cuda")
    for parallel in (True, False):
        assert _entry(_pack(other), other, p, idx, deltas, parallel) == 0
        stale = (buf.cpu().numpy().tobytes(), idx.cpu().numpy().tobytes())
        d = _pack(case)
        runs = []
        for _ in range(3):
            assert _entry(d, case, p, idx, deltas, parallel) == 0
            runs.append((buf.cpu().numpy(), idx.cpu().numpy(), deltas.cpu().numpy()))
        assert runs[0][0].tobytes() != stale[0] and runs[0][1].tobytes() != stale[1]         # (the other batch really differed)
        for r in runs[1:]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(r, runs[0]))
        before, gt, after = _split(buf, gt_r.size, 0)
        assert np.isnan(before).all() and np.isnan(after).all()
        _check(case, ref, gt.reshape(gt_r.shape), runs[0][1], runs[0][2], f"stale {name} parallel={parallel}")


# ------------------------------------------------------------------------------------------------------------ through the product
def _product_case(grid, C, seed):
    arch, size, seed_ = R.GRIDS[grid]
    cfg = sqd.make_cfg(arch=arch, input_size=size, anchors_seed=seed_, num_classes=C, device="cuda")
    src = CASES[f"grid-{grid}-C1-dense"]
    rs = np.random.RandomState(seed)
    cls = [rs.randint(0, C, b.shape[0]).astype(np.int32) for b in src["boxes"]]
    return cfg, dict(src, name=f"product-{grid}-C{C}", cls=cls, C=C)


def test_encode_annotations_return_sparse():
    from squeezedet_pytorch_amd.annotations import encode_annotations
    cfg, case = _product_case("64x96", 3, 1)
    case = dict(case, dense=True)
    _counts(case)
    gt, idx, deltas, offs = encode_annotations(case["cls"], case["boxes"], cfg.anchors, 3, device="cuda", return_sparse=True)
    torch.cuda.synchronize()
    assert offs.cpu().tolist() == np.concatenate([[0], np.cumsum([b.shape[0] for b in case["boxes"]])]).tolist()
    _check(case, _reference(case), gt.cpu().numpy(), idx.cpu().numpy(), deltas.cpu().numpy(), "encode_annotations(return_sparse=True)")


def test_encode_annotations_sparse_form():
    from squeezedet_pytorch_amd import ops
    from squeezedet_pytorch_amd.annotations import encode_annotations
    cfg, case = _product_case("48x80", 20, 2)
    case = dict(case, dense=False)
    _counts(case)
    sgt = encode_annotations(case["cls"], case["boxes"], cfg.anchors, 20, device="cuda", dense=False)
    torch.cuda.synchronize()
    assert isinstance(sgt, ops.SparseGT)
    _check(case, _reference(case), None, sgt.anchor_idx.cpu().numpy(), sgt.deltas.cpu().numpy(), "encode_annotations(dense=False)")
    assert np.array_equal(sgt.boxes.cpu().numpy(), np.concatenate(case["boxes"], 0))
    assert np.array_equal(sgt.class_ids.cpu().numpy(), np.concatenate(case["cls"]))
    assert sgt.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([b.shape[0] for b in case["boxes"]])]).tolist()


class _Dataset:
    """portrait and landscape images with 1 .. 4 boxes each, class ids 0 .. 19"""

    def __init__(self, n, seed=0, sizes=((60, 100), (100, 60), (57, 91), (90, 40))):
        rs = np.random.RandomState(seed)
        self.images, self.ann = [], []
        for i in range(n):
            h, w = sizes[i % len(sizes)]
            self.images.append(rs.randint(0, 256, (h, w, 3), dtype=np.uint8))
            m = int(rs.randint(1, 5))
            x1 = rs.uniform(0, w * 0.6, m); y1 = rs.uniform(0, h * 0.6, m)
            b = np.stack([x1, y1, x1 + rs.uniform(6, w * 0.4, m), y1 + rs.uniform(6, h * 0.4, m)], 1).astype(np.float32)
            self.ann.append((rs.randint(0, 20, m).astype(np.int64), b))

    def __len__(self):
        return len(self.images)

    def load_image(self, i):
        return self.images[i], f"{i:06d}"

    def load_annotations(self, i):
        c, b = self.ann[i]
        return c.copy(), b.copy()


def test_train_loader_letterbox_encodes_the_transformed_boxes():
    """TrainLoader with letterbox on the 48x80 grid, C = 20: the batch's gt is the restatement applied to the loader's transformed
    boxes (``plan()``)"""
    from squeezedet_pytorch_amd.train_data import TrainLoader
    cfg = sqd.make_cfg(input_size=(48, 80), num_classes=20, device="cuda", batch_size=4, num_workers=2, letterbox=True)
    ds = _Dataset(8)
    plans = list(TrainLoader(ds, cfg, seed=7).plan())
    batches = list(TrainLoader(ds, cfg, seed=7))
    assert len(plans) == len(batches) == 2
    for n, (batch, p) in enumerate(zip(batches, plans)):
        boxes = [np.asarray(b, np.float32).reshape(-1, 4) for b in p["boxes"]]
        case = dict(name=f"loader-batch{n}", anchors=np.asarray(cfg.anchors, np.float64), boxes=boxes,
                    cls=[np.asarray(c, np.int32) for c in p["class_ids"]], C=20, dense=True, geom=f"loader-{n}", group="product")
        _counts(case)
        assert sum(b.shape[0] for b in boxes) >= 4
        gt = batch["gt"].cpu().numpy()
        ref = _reference(case)
        assert gt.shape == ref[0].shape == (4, 135, 29)
        for lo, hi in ((0, 7), (9, 29)):
            assert _same_bits(gt[..., lo:hi], ref[0][..., lo:hi]), f"loader batch {n}: dense gt columns {lo}:{hi}"
        assert _ulps(gt[..., 7:9], ref[0][..., 7:9]) <= 1
