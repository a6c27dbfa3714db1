"""A plain numpy restatement of the GT encoder's rule, written from the header of csrc/gt_encode.hip and from nothing else: it
calls neither the oracle nor the package.  tests/test_gt_encode_grids.py holds it to ``oracle.compute_deltas(ties='lowest')`` bit
for bit; tests/test_gt_encode_sweep_gpu.py holds the HIP encoder to it.  ``sweep_cases()`` is the one case list both share.

The rule.  Boxes are float32 xyxy, anchors float64 (cx, cy, w, h).  Per box, in input order:
  box (cx, cy, w, h)   float32 arithmetic: (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1 + 1, y2 - y1 + 1
  anchor corners       float64: c -+ 0.5 (s - 1)
  overlap              float64 inter / (union + 1e-10); the box area (x2 - x1) (y2 - y1) is a float32 product, widened afterwards
  distance             float64 ((dcx^2 + dcy^2) + dw^2) + dh^2, added left to right
  pick                 the free anchor of largest overlap if that overlap is > 0, else the free anchor of smallest distance; an
                       anchor is taken once; ties go to the LOWEST anchor index; with no anchor left the box stays unassigned
  deltas               float64 ((bcx - ax) / aw, (bcy - ay) / ah, log(bw / aw), log(bh / ah)) rounded to float32
  anchor_idx           the pick, or A for an unassigned box

``mutant``: one wrong convention at a time (MUTANTS), the CPU tier's teeth: every one of them has to move an index or a delta on
some sweep case, or the case list could not tell that kernel from the right one.
"""
import numpy as np

MUTANTS = ('ties_highest', 'ignore_taken', 'no_fallback', 'dist_xy_only', 'no_plus_one', 'unassigned_minus_one')

F32 = np.float32


def compute_deltas(boxes_xyxy, anchors_xywh, mutant=None):
    """-> (deltas float32 [n,4], anchor_idx int32 [n]).  The deltas row of an unassigned box is 0 here (the kernel leaves it
    unwritten)."""
    assert mutant is None or mutant in MUTANTS
    b = np.asarray(boxes_xyxy, F32).reshape(-1, 4)
    a = np.asarray(anchors_xywh, np.float64)
    A, n = a.shape[0], b.shape[0]
    plus = F32(0) if mutant == 'no_plus_one' else F32(1)
    bcx = (b[:, 0] + b[:, 2]) / F32(2)                                   # float32 throughout
    bcy = (b[:, 1] + b[:, 3]) / F32(2)
    bw = b[:, 2] - b[:, 0] + plus
    bh = b[:, 3] - b[:, 1] + plus
    barea = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])                    # float32 product
    assert bcx.dtype == F32 and bw.dtype == F32 and barea.dtype == F32
    b64, bcx, bcy, bw, bh, barea = (v.astype(np.float64) for v in (b, bcx, bcy, bw, bh, barea))
    ax, ay, aw, ah = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    x0, y0 = ax - 0.5 * (aw - 1.0), ay - 0.5 * (ah - 1.0)
    x1, y1 = ax + 0.5 * (aw - 1.0), ay + 0.5 * (ah - 1.0)
    aarea = (x1 - x0) * (y1 - y0)
    taken = np.zeros(A, bool)
    idx = np.empty(n, np.int32)
    deltas = np.zeros((n, 4), F32)
    last = mutant == 'ties_highest'
    for i in range(n):
        free = np.ones(A, bool) if mutant == 'ignore_taken' else ~taken
        if not free.any():
            idx[i] = -1 if mutant == 'unassigned_minus_one' else A
            continue
        lr = np.maximum(np.minimum(x1, b64[i, 2]) - np.maximum(x0, b64[i, 0]), 0.0)
        tb = np.maximum(np.minimum(y1, b64[i, 3]) - np.maximum(y0, b64[i, 1]), 0.0)
        inter = lr * tb
        ov = inter / ((aarea + barea[i] - inter) + 1e-10)
        best = ov[free].max()
        if best > 0 or mutant == 'no_fallback':
            hits = np.nonzero(free & (ov == best))[0]
        else:
            d0, d1, d2, d3 = bcx[i] - ax, bcy[i] - ay, bw[i] - aw, bh[i] - ah
            dist = d0 * d0 + d1 * d1
            if mutant != 'dist_xy_only':
                dist = (dist + d2 * d2) + d3 * d3
            hits = np.nonzero(free & (dist == dist[free].min()))[0]
        j = int(hits[-1] if last else hits[0])
        taken[j] = True
        idx[i] = j
        deltas[i] = [(bcx[i] - ax[j]) / aw[j], (bcy[i] - ay[j]) / ah[j], np.log(bw[i] / aw[j]), np.log(bh[i] / ah[j])]
    return deltas, idx


def encode_gt(class_ids, boxes_xyxy, anchors_xywh, num_classes, mutant=None, assigned=None):
    """The image's dense gt float32 [A, C+9] = [1, x1, y1, x2, y2, dx, dy, dw, dh, one-hot] as the kernel writes it: zero, then one
    row per assigned box; a class id outside 0 .. C-1 leaves the one-hot part zero; an unassigned box writes no row.
    ``assigned``: (deltas, anchor_idx) of these boxes if ``compute_deltas`` has run already.  -> (gt, deltas, anchor_idx)."""
    b = np.asarray(boxes_xyxy, F32).reshape(-1, 4)
    cls = np.asarray(class_ids).reshape(-1)
    A = np.asarray(anchors_xywh).shape[0]
    deltas, idx = compute_deltas(b, anchors_xywh, mutant) if assigned is None else assigned
    gt = np.zeros((A, num_classes + 9), F32)
    for i in range(b.shape[0]):
        j = int(idx[i])
        if not 0 <= j < A:
            continue
        gt[j, 0] = 1.
        gt[j, 1:5] = b[i]
        gt[j, 5:9] = deltas[i]
        if 0 <= int(cls[i]) < num_classes:
            gt[j, 9 + int(cls[i])] = 1.
    return gt, deltas, idx


# --------------------------------------------------------------------------------------------------------- host-side path counts
MAXB = 256                     # boxes / first choices of an image that encode_gt_kernel stages in LDS
STATIC_LDS = 16 * 24 + MAXB * 16 + MAXB * 16 + 4       # wave_c, s_box, s_cand, s_next of encode_gt_kernel
ATTR_LDS = 48 * 1024           # dynamic LDS above which sqd_encode_gt_fwd sets the kernel's attribute


def first_choices(boxes_xyxy, anchors_xywh):
    """Per box the unmasked pick (what gt_candidates_kernel hands the serial walk), by the rule with an empty taken set."""
    b = np.asarray(boxes_xyxy, F32).reshape(-1, 4)
    return np.array([compute_deltas(b[i:i + 1], anchors_xywh)[1][0] for i in range(b.shape[0])], np.int64)


def path_counts(case):
    """What the case makes the kernel do, derived from its inputs alone: conflicts (boxes whose first choice is taken when their
    turn comes, i.e. the masked scans of the parallel form), boxes past the LDS stage, those of them that walk without a scan,
    images whose dense slice starts off a 16-byte boundary, and the dynamic LDS the launch asks for."""
    anchors, C = case['anchors'], case['C']
    A = anchors.shape[0]
    conflicts = past = past_free = 0
    for bx in case['boxes']:
        n = bx.shape[0]
        past += max(0, n - MAXB)
        if n == 0:
            continue
        fc = first_choices(bx, anchors)
        idx = compute_deltas(bx, anchors)[1]
        clash = fc != idx                       # the first choice was free exactly when the masked pick equals it
        conflicts += int(clash.sum())
        past_free += int((~clash[MAXB:]).sum())
    row = C + 9
    unaligned = sum(1 for b in range(len(case['boxes'])) if (b * A * row * 4 + case.get('gt_byte_offset', 0)) % 16) if case['dense'] else 0
    lds = ((A + 31) // 32) * 4
    return dict(conflicts=conflicts, past_256=past, past_256_free=past_free,
                unaligned_images=unaligned, lds_dynamic=lds, lds_total=lds + STATIC_LDS, lds_attribute=lds > ATTR_LDS)


# ------------------------------------------------------------------------------------------------------------------ the sweep
KITTI_SEED = np.array([[34, 30], [75, 45], [38, 90], [127, 68], [80, 174], [196, 97], [194, 178], [283, 156], [381, 185]], F32)
SEED_1 = np.array([[30, 24]], F32)
SEED_20 = np.array([[12 + 9 * k + (k % 3) * 5, 10 + 7 * ((k * 7) % 20) + (k % 2) * 3] for k in range(20)], F32)

# name -> (arch, input size, anchors seed): the grids of tests/golden/gt_encode_grids.npz
GRIDS = {
    '64x96': ('squeezedet', (64, 96), KITTI_SEED),
    '48x80': ('squeezedet', (48, 80), KITTI_SEED),
    '720x1280': ('squeezedet', (720, 1280), KITTI_SEED),
    '192x624plus': ('squeezedetplus', (192, 624), KITTI_SEED),
    'seed1_96x160': ('squeezedet', (96, 160), SEED_1),
    'seed20_80x112': ('squeezedet', (80, 112), SEED_20),
}
CLASS_COUNTS = (1, 4, 20, 80, 256)
CLOUD_SIZES = (1, 31, 32, 33, 1023, 1024, 1025)
BIG_A = (393216 + 32, 1 << 20)


def grid_anchors(name):
    """(grid_h * grid_w * N, 4) float64 (cx, cy, w, h), ordered (y, x, k): cell centres at input * (1 / (2 grid) + i / grid), the
    expression the product's and the reference's ``generate_anchors`` share (the test checks it against ``make_cfg(...).anchors``)."""
    _, (in_h, in_w), seed = GRIDS[name]
    gh, gw, n = in_h // 16, in_w // 16, seed.shape[0]
    xs = in_w * (1 / (gw * 2) + np.linspace(0, 1, gw + 1)[:-1])
    ys = in_h * (1 / (gh * 2) + np.linspace(0, 1, gh + 1)[:-1])
    a = np.zeros((gh, gw, n, 4), np.float64)
    a[..., 0] = xs.reshape(1, gw, 1)
    a[..., 1] = ys.reshape(gh, 1, 1)
    a[..., 2:] = seed.reshape(1, 1, n, 2)
    return a.reshape(-1, 4)


def _rand_boxes(rs, n, H, W, lo=3.0):
    cx, cy = rs.uniform(0, W, n), rs.uniform(0, H, n)
    w = np.exp(rs.uniform(np.log(lo), np.log(0.8 * W), n))
    h = np.exp(rs.uniform(np.log(lo), np.log(0.8 * H), n))
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, W - 1)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, H - 1)
    b = b[(b[:, 2] - b[:, 0] > 1) & (b[:, 3] - b[:, 1] > 1)]
    return b.astype(F32)


def _grid_boxes(name):
    """Three images' worth of boxes for a grid: a random set with a repeated box (a conflict) and a far box (the distance fallback),
    and a crowd around one place."""
    _, (H, W), _ = GRIDS[name]
    rs = np.random.RandomState(1000 + sorted(GRIDS).index(name))
    a = _rand_boxes(rs, 10, H, W)
    a = np.concatenate([a, a[2:3], np.array([[3. * W, 0.3 * H, 3. * W + 0.2 * W, 0.3 * H + 0.3 * H]], F32),
                        np.array([[-2. * W, -2. * H, -2. * W + 9, -2. * H + 7]], F32), a[2:3]], 0)
    c = np.array([0.3 * W, 0.3 * H, 0.7 * W, 0.8 * H]) + rs.uniform(-2, 2, (7, 4))
    return a, c.astype(F32)


def _case(name, anchors, boxes, C, dense, seed, **kw):
    rs = np.random.RandomState(seed)
    cls = kw.pop('cls', None)
    if cls is None:
        cls = [rs.randint(0, C, b.shape[0]).astype(np.int32) for b in boxes]
    return dict(name=name, anchors=np.ascontiguousarray(anchors, dtype=np.float64), boxes=[np.ascontiguousarray(b, dtype=F32) for b in boxes],
                cls=cls, C=C, dense=dense, **kw)


def _cloud(rs, A, extent=200.0):
    return np.stack([rs.uniform(0, extent, A), rs.uniform(0, extent, A), rs.uniform(4, 60, A), rs.uniform(4, 60, A)], 1)


def _lattice(conflict_from=None):
    """~300 small boxes on the 720x1280 grid, one per cell of a 20 x 15 sub-lattice of the 80 x 45 cells, each sitting on the
    centre of its cell with the size of anchor shape 0 (34 x 30), slightly shrunk: its first choice is that cell's anchor 0 and no
    other box wants it.  ``conflict_from``: from that position on every third box repeats an earlier box (a conflict each)."""
    a = grid_anchors('720x1280').reshape(45, 80, 9, 4)
    out = []
    for gy in range(0, 45, 3):
        for gx in range(0, 80, 4):
            cx, cy = a[gy, gx, 0, 0], a[gy, gx, 0, 1]
            k = len(out)
            w, h = 30.0 + (k % 5) * 0.5, 26.0 + (k % 3) * 0.75
            out.append([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    b = np.array(out, F32)
    if conflict_from is not None:
        for k in range(conflict_from, b.shape[0], 3):
            b[k] = b[k - conflict_from // 2]
    return b


def _groups():
    """Interleaved groups of identical boxes: 6 distinct boxes, cycled 50 times (300 boxes), so that every box from the second
    round on finds its first choice taken and the k-th copy walks k - 1 anchors down its overlap order."""
    rs = np.random.RandomState(41)
    base = _rand_boxes(rs, 12, 720, 1280, lo=20.0)[:6]
    return np.tile(base, (50, 1))


_CASES = None


def sweep_cases():
    """The case list (built once).  A case: name, anchors float64 [A,4], boxes (one float32 [n,4] per image), cls (one int32 [n] per
    image), C, dense, group (the part of the sweep it belongs to) and geom (cases with the same geom share anchors and boxes: the
    CPU tier checks a geometry once)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = []
    empty = np.zeros((0, 4), F32)
    # grids x classes: B = 3, image 0 or image 1 empty
    for gi, g in enumerate(GRIDS):
        anchors = grid_anchors(g)
        a, c = _grid_boxes(g)
        for ci, C in enumerate(CLASS_COUNTS):
            first_empty = (gi + ci) % 2 == 0
            boxes = [empty, a, c] if first_empty else [a, empty, c]
            for dense in (True, False):
                cases.append(_case(f'grid-{g}-C{C}-{"dense" if dense else "sparse"}', anchors, boxes, C, dense, 7 + ci,
                                   geom=f'grid-{g}-{int(first_empty)}', group='grid'))
    # unaligned images: 135 x 13 floats per image, B = 4
    anchors = grid_anchors('48x80')
    a, c = _grid_boxes('48x80')
    cases.append(_case('unaligned-A135-C4', anchors, [a, c, empty, a[::-1].copy()], 4, True, 3, geom='unaligned', group='unaligned'))
    # bitmap word edges and the 1024-thread stride: random anchor clouds
    for k, A in enumerate(CLOUD_SIZES):
        rs = np.random.RandomState(200 + A)
        anchors = _cloud(rs, A)
        n = (1, 7, 20, 33, 40, 40, 40)[k]
        b = _rand_boxes(rs, n + 4, 200, 200)[:min(n, A)]
        far = np.array([[900., 900., 930., 915.]], F32)
        boxes = [b, far] if A > 1 else [b[:1], empty]
        cases.append(_case(f'cloud-A{A}', anchors, boxes, 3, True, 5, geom=f'cloud-{A}', group='cloud'))
    # past 256 boxes on 720x1280; one image with 0 boxes, one with 1, the long one last
    anchors = grid_anchors('720x1280')
    one = np.array([[100.5, 120.25, 300.75, 250.5]], F32)
    for nm, long_ in (('free', _lattice()), ('late-conflicts', _lattice(conflict_from=258)), ('groups', _groups())):
        cases.append(_case(f'past256-{nm}', anchors, [empty, one, long_], 3, True, 9, geom=f'past256-{nm}', group='past256'))
    # more boxes than anchors
    for A in (1, 33):
        rs = np.random.RandomState(300 + A)
        anchors = _cloud(rs, A)
        b = _rand_boxes(rs, A + 12, 200, 200)[:A + 5]
        assert b.shape[0] == A + 5
        cases.append(_case(f'overfull-A{A}', anchors, [b, b[:2]], 5, True, 11, geom=f'overfull-{A}', group='overfull'))
    # large anchor counts: sparse outputs only, 8 boxes, two of them identical
    for A in BIG_A:
        rs = np.random.RandomState(A % 9973)
        anchors = _cloud(rs, A, extent=4000.0)
        b = _rand_boxes(rs, 12, 4000, 4000, lo=8.0)[:7]
        b = np.concatenate([b[:5], b[1:2], b[5:]], 0)
        assert b.shape[0] == 8
        cases.append(_case(f'big-A{A}', anchors, [b[:3], b], 3, False, 13, geom=f'big-{A}', group='big'))
    _CASES = cases
    return cases


def geometries():
    """One case per distinct geom, in list order."""
    seen, out = set(), []
    for c in sweep_cases():
        if c['geom'] not in seen:
            seen.add(c['geom']); out.append(c)
    return out
