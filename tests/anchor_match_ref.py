"""A plain numpy restatement of the IoU-threshold matcher's rule, written from the rule as DESIGN.md section 3 ("IoU-threshold
matching") and include/sqd_hip.h state it and from nothing else: it calls neither ``boxes.py`` nor the package (the primaries come from
tests/gt_encode_ref.py, the restatement of the encoder).  tests/test_anchor_match_host.py holds ``boxes.anchor_match`` to it bit for bit;
tests/test_anchor_match_gpu.py holds the HIP matcher to it.  ``cases()`` is the one case list both share.

The rule, per image.  Boxes float32 xyxy in input order, anchors float64 (cx, cy, w, h), the encoder's pick per box (the primaries).
  ov(i, j)    the encoder's overlap: anchor corners c -+ 0.5 (s - 1) in float64; the box area (x2 - x1) (y2 - y1) a float32 product,
              widened afterwards; inter / (union + 1e-10)
  scoring     every anchor j that is no primary of the image: m = max_i ov(i, j), i* = the lowest box index attaining it;
              m >= pos_iou: an extra positive of box i*; else m >= ign_iou: a band anchor; else a negative.  No boxes: neither.
  capacity    the first max_extra extras by ascending anchor index are kept, the rest are overflow
  list        total + B max_extra entries, image b at box_offsets[b] + b max_extra: the primaries in box order (copied), the kept extras
              in ascending anchor order (anchor j, box i*, the encoder's deltas expression), padding (anchor A, zeros)
  bitmap      ignore_in | band | overflow;  overflow[b] = the number of overflow anchors

``mutant``: one wrong convention at a time (MUTANTS), the CPU tier's teeth: each of them has to change some output on some case.
"""
import numpy as np

import gt_encode_ref as G

MUTANTS = ('strict_thresholds', 'ties_highest', 'primaries_reassigned', 'band_includes_positives', 'overflow_negative',
           'extras_by_box', 'no_plus_one', 'ignore_in_dropped')

F32 = np.float32


def overlaps(boxes_xyxy, anchors_xywh):
    """ov [n, A] float64."""
    b = np.asarray(boxes_xyxy, F32).reshape(-1, 4)
    a = np.asarray(anchors_xywh, np.float64)
    barea = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    assert barea.dtype == F32
    barea, b64 = barea.astype(np.float64), b.astype(np.float64)
    x0, y0 = a[:, 0] - 0.5 * (a[:, 2] - 1.0), a[:, 1] - 0.5 * (a[:, 3] - 1.0)
    x1, y1 = a[:, 0] + 0.5 * (a[:, 2] - 1.0), a[:, 1] + 0.5 * (a[:, 3] - 1.0)
    aarea = (x1 - x0) * (y1 - y0)
    ov = np.zeros((b.shape[0], a.shape[0]), np.float64)
    for i in range(b.shape[0]):
        lr = np.maximum(np.minimum(x1, b64[i, 2]) - np.maximum(x0, b64[i, 0]), 0.0)
        tb = np.maximum(np.minimum(y1, b64[i, 3]) - np.maximum(y0, b64[i, 1]), 0.0)
        inter = lr * tb
        ov[i] = inter / ((aarea + barea[i] - inter) + 1e-10)
    return ov


def _deltas(box, anchor, plus):
    bcx, bcy = (box[0] + box[2]) / F32(2), (box[1] + box[3]) / F32(2)               # float32 throughout
    bw, bh = box[2] - box[0] + plus, box[3] - box[1] + plus
    assert bcx.dtype == F32 and bw.dtype == F32
    bcx, bcy, bw, bh = (np.float64(v) for v in (bcx, bcy, bw, bh))
    return np.array([(bcx - anchor[0]) / anchor[2], (bcy - anchor[1]) / anchor[3], np.log(bw / anchor[2]), np.log(bh / anchor[3])]).astype(F32)


def match(anchors, boxes_list, prim_idx_list, prim_deltas_list, pos_iou, ign_iou, max_extra, ignore_in=None, mutant=None):
    """-> dict: anchor_idx int32 [T], box_idx int64 [T] (index into the concatenated boxes, -1 for padding), deltas float32 [T,4],
    offsets int32 [B+1], ignore bool [B,A], overflow int32 [B], and the per-image counts ``extras`` and ``band`` (before the capacity)."""
    assert mutant is None or mutant in MUTANTS
    a = np.asarray(anchors, np.float64)
    A, B = a.shape[0], len(boxes_list)
    ignore = np.zeros((B, A), bool)
    if ignore_in is not None and mutant != 'ignore_in_dropped':
        ignore |= np.asarray(ignore_in, bool)
    overflow, offsets = np.zeros(B, np.int32), np.zeros(B + 1, np.int32)
    n_extras, n_band = np.zeros(B, np.int64), np.zeros(B, np.int64)
    idx_out, box_out, del_out = [], [], []
    plus = F32(0) if mutant == 'no_plus_one' else F32(1)
    first = 0
    for b in range(B):
        bx = np.asarray(boxes_list[b], F32).reshape(-1, 4)
        prim = np.asarray(prim_idx_list[b], np.int64).reshape(-1)
        pdel = np.asarray(prim_deltas_list[b], F32).reshape(-1, 4)
        n = bx.shape[0]
        assert prim.shape[0] == n and pdel.shape[0] == n
        extras, band = [], []                           # (anchor, box)
        prim_box = np.arange(n)
        if n:
            ov = overlaps(bx, a)
            m = ov.max(0)
            is_prim = np.zeros(A, bool)
            is_prim[prim[(prim >= 0) & (prim < A)]] = True
            for j in range(A):
                hits = np.nonzero(ov[:, j] == m[j])[0]
                istar = int(hits[-1] if mutant == 'ties_highest' else hits[0])
                if is_prim[j]:
                    if mutant == 'primaries_reassigned':
                        prim_box[np.nonzero(prim == j)[0][0]] = istar
                    continue
                up = (m[j] > pos_iou) if mutant == 'strict_thresholds' else (m[j] >= pos_iou)
                mid = (m[j] > ign_iou) if mutant == 'strict_thresholds' else (m[j] >= ign_iou)
                if up:
                    extras.append((j, istar))
                if mid and (not up or mutant == 'band_includes_positives'):
                    band.append(j)
        n_extras[b], n_band[b] = len(extras), len(band)
        kept, over = extras[:max_extra], extras[max_extra:]
        if mutant == 'extras_by_box':
            kept = sorted(kept, key=lambda e: (e[1], e[0]))
        overflow[b] = len(over)
        ignore[b, band] = True
        if mutant != 'overflow_negative':
            ignore[b, [j for j, _ in over]] = True
        pad = max_extra - len(kept)
        idx_out.append(np.concatenate([prim, [j for j, _ in kept], [A] * pad]).astype(np.int32))
        box_out.append(np.concatenate([prim_box + first, [i + first for _, i in kept], [-1] * pad]).astype(np.int64))
        d = np.zeros((n + max_extra, 4), F32)
        d[:n] = pdel
        if mutant == 'primaries_reassigned':
            for k in range(n):
                if prim_box[k] != k and 0 <= prim[k] < A:
                    d[k] = _deltas(bx[prim_box[k]], a[prim[k]], plus)
        for k, (j, i) in enumerate(kept):
            d[n + k] = _deltas(bx[i], a[j], plus)
        del_out.append(d)
        first += n
        offsets[b + 1] = offsets[b] + n + max_extra
    return dict(anchor_idx=np.concatenate(idx_out), box_idx=np.concatenate(box_out), deltas=np.concatenate(del_out, 0), offsets=offsets,
                ignore=ignore, overflow=overflow, extras=n_extras, band=n_band)


def primaries(case):
    """The encoder's output for a case, by its restatement: (anchor_idx per image, deltas per image; an unassigned box has zero deltas)."""
    out = [G.compute_deltas(b, case['anchors']) for b in case['boxes']]
    return [o[1] for o in out], [o[0] for o in out]


_REF = {}


def reference(case, mutant=None):
    """``match`` of a case (memoised: the tests share it and leave it unchanged)."""
    key = (case['name'], mutant)
    if key not in _REF:
        if (case['name'], 'prim') not in _REF:
            _REF[(case['name'], 'prim')] = primaries(case)
        idx, dl = _REF[(case['name'], 'prim')]
        _REF[key] = match(case['anchors'], case['boxes'], idx, dl, case['pos_iou'], case['ign_iou'], case['max_extra'], case['ignore_in'], mutant)
        for v in _REF[key].values():
            v.setflags(write=False)
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------ the case list
EMPTY = np.zeros((0, 4), F32)


def _case(name, anchors, boxes, pos_iou, ign_iou, max_extra, C=3, seed=0, ignore_density=0.0, overflows=False, **kw):
    rs = np.random.RandomState(seed)
    anchors = np.ascontiguousarray(anchors, dtype=np.float64)
    boxes = [np.ascontiguousarray(b, dtype=F32).reshape(-1, 4) for b in boxes]
    cls = [rs.randint(0, C, b.shape[0]).astype(np.int32) for b in boxes]
    ign = rs.rand(len(boxes), anchors.shape[0]) < ignore_density if ignore_density > 0 else None
    return dict(name=name, anchors=anchors, boxes=boxes, cls=cls, C=C, pos_iou=float(pos_iou), ign_iou=float(ign_iou),
                max_extra=int(max_extra), ignore_in=ign, overflows=bool(overflows), **kw)


def _around(anchors, picks, rs, jitter):
    """Boxes made from the anchors ``picks``, their corners moved by up to ``jitter`` of the anchor's size: what overlaps those anchors
    (and their neighbours) well."""
    out = []
    for j in picks:
        cx, cy, w, h = anchors[j]
        d = rs.uniform(-jitter, jitter, 4) * np.array([w, h, w, h])
        out.append([cx - 0.5 * (w - 1) + d[0], cy - 0.5 * (h - 1) + d[1], cx + 0.5 * (w - 1) + d[2], cy + 0.5 * (h - 1) + d[3]])
    return np.array(out, F32).reshape(-1, 4)


def kitti_anchors():
    """The KITTI grid (24 x 78 cells x 9 shapes = 16848 anchors on 384 x 1248), by ``gt_encode_ref.grid_anchors``' expression."""
    gh, gw, seed = 24, 78, G.KITTI_SEED
    xs = 1248 * (1 / (gw * 2) + np.linspace(0, 1, gw + 1)[:-1])
    ys = 384 * (1 / (gh * 2) + np.linspace(0, 1, gh + 1)[:-1])
    a = np.zeros((gh, gw, 9, 4), np.float64)
    a[..., 0], a[..., 1], a[..., 2:] = xs.reshape(1, gw, 1), ys.reshape(gh, 1, 1), seed.reshape(1, 1, 9, 2)
    return a.reshape(-1, 4)


_CASES = None


def cases():
    """The case list (built once).  A case: name, anchors float64 [A,4], boxes (one float32 [n,4] per image), cls, C, pos_iou, ign_iou,
    max_extra, ignore_in (bool [B,A] or None), overflows (whether some image must overflow)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    # the small grids of the encoder's sweep with their boxes (a repeated box: a tie between two boxes at every anchor; a far box; a
    # crowd), plus boxes around a few anchors so that the thresholds have something on either side; image 1 has no box
    for k, g in enumerate(('64x96', '48x80', 'seed20_80x112')):
        anchors = G.grid_anchors(g)
        a, c = G._grid_boxes(g)
        rs = np.random.RandomState(70 + k)
        near = _around(anchors, rs.choice(anchors.shape[0], 4, replace=False), rs, 0.12)
        out.append(_case(f'grid-{g}', anchors, [np.concatenate([a, near], 0), EMPTY, c], 0.5, 0.35, 128, seed=k, ignore_density=0.1 * k))
    # bitmap word edges: random anchor clouds, boxes around some of the anchors
    for A in (1, 31, 32, 33, 1023, 1025):
        rs = np.random.RandomState(400 + A)
        anchors = G._cloud(rs, A, extent=min(200.0, 20.0 + 6.0 * A ** 0.5))      # dense enough for anchors to share a box
        n = min(A, 6)
        if A > 1:                                       # the last anchor (the top bit of the tail word) nearly repeats anchor 0: one of the
            anchors[A - 1] = anchors[0] * 1.03          # two is the primary of the box around anchor 0, the other an extra
        b0 = _around(anchors, np.concatenate([[0], 1 + rs.choice(A - 1, n - 1, replace=False)]) if A > 1 else [0], rs, 0.1)
        b1 = _around(anchors, rs.choice(A, min(A, 3), replace=False), rs, 0.2)
        out.append(_case(f'cloud-A{A}', anchors, [b0, b1, EMPTY], 0.5, 0.3, 40, seed=A, ignore_density=0.2 if A in (33, 1025) else 0.0))
    # an image with no boxes at all next to one with boxes, and a batch of one
    anchors = G.grid_anchors('64x96')
    rs = np.random.RandomState(11)
    near = _around(anchors, [40, 41, 100], rs, 0.1)
    out.append(_case('no-boxes-first', anchors, [EMPTY, near], 0.45, 0.3, 64, seed=1, ignore_density=0.3))
    out.append(_case('one-image', anchors, [near], 0.45, 0.3, 64, seed=2))
    # two identical boxes: every anchor ties between them, the lower index owns the extras
    two = np.concatenate([near[:1], near[:1], near[2:]], 0)
    out.append(_case('identical-boxes', anchors, [two, two[::-1].copy()], 0.4, 0.25, 32, seed=3))
    # the boundary: pos_iou (then ign_iou) is the computed overlap of a chosen (box, anchor) pair -- >= takes it, > would not
    ov = overlaps(near, anchors)
    prim = G.compute_deltas(near, anchors)[1]
    cand = [(ov[:, j].max(), j) for j in range(anchors.shape[0]) if j not in set(prim.tolist()) and 0.3 < ov[:, j].max() < 0.8]
    cand.sort()
    edge_pos, edge_ign = cand[len(cand) // 2], cand[len(cand) // 4]
    assert edge_ign[0] < edge_pos[0]
    out.append(_case('boundary-pos', anchors, [near], edge_pos[0], edge_ign[0], 64, seed=4, edge=(int(edge_pos[1]), int(edge_ign[1]))))
    # capacity: max_extra = 0, the exact number of extras of the fullest image, and one fewer
    cap_boxes = [near, _around(anchors, [7, 150], rs, 0.05)]
    probe = _case('capacity-probe', anchors, cap_boxes, 0.4, 0.3, 0, seed=5)
    idx, dl = primaries(probe)
    most = int(match(anchors, cap_boxes, idx, dl, 0.4, 0.3, 0)['extras'].max())
    assert most >= 2
    out.append(_case('capacity-0', anchors, cap_boxes, 0.4, 0.3, 0, seed=5, overflows=True))
    out.append(_case('capacity-exact', anchors, cap_boxes, 0.4, 0.3, most, seed=5))
    out.append(_case('capacity-one-fewer', anchors, cap_boxes, 0.4, 0.3, most - 1, seed=5, ignore_density=0.15, overflows=True))
    # more than 256 boxes in one image (the staging chunk): the lattice of the encoder's sweep on 720x1280, A = 32400 (127 blocks of
    # the count table).  The boxes are small (30 x 26 on a 16-pixel lattice), so the thresholds are low; 2950 extras against a
    # capacity of 1024: the overflow bits spread over many blocks
    out.append(_case('past256', G.grid_anchors('720x1280'), [EMPTY, G._lattice()], 0.2, 0.12, 1024, seed=6, overflows=True))
    _CASES = out
    return out


def kitti_case():
    """The KITTI grid, B = 3 (GPU tier; the CPU tier checks its counts too): cars of 20..400 px, as the estimate in DESIGN.md."""
    rs = np.random.RandomState(2024)
    anchors = kitti_anchors()
    boxes = []
    for n in (5, 0, 11):
        w = rs.uniform(20, 400, n)
        h = np.minimum(w / rs.uniform(0.4, 2.0, n), 380)
        x, y = rs.uniform(0, 1247 - w), rs.uniform(0, 383 - h)
        boxes.append(np.stack([x, y, x + w, y + h], 1).astype(F32).reshape(-1, 4))
    return _case('kitti-B3', anchors, boxes, 0.5, 0.4, 512, seed=7, ignore_density=0.05)
