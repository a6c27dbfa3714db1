#!/usr/bin/env python
"""Golden vectors for the GT encoder on grids other than KITTI's: the REFERENCE's ``compute_deltas`` (src/utils/boxes.py:84-135,
imported read-only as in make_golden_gt.py) on seeded box sets -> tests/golden/gt_encode_grids.npz.  Data only: per grid the
architecture name, input size and anchor seed (the test rebuilds the anchors with ``make_cfg``; this script asserts that they are
the reference's ``generate_anchors`` bit for bit), and per set the float32 xyxy boxes, class ids, the reference's anchor indices
and deltas, and the per-box "uniquely determined" flag of make_golden_gt.py.

Sets per grid: two random ones, a crowd, tiny boxes, integer-aligned boxes, far-away boxes (zero overlap with every anchor: the
nearest-anchor fallback), and a FULLY DETERMINED set.  The unscaled KITTI anchor shapes contain most boxes of a small image, so on
random sets the reference's pick stops being unique after a few boxes and the index comparison would be nearly empty.  The
determined set is built greedily: a proposed box is kept only if the reference's pick for it is unique given the picks so far;
the reference's ``compute_deltas`` then runs on the finished set and every flag must be set.

The archive is written with fixed member timestamps, so a re-run reproduces the committed file byte for byte.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gt_grids.py
"""
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
from make_golden import import_reference  # noqa: E402
import squeezedet_pytorch_amd as sqd  # noqa: E402
from gt_encode_ref import GRIDS  # noqa: E402     (names, input sizes and anchor seeds only)

KINDS = ('random', 'random', 'crowd', 'tiny', 'integer', 'far', 'determined')
MIN_DETERMINED = 12


def replay(ref_boxes, bx, anchors, axyxy, idx):
    """uniqueness of every pick, replayed with the reference's own arithmetic and its own taken-set sequence; also which boxes took
    the zero-overlap fallback"""
    taken = np.zeros(anchors.shape[0], bool)
    unique = np.zeros(bx.shape[0], bool)
    fallback = np.zeros(bx.shape[0], bool)
    bxywh = ref_boxes.xyxy_to_xywh(bx)
    for i in range(bx.shape[0]):
        ov = ref_boxes.compute_overlaps(axyxy, bx[i])
        free = ~taken
        best = ov[free].max()
        if best > 0:
            unique[i] = np.count_nonzero(ov[free] == best) == 1
            assert ov[idx[i]] == best
        else:
            d = np.sum((bxywh[i] - anchors) ** 2, axis=1)
            unique[i] = np.count_nonzero(d[free] == d[free].min()) == 1
            fallback[i] = True
            assert d[idx[i]] == d[free].min()
        taken[idx[i]] = True
    return unique, fallback


def determined_set(ref_boxes, rs, anchors, axyxy, H, W, want=16, tries=4000):
    """greedy: keep a proposal only if the reference's pick for it is unique given the picks so far"""
    A = anchors.shape[0]
    taken = np.zeros(A, bool)
    kept, picks = [], []
    for t in range(tries):
        if len(kept) == min(want, A):
            break
        if t % 2 == 0:                               # an anchor's own rectangle, jittered: a partial overlap with a clear winner
            j = rs.randint(A)
            w, h = anchors[j, 2], anchors[j, 3]
            box = axyxy[j] + rs.uniform(-0.25, 0.25, 4) * np.array([w, h, w, h])
        else:
            cx, cy = rs.uniform(0, W), rs.uniform(0, H)
            w, h = np.exp(rs.uniform(np.log(6), np.log(W))), np.exp(rs.uniform(np.log(6), np.log(H)))
            box = np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
        box = box.astype(np.float32)
        if not (box[2] - box[0] > 1 and box[3] - box[1] > 1):
            continue
        ov = ref_boxes.compute_overlaps(axyxy, box)
        free = ~taken
        best = ov[free].max()
        if not best > 0 or np.count_nonzero(ov[free] == best) != 1:
            continue
        j = int(np.nonzero(free & (ov == best))[0][0])
        taken[j] = True
        kept.append(box); picks.append(j)
    return np.array(kept, np.float32), np.array(picks, np.int32)


def box_sets(ref_boxes, rs, anchors, axyxy, H, W):
    def clip(b):
        b = np.asarray(b, np.float64)
        b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, W - 1); b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, H - 1)
        return b[(b[:, 2] - b[:, 0] > 1) & (b[:, 3] - b[:, 1] > 1)].astype(np.float32)

    sets = []
    for n in (12, 25):
        cx = rs.uniform(0, W, n); cy = rs.uniform(0, H, n)
        w = np.exp(rs.uniform(np.log(4), np.log(0.6 * W), n)); h = w * rs.uniform(0.4, 1.6, n)
        sets.append(clip(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)))
    # crowd: near-identical boxes compete for the same anchors
    sets.append(clip(np.array([0.35 * W, 0.25 * H, 0.7 * W, 0.8 * H]) + rs.uniform(-2, 2, (20, 4))))
    # tiny boxes inside one grid cell: exact IoU ties between cells
    cx = rs.uniform(6, W - 6, 12); cy = rs.uniform(6, H - 6, 12)
    sets.append(clip(np.stack([cx - 2, cy - 2.5, cx + 2, cy + 2.5], 1)))
    # integer-aligned boxes (exact arithmetic -> exact ties)
    x0 = rs.randint(0, W // 16 - 1, 10) * 16.; y0 = rs.randint(0, H // 16 - 1, 10) * 16.
    sets.append(clip(np.stack([x0, y0, x0 + 12, y0 + 10], 1)))
    # far away: zero overlap with every anchor (boxes.py:115-121); not clipped; the first two identical
    sets.append(np.array([[3. * W + 500, 50., 3. * W + 600, 120.], [3. * W + 500, 50., 3. * W + 600, 120.],
                          [3. * W + 510, 60., 3. * W + 590, 130.], [-900., -700., -800., -650.]], np.float32))
    det, picks = determined_set(ref_boxes, rs, anchors, axyxy, H, W)
    sets.append(det)
    return sets, picks


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the time of the run)"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for name, arr in arrays.items():
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arr), allow_pickle=False)


def main():
    _, _, ref_boxes, _ = import_reference()
    out = {'grids': np.array(list(GRIDS)), 'kinds': np.array(KINDS)}
    for g, (name, (arch, size, seed)) in enumerate(GRIDS.items()):
        cfg = sqd.make_cfg(arch=arch, input_size=size, anchors_seed=seed, device='cpu')
        anchors = cfg.anchors
        a_ref = ref_boxes.generate_anchors(cfg.grid_size, size, np.asarray(seed))
        assert a_ref.dtype == np.float64 and np.array_equal(a_ref, anchors), name
        axyxy = ref_boxes.xywh_to_xyxy(anchors)
        rs = np.random.RandomState(500 + g)
        sets, det_picks = box_sets(ref_boxes, rs, anchors, axyxy, size[0], size[1])
        assert len(sets) == len(KINDS)
        any_fallback = any_tie = False
        for s, bx in enumerate(sets):
            cls = rs.randint(0, 3, bx.shape[0])
            deltas, idx = ref_boxes.compute_deltas(bx.copy(), anchors)
            unique, fallback = replay(ref_boxes, bx, anchors, axyxy, idx)
            any_fallback |= bool(fallback.any()); any_tie |= not bool(unique.all())
            if KINDS[s] == 'determined':
                assert bx.shape[0] >= MIN_DETERMINED, (name, bx.shape[0])
                assert unique.all() and np.array_equal(idx, det_picks), name
            if KINDS[s] == 'far':
                assert fallback.all(), name
            k = f'g{g}_'
            out[k + f'boxes{s}'] = bx; out[k + f'cls{s}'] = cls.astype(np.int32)
            out[k + f'idx{s}'] = idx; out[k + f'deltas{s}'] = deltas; out[k + f'unique{s}'] = unique
            print(f'{name} set {s} ({KINDS[s]}): {bx.shape[0]} boxes, {int(unique.sum())} uniquely determined, {int(fallback.sum())} by distance')
        assert any_fallback, f'{name}: no box takes the zero-overlap fallback'
        assert any_tie, f'{name}: no exact tie'
        out[f'g{g}_arch'] = np.array(arch); out[f'g{g}_input_size'] = np.array(size, np.int32)
        out[f'g{g}_seed'] = np.asarray(seed, np.float32); out[f'g{g}_num_anchors'] = np.array([anchors.shape[0]], np.int32)
    path = os.path.join(HERE, 'gt_encode_grids.npz')
    write_npz(path, out)
    print(f'{path}: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
