"""float64 reference of the masked sparse loss (``ops.loss_masked_*``), derived from ``fp64_ref.loss`` (helper module of
tests/test_ignore_host.py and tests/test_ignore_gpu.py; no project kernels).

Per image: pos = the rows with gt mask 1, ign = the rows whose ignore bit is set and that are not in pos, n_obj = |pos|, n_neg =
A - n_obj - |ign|.  The masked loss of the image IS the unmasked loss of the image with the rows of ign taken out of pred, gt and
the anchors: the positive rows and the three / n_obj terms are taken over as they are, and the negative term and the negative rows
come out re-normalised from A - n_obj to n_neg (the unmasked denominator of the shortened image), the magnitudes M with them.  So
each image is one ``fp64_ref.loss`` call on its kept rows (B = 1, the upstream gradients of the image handed over as they reach the
kernel), scattered back to [A, C+5] with exact zeros (M = 0) on the rows of ign.  Two conventions have no unmasked counterpart:

* n_obj = 0: class = pos = bbox = 0 and only sigmoid(conf)^2 terms are left: a closed form (``_negatives_only``) in the V algebra
  of fp64_ref, which has no branch to flip;
* n_neg = 0 with n_obj > 0: neg = 0.  ``fp64_ref.loss`` has 0 / 0 there, so one stand-in negative row is appended whose confidence
  logit is -200: its sigmoid^2 is 1e-174 in float64 and 0 in float32, below every bar by 150 orders of magnitude; its gradient row
  is dropped.
"""
import numpy as np
import torch

import fp64_ref as R

F64, F32 = torch.float64, torch.float32
STAND_IN_LOGIT = -200.0


def _f32(v):
    return float(torch.tensor(float(v), dtype=F32))


def _negatives_only(z, u_score, w_neg, n_neg):
    """An image without positives: kept rows with confidence logits ``z`` [n] (n = n_neg > 0).  -> (neg V 0-dim, dconf V [n]) for the
    upstream gradient ``u_score`` of the score component; the chain of fp64_ref._loss_chain at mask = 0."""
    conf = R._div(R._c(torch.tensor(1.0, dtype=F64)), R._add(R._c(torch.tensor(1.0, dtype=F64)), R._exp(R._neg(R._lf(z)))))
    ee = R._neg(conf)
    e2 = R._mul(ee, ee)
    nn = R._lf(torch.tensor(float(n_neg), dtype=F64))
    neg = R._div(R._mul(R._c(torch.tensor(w_neg, dtype=F64)), R._sum(e2, 0, R.SUM_DEPTH_A)), nn)
    us = R._V(torch.tensor(u_score, dtype=F64), torch.tensor(abs(u_score), dtype=F64))
    k = R._mul(us, R._div(R._c(torch.tensor(w_neg, dtype=F64)), nn))
    dL_de = R._mul(R._mul(R._c(torch.tensor(2.0, dtype=F64)), k), ee)
    dconf = R._neg(R._mul(R._mul(dL_de, conf), R._sub(R._c(torch.tensor(1.0, dtype=F64)), conf)))
    return neg, dconf


def _negatives_only_f32(z, u_score, w_neg, n_neg):
    """The same in a plain float32 chain (the b32 member of the Refs)."""
    z = z.to(F32)
    conf = 1.0 / (1.0 + torch.exp(-z))
    neg = torch.tensor(w_neg, dtype=F32) * (conf * conf).sum() / float(n_neg)
    k = torch.tensor(u_score, dtype=F32) * (torch.tensor(w_neg, dtype=F32) / float(n_neg))
    return neg, -(2.0 * k * (-conf)) * conf * (1.0 - conf)


def masked_loss(pred, gt, ign, anchors, input_size, C, weights, gmean=None, coef=None):
    """``fp64_ref.loss`` for the masked launches.  pred [B,A,C+5], gt [B,A,C+9] (the dense gt the SparseGT stands for), ign bool [B,A]
    (the bitmap, positives' own bits included as they come), anchors [A,4].  -> dict: ``losses`` [4,B] / ``mean4`` [4] Ref,
    ``counts`` [2,B] = (n_obj, n_neg) exact, ``dmean`` / ``dcoef`` Ref of dpred [B,A,C+5] with ``*_alt`` and ``flips`` [B,A] as
    ``fp64_ref.loss`` returns them, ``ign`` bool [B,A] = the rows that must be exact zeros."""
    pred, gt, anchors = pred.detach().cpu().float(), gt.detach().cpu().float(), anchors.detach().cpu().float()
    ign = torch.as_tensor(np.asarray(ign)).bool()
    B, A, W = pred.shape
    w_neg = _f32(weights[2])
    gm = None if gmean is None else float(np.float32(gmean) / np.float32(B))       # the kernel's gmean[0] / (float)B
    cf = None if coef is None else coef.detach().cpu().to(F32)
    names = ([] if gm is None else ['dmean']) + ([] if cf is None else ['dcoef'])
    out = {'counts': torch.zeros(2, B, dtype=F64), 'flips': torch.zeros(B, A, dtype=torch.bool), 'ign': torch.zeros(B, A, dtype=torch.bool)}
    L = [torch.zeros(4, B, dtype=F64), torch.zeros(4, B, dtype=F64), torch.zeros(4, B, dtype=F32)]
    D = {n: [torch.zeros(B, A, W, dtype=F64), torch.zeros(B, A, W, dtype=F64), torch.zeros(B, A, W, dtype=F32), torch.zeros(B, A, W, dtype=F64)]
         for n in names}
    for b in range(B):
        pos = gt[b, :, 0] > 0
        ig = ign[b] & ~pos
        keep = ~ig
        n_obj, n_neg = int(pos.sum()), int(keep.sum()) - int(pos.sum())
        out['counts'][:, b] = torch.tensor([n_obj, n_neg], dtype=F64)
        out['ign'][b] = ig
        if n_obj == 0:
            if n_neg == 0:
                continue                                     # every row ignored: exact zeros everywhere
            z = pred[b, keep, C]
            ups = {'dmean': gm, 'dcoef': None if cf is None else float(cf[1, b])}
            neg, _ = _negatives_only(z, 0.0, w_neg, n_neg)
            neg32, _ = _negatives_only_f32(z, 0.0, w_neg, n_neg)
            for j in (1, 3):
                L[0][j, b], L[1][j, b], L[2][j, b] = neg.v, neg.m, neg32
            for n in names:
                _, dconf = _negatives_only(z, ups[n], w_neg, n_neg)
                _, d32 = _negatives_only_f32(z, ups[n], w_neg, n_neg)
                D[n][0][b, keep, C], D[n][1][b, keep, C], D[n][2][b, keep, C], D[n][3][b, keep, C] = dconf.v, dconf.m, d32, dconf.v
            continue
        p, g, an = pred[b, keep], gt[b, keep], anchors[keep]
        if n_neg == 0:                                       # the stand-in negative row (module docstring)
            row = torch.zeros(1, W)
            row[0, C] = STAND_IN_LOGIT
            p, g = torch.cat([p, row]), torch.cat([g, torch.zeros(1, g.shape[1])])
            an = torch.cat([an, torch.tensor([[8.0, 8.0, 5.0, 5.0]])])
        r = R.loss(p.unsqueeze(0), g.unsqueeze(0), an, input_size, C, weights, gmean=gm, coef=None if cf is None else cf[:, b:b + 1])
        assert float(r['nobj'][0]) == n_obj
        nk = int(keep.sum())
        for i in range(3):
            L[i][:, b] = r['losses'][i][:, 0]
        out['flips'][b, keep] = r['flips'][0, :nk]
        for n in names:
            for i in range(3):
                D[n][i][b, keep] = r[n][i][0, :nk].to(D[n][i].dtype)
            D[n][3][b, keep] = r[n + '_alt'][0, :nk]
    assert not any(torch.isnan(t).any() for t in L[:2]), 'the masked reference holds no NaN'
    out['losses'] = R.Ref(*L)
    out['mean4'] = R.Ref(L[0].mean(1), (L[1].sum(1) + R.SUM_DEPTH_B * L[0].abs().sum(1)) / B, L[2].mean(1))
    for n in names:
        out[n] = R.Ref(*D[n][:3])
        out[n + '_alt'] = D[n][3]
    return out


def case_with_ignore(LG, A, C, seed, density):
    """``LG.random_case`` (LG = tests/test_fp64_loss_gpu) with the four kinds of image the conventions are about, and their bitmaps:
    image 0: positives and negatives, bits at ``density`` (positives' own bits among them); image 1: n_obj = 0, bits at ``density``;
    image 2: positives, every bit set (n_neg = 0: the positives win over their own bits); image 3: n_obj = 0 and every bit set
    (all zeros).  -> (pred, gt, anchors, ign bool [4, A])."""
    n0, n2 = max(1, A // 10), max(1, A // 20)
    pred, gt, anchors = LG.random_case(4, A, C, seed=seed, nobj=[n0, 0, n2, 0])
    rs = np.random.RandomState(seed + 7)
    ign = np.zeros((4, A), dtype=bool)
    ign[:2] = rs.rand(2, A) < density
    if density > 0 and A > 1:
        ign[0, int(torch.nonzero(gt[0, :, 0] > 0)[0])] = True       # a positive whose own bit is set
    ign[2:] = True
    return pred, gt, anchors, ign


def boundary_cases():
    """Hand-checkable constructions of the ignore rule: [(name, anchors float64 [n,4], ignore boxes float32 [m,4], overlap, expected
    bool [n])].  The anchor (20, 20, 11, 11) has the corners 15 .. 25 on both axes and the area 100."""
    f = np.float32
    one = np.array([[20., 20., 11., 11.]])
    below20, below15 = np.nextafter(f(20), f(-np.inf)), np.nextafter(f(15), f(-np.inf))
    return [
        ('inside at overlap 1', one, np.array([[10, 10, 30, 30]], f), 1.0, [True]),
        ('a hair short at overlap 1', one, np.array([[10, 10, 30, np.nextafter(f(25), f(0))]], f), 1.0, [False]),
        ('exactly half at 0.5', one, np.array([[15, 0, 20, 40]], f), 0.5, [True]),
        ('half, one float32 step away', one, np.array([[below15, 0, below20, 40]], f), 0.5, [False]),
        ('two regions of 0.3 each', one, np.array([[15, 0, 18, 40], [22, 0, 25, 40]], f), 0.5, [False]),
        ('the larger of two regions counts', one, np.array([[15, 0, 18, 40], [19, 0, 25, 40]], f), 0.5, [True]),
        ('zero-area anchors', np.array([[20., 20., 1., 11.], [20., 20., 11., 1.], [20., 20., 1., 1.]]), np.array([[0, 0, 40, 40]], f), 2.0 ** -20,
         [False, False, False]),
        ('no regions', np.array([[20., 20., 11., 11.], [5., 5., 3., 3.]]), np.zeros((0, 4), f), 0.5, [False, False]),
    ]


class FlaggedDataset:
    """7 images of mixed sizes; image 3 has flagged boxes only, image 5 no annotation at all.  ``mode``: 'flags' (3-tuples), 'deleted'
    (the flagged boxes deleted, 2-tuples)."""
    SIZES = [(80, 120), (70, 100), (96, 128), (64, 200), (90, 90), (70, 100), (120, 160)]

    def __init__(self, mode='flags', seed=5):
        self.mode = mode
        rs = np.random.RandomState(seed)
        self.ann = []
        for i, (h, w) in enumerate(self.SIZES):
            n, m = (0, 2) if i == 3 else ((0, 0) if i == 5 else (2 + i % 2, i % 3))
            b = np.zeros((n + m, 4), np.float32)
            b[:, 0] = rs.uniform(4, w / 2, n + m); b[:, 1] = rs.uniform(4, h / 2, n + m)
            b[:, 2] = b[:, 0] + rs.uniform(8, w / 2 - 6, n + m); b[:, 3] = b[:, 1] + rs.uniform(8, h / 2 - 6, n + m)
            flags = np.zeros(n + m, np.uint8)
            flags[rs.permutation(n + m)[:m]] = 1
            self.ann.append((rs.randint(0, 3, n + m).astype(np.int64), b, flags))
        self.rgb_mean, self.rgb_std = np.array([93.877, 98.801, 95.923], np.float32), np.array([78.782, 80.130, 81.200], np.float32)

    def __len__(self):
        return len(self.SIZES)

    def image_size(self, i):
        return self.SIZES[i]

    def load_image(self, i):
        h, w = self.SIZES[i]
        return np.random.RandomState(100 + i).randint(0, 256, (h, w, 3)).astype(np.uint8)

    def load_annotations(self, i):
        c, b, f = self.ann[i]
        if self.mode == 'flags':
            return c, b, f
        return c[f == 0], b[f == 0]
