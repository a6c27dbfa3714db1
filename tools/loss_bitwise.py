#!/usr/bin/env python
"""Do two builds of the library give the same bits on every loss launch?  (A/B of a loss refactor against its parent commit.)

    python tools/loss_bitwise.py --parent-lib PARENT/libsqdhip.so [--new-lib PATH] [--out profiles/loss_refactor_bitwise.log]

The sixteen ``ops.loss_*`` wrappers are run from each library in a fresh child process of its own (``SQD_HIP_LIBRARY``; the second
child starts only if the first ended well, each under its own ``timeout``) on the same seeded operands, and every output is compared
by the SHA-256 of its raw bytes (a dpred reaches 1.1 GB), one line per case; the operands' digest is compared too.

Forward (losses, nobj or counts, mean4 of the mean entries): B in {1, 65} (65: both finalize forms past one wave), A in {1, 17, 257,
16848}, C in {1, 3, 16} for the <= 16-class entries and {1, 16, 17, 80, 256} for the many-class, sparse and masked ones; image 3 of
every 65-image batch has no positives (NaN bytes in the unmasked families, finite zeros in the masked one, which the child checks);
bitmap densities 0, 0.3 and 1 for the masked family.  Backward (dpred) on the same grid: a positive coef, a coef with negative
components (the -0 path of the negative rows), the mean form; the masked backward with the negative coef writes ``out=`` at a
storage offset of 4 bytes."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = (384, 1248)
WEIGHTS = (1.0, 3.75, 100.0, 6.0)
BS, AS = (1, 65), (1, 17, 257, 16848)
CS_NARROW, CS_MANY = (1, 3, 16), (1, 16, 17, 80, 256)
DENSITIES = (0.0, 0.3, 1.0)
EMPTY_IMAGE = 3


def digest(t):
    a = t.detach().contiguous().cpu().numpy()
    return [a.nbytes, hashlib.sha256(a.reshape(-1).view('uint8')).hexdigest()]


def operands(torch, ops, B, A, C, seed):
    """pred, anchors, SparseGT, dense gt: 1 .. 40 positives per image (none in image EMPTY_IMAGE of a batch), boxes around their
    anchors."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device='cuda', generator=g)
    pred = torch.randn(B, A, C + 5, device='cuda', generator=g)
    pred[..., :C + 1] *= 2.0
    pred[..., C + 1:] *= 0.4
    anchors = torch.stack([rnd(A) * SIZE[1], rnd(A) * SIZE[0], 20 + rnd(A) * 300, 20 + rnd(A) * 200], 1)
    idx, offsets = [], [0]
    for b in range(B):
        n = 0 if (b == EMPTY_IMAGE and B > 1) else min(A, 1 + (7 * b) % 40)
        idx.append(torch.randperm(A, device='cuda', generator=g)[:n])
        offsets.append(offsets[-1] + n)
    idx = torch.cat(idx)
    total = idx.shape[0]
    a = anchors[idx]
    ctr = a[:, :2] + (rnd(total, 2) - 0.5) * 0.3 * a[:, 2:]
    half = 0.5 * a[:, 2:] * (0.6 + 0.8 * rnd(total, 2))
    boxes = torch.cat([ctr - half, ctr + half], 1).contiguous()
    deltas = (rnd(total, 4) - 0.5) * 0.6
    cls = torch.randint(0, C, (total,), device='cuda', generator=g).to(torch.int32)
    sgt = ops.SparseGT(idx.to(torch.int32), boxes, deltas, cls, torch.tensor(offsets, dtype=torch.int32, device='cuda'))
    return pred, anchors, sgt, g


def bitmap(torch, ops, B, A, density, g):
    bits = (torch.rand(B, ops.ignore_words(A), 32, device='cuda', generator=g) < density).long()
    words = (bits << torch.arange(32, device='cuda')).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def coefs(torch, B, g):
    pos = 0.25 + torch.rand(3, B, device='cuda', generator=g)
    neg = pos.clone()
    neg[0] = -neg[0]
    neg[2, ::2] = -neg[2, ::2]
    return pos, neg


def child(path):
    sys.path.insert(0, ROOT)
    import torch
    from squeezedet_pytorch_amd import ops
    res = {}

    def put(case, names, tensors):
        res[case] = {n: digest(t) for n, t in zip(names, tensors)}

    seed = 0
    for B in BS:
        for A in AS:
            for C in sorted(set(CS_NARROW) | set(CS_MANY)):
                seed += 1
                pred, anchors, sgt, g = operands(torch, ops, B, A, C, seed)
                tag = f'B{B} A{A} C{C}'
                put(f'operands {tag}', ['pred', 'anchors'] + ['sgt.' + f for f in sgt._fields], [pred, anchors, *sgt])
                gmean = torch.full((1,), 0.75, device='cuda')
                cpos, cneg = coefs(torch, B, g)
                dense = [(n, getattr(ops, 'loss_fwd' + s), getattr(ops, 'loss_mean_fwd' + s), getattr(ops, 'loss_bwd' + s),
                          getattr(ops, 'loss_mean_bwd' + s))
                         for n, s, cs in (('narrow', '', CS_NARROW), ('many', '_many', CS_MANY)) if C in cs]
                if dense:
                    gt = ops.sparse_gt_to_dense(sgt, A, C)
                for fam, fwd, mean_fwd, bwd, mean_bwd in dense:
                    losses, nobj = fwd(pred, gt, anchors, SIZE, C, WEIGHTS)
                    put(f'{fam} fwd {tag}', ['losses', 'nobj'], [losses, nobj])
                    put(f'{fam} mean_fwd {tag}', ['losses', 'nobj', 'mean4'], mean_fwd(pred, gt, anchors, SIZE, C, WEIGHTS))
                    put(f'{fam} bwd coef+ {tag}', ['dpred'], [bwd(pred, gt, anchors, nobj, cpos, SIZE, C, WEIGHTS)])
                    put(f'{fam} bwd coef- {tag}', ['dpred'], [bwd(pred, gt, anchors, nobj, cneg, SIZE, C, WEIGHTS)])
                    put(f'{fam} mean_bwd {tag}', ['dpred'], [mean_bwd(pred, gt, anchors, nobj, gmean, SIZE, C, WEIGHTS)])
                if dense:
                    del gt
                if C not in CS_MANY:
                    continue
                losses, nobj = ops.loss_sparse_fwd(pred, sgt, anchors, SIZE, C, WEIGHTS)
                put(f'sparse fwd {tag}', ['losses', 'nobj'], [losses, nobj])
                put(f'sparse mean_fwd {tag}', ['losses', 'nobj', 'mean4'], ops.loss_sparse_mean_fwd(pred, sgt, anchors, SIZE, C, WEIGHTS))
                put(f'sparse bwd coef+ {tag}', ['dpred'], [ops.loss_sparse_bwd(pred, sgt, anchors, nobj, cpos, SIZE, C, WEIGHTS)])
                put(f'sparse bwd coef- {tag}', ['dpred'], [ops.loss_sparse_bwd(pred, sgt, anchors, nobj, cneg, SIZE, C, WEIGHTS)])
                put(f'sparse mean_bwd {tag}', ['dpred'], [ops.loss_sparse_mean_bwd(pred, sgt, anchors, nobj, gmean, SIZE, C, WEIGHTS)])
                if B > 1 and not bool(torch.isnan(losses[:, EMPTY_IMAGE]).any()):
                    raise SystemExit(f'{tag}: the image without positives gave no NaN in the unmasked sparse forward')
                for d in DENSITIES:
                    ign = bitmap(torch, ops, B, A, d, g)
                    mtag = f'{tag} density {d}'
                    losses, counts = ops.loss_masked_fwd(pred, sgt, ign, anchors, SIZE, C, WEIGHTS)
                    mean = ops.loss_masked_mean_fwd(pred, sgt, ign, anchors, SIZE, C, WEIGHTS)
                    put(f'masked fwd {mtag}', ['ignore', 'losses', 'counts'], [ign, losses, counts])
                    put(f'masked mean_fwd {mtag}', ['losses', 'counts', 'mean4'], mean)
                    buf = torch.empty(pred.numel() + 1, device='cuda')
                    out = buf[1:].view(pred.shape)
                    assert out.data_ptr() % 16 == 4
                    grads = [ops.loss_masked_bwd(pred, sgt, ign, anchors, counts, cpos, SIZE, C, WEIGHTS),
                             ops.loss_masked_bwd(pred, sgt, ign, anchors, counts, cneg, SIZE, C, WEIGHTS, out=out),
                             ops.loss_masked_mean_bwd(pred, sgt, ign, anchors, counts, gmean, SIZE, C, WEIGHTS)]
                    for kind, t in zip(('bwd coef+', 'bwd coef- out=+4B', 'mean_bwd'), grads):
                        put(f'masked {kind} {mtag}', ['dpred'], [t])
                    for t in (losses, mean[2], *grads):
                        if not bool(torch.isfinite(t).all()):
                            raise SystemExit(f'{mtag}: the masked launches gave a value that is not finite')
                    if B > 1 and (float(losses[0, EMPTY_IMAGE]) != 0.0 or float(losses[2, EMPTY_IMAGE]) != 0.0):
                        raise SystemExit(f'{mtag}: class / bbox of the image without positives are not zero')
                    del grads, buf, out
            print(f'  B={B} A={A}: {len(res)} cases so far', flush=True)
        torch.cuda.synchronize()
    with open(path, 'w') as fh:
        json.dump(res, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--new-lib', default=os.path.join(ROOT, 'squeezedet-pytorch_amd', 'csrc', 'libsqdhip.so'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'loss_refactor_bitwise.log'))
    ap.add_argument('--timeout', type=int, default=420, help='seconds per child')
    ap.add_argument('--dump', help='(child) run the cases from the library SQD_HIP_LIBRARY names and write their digests here')
    args = ap.parse_args()
    if args.dump:
        return child(args.dump)
    if not args.parent_lib:
        ap.error('--parent-lib is required')
    work = tempfile.mkdtemp(prefix='loss_bitwise_')
    dumps = {}
    for side, lib in (('parent', args.parent_lib), ('new', args.new_lib)):
        dumps[side] = os.path.join(work, side + '.json')
        r = subprocess.run(['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--dump', dumps[side]],
                           env=dict(os.environ, SQD_HIP_LIBRARY=os.path.abspath(lib)))
        if r.returncode != 0:
            print(f'{side} library {lib}: the child ended with status {r.returncode}; nothing more is run')
            return 2
    old, new = (json.load(open(dumps[s])) for s in ('parent', 'new'))
    lines, bad = [], 0
    if list(old) != list(new):
        lines.append('the two children ran different case lists')
        bad += 1
    for case in old:
        same = case in new and old[case] == new[case]
        bad += not same
        outs = ' '.join(f'{n}[{v[0]}]' for n, v in old[case].items())
        lines.append(f'{"BYTE-EQUAL" if same else "DIFFERENT "}  {case}: {outs}')
    n_op = sum(c.startswith('operands') for c in old)
    head = [f'parent library against this tree\'s ({os.path.relpath(args.new_lib, ROOT)}): {len(old) - n_op} cases + {n_op} operand sets, outputs compared by '
            f'the SHA-256 of their raw bytes (name[bytes]); {bad} differ']
    text = '\n'.join(head + lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text)
    print('\n'.join(head + [l for l in lines if not l.startswith('BYTE-EQUAL')]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
