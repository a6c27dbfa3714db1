#!/usr/bin/env python
"""Do two builds of the library give the same bits on every stem launch?  (A/B of a stem refactor against its parent commit.)

    python tools/stem_bitwise.py --parent-lib PARENT/libsqdhip.so [--new-lib PATH] [--out profiles/stem_refactor_bitwise.log]

The stem wrappers of ``ops`` are run from each library in a fresh child process of its own (``SQD_HIP_LIBRARY``; a child starts only
if the one before it ended well, each under its own ``timeout``) on the same seeded operands, and every output is compared by the
SHA-256 of its raw bytes, one line per case; the operands' digest is compared too.  Each pair of children runs under three
environments, set before the child starts: the default, ``SQD_STEM_WAVE=0`` (the workgroup kernel where the wave kernel would run)
and ``SQD_STEM_WGRAD_GATHER=0`` (the dense pooled weight gradient where the gather kernel would run).

Ops: stem_conv_relu (relu on / off), stem_pool and stem_pool_squeeze (with and without argmax), stem_wgrad, stem_wgrad_pooled (with
and without the pooled tensor).  Shapes, B in {1, 3}: for the 3x3 / 64 stem 9x8 and 12x16 (maps smaller than one tile), 37x44 and
50x68 (partial tiles, all four borders), 50x70 and 37x45 (widths the 16-byte DMA refuses: the fallback kernels; stem_pool_squeeze
has no kernel there and its refusal is the recorded outcome), 64x96; for the 7x7 / 96 stem 30x50 and 64x96; and 384x1248 at B = 1
for the 3x3 stem."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = (('default', {}), ('SQD_STEM_WAVE=0', {'SQD_STEM_WAVE': '0'}), ('SQD_STEM_WGRAD_GATHER=0', {'SQD_STEM_WGRAD_GATHER': '0'}))
SHAPES3 = ((9, 8), (12, 16), (37, 44), (50, 68), (50, 70), (37, 45), (64, 96))
SHAPES7 = ((30, 50), (64, 96))
CASES = [(3, 64, B, H, W) for B in (1, 3) for H, W in SHAPES3] + [(7, 96, B, H, W) for B in (1, 3) for H, W in SHAPES7] \
    + [(3, 64, 1, 384, 1248)]


def digest(t):
    a = t.detach().contiguous().cpu().numpy()
    return [a.nbytes, hashlib.sha256(a.reshape(-1).view('uint8')).hexdigest()]


def child(path):
    sys.path.insert(0, ROOT)
    import torch
    from squeezedet_pytorch_amd import ops
    res = {}

    def put(case, names, tensors):
        res[case] = {n: digest(t) for n, t in zip(names, tensors)}

    for seed, (k, N, B, H, W) in enumerate(CASES, 1):
        g = torch.Generator(device='cuda').manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device='cuda', generator=g)
        tag = f'{k}x{k}/{N} B{B} {H}x{W}'
        x, w, b = rnd(B, 3, H, W), rnd(N, 3, k, k) * (2.0 / (3 * k * k)) ** 0.5, rnd(N) * 0.1
        ws, bs = rnd(16, N, 1, 1) * 0.2, rnd(16) * 0.1
        Ho, Wo = ops.stem_out_size(H, W, k)
        Hp, Wp = ops.pool_out_size(Ho, Wo)
        dy, dpool = rnd(B, Ho, Wo, N), rnd(B, Hp, Wp, N)
        put(f'operands {tag}', ['x', 'w', 'b', 'ws', 'bs', 'dy', 'dpool'], [x, w, b, ws, bs, dy, dpool])
        put(f'stem_conv_relu relu {tag}', ['y'], [ops.stem_conv_relu(x, w, b)])
        put(f'stem_conv_relu bare {tag}', ['y'], [ops.stem_conv_relu(x, w, b, relu=False)])
        put(f'stem_pool {tag}', ['y'], [ops.stem_pool(x, w, b)])
        am = torch.full((B, Hp, Wp, N), 77, dtype=torch.uint8, device='cuda')
        pooled = ops.stem_pool(x, w, b, argmax=am)
        put(f'stem_pool argmax {tag}', ['y', 'argmax'], [pooled, am])
        if k == 3:
            try:
                put(f'stem_pool_squeeze {tag}', ['y'], [ops.stem_pool_squeeze(x, w, b, ws, bs)])
                am2 = torch.full((B, Hp, Wp, N), 77, dtype=torch.uint8, device='cuda')
                ysq, yp = ops.stem_pool_squeeze(x, w, b, ws, bs, argmax=am2)
                put(f'stem_pool_squeeze argmax {tag}', ['y_sq', 'y_pooled', 'argmax'], [ysq, yp, am2])
            except ValueError as e:
                if W % 4 == 0:
                    raise
                res[f'stem_pool_squeeze {tag}'] = {'refused': [0, hashlib.sha256(str(e).encode()).hexdigest()]}
        put(f'stem_wgrad {tag}', ['dw', 'db'], ops.stem_wgrad(dy, x, N, k))
        put(f'stem_wgrad_pooled {tag}', ['dw', 'db'], ops.stem_wgrad_pooled(dpool, None, am, x, N, k))
        put(f'stem_wgrad_pooled pooled {tag}', ['dw', 'db'], ops.stem_wgrad_pooled(dpool, pooled, am, x, N, k))
        torch.cuda.synchronize()
    with open(path, 'w') as fh:
        json.dump(res, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--new-lib', default=os.path.join(ROOT, 'squeezedet-pytorch_amd', 'csrc', 'libsqdhip.so'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stem_refactor_bitwise.log'))
    ap.add_argument('--timeout', type=int, default=120, help='seconds per child')
    ap.add_argument('--dump', help='(child) run the cases from the library SQD_HIP_LIBRARY names and write their digests here')
    args = ap.parse_args()
    if args.dump:
        return child(args.dump)
    if not args.parent_lib:
        ap.error('--parent-lib is required')
    work = tempfile.mkdtemp(prefix='stem_bitwise_')
    lines, bad, ncases = [], 0, 0
    for ei, (ename, env) in enumerate(ENVS):
        dumps = {}
        for side, lib in (('parent', args.parent_lib), ('new', args.new_lib)):
            dumps[side] = os.path.join(work, f'{side}{ei}.json')
            child_env = {k: v for k, v in os.environ.items() if k not in ('SQD_STEM_WAVE', 'SQD_STEM_WGRAD_GATHER')}
            child_env.update(env, SQD_HIP_LIBRARY=os.path.abspath(lib))
            r = subprocess.run(['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--dump', dumps[side]],
                               env=child_env)
            if r.returncode != 0:
                print(f'{ename}: {side} library {lib}: the child ended with status {r.returncode}; nothing more is run')
                return 2
        old, new = (json.load(open(dumps[s])) for s in ('parent', 'new'))
        if list(old) != list(new):
            lines.append(f'[{ename}] the two children ran different case lists')
            bad += 1
        for case in old:
            same = case in new and old[case] == new[case]
            bad += not same
            ncases += not case.startswith('operands')
            outs = ' '.join(f'{n}[{v[0]}]' for n, v in old[case].items())
            lines.append(f'{"BYTE-EQUAL" if same else "DIFFERENT "}  [{ename}] {case}: {outs}')
    head = [f'parent library against this tree\'s ({os.path.relpath(args.new_lib, ROOT)}): {ncases} cases in {len(ENVS)} environments '
            f'({", ".join(e for e, _ in ENVS)}), outputs compared by the SHA-256 of their raw bytes (name[bytes]); {bad} differ']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(head + lines) + '\n')
    print('\n'.join(head + [l for l in lines if not l.startswith('BYTE-EQUAL')]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
