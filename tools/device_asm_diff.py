"""Is the gfx950 device code of two source trees the same, kernel by kernel?  Needs no GPU.

usage: python tools/device_asm_diff.py OLD_CSRC NEW_CSRC [--work DIR] [--jobs N] [--map OLD_SUBSTR=NEW_SUBSTR ...]

Every file of each side's Makefile SRCS is compiled with the flags that Makefile gives that file, plus
--cuda-device-only -S.  The listings are split by kernel symbol; basic-block label numbers (BB<n>_ -> BB_), comments and
whitespace are normalised; then the kernel symbol sets, each kernel's instruction text and each kernel's .amdhsa_kernel
descriptor (registers, LDS, scratch) are compared.  A kernel is paired by its symbol wherever it lives: one that moved to another
file is compared across files and reported under the file that holds it now.  --map pairs a renamed symbol (a template parameter
that went away changes the mangled name): the substring is replaced in the old side's symbols and text before the comparison.
Prints one line per file and every difference -- for a kernel that differs also its instruction count, its vector-memory
instructions (all, and the 16-byte loads / stores) and its VGPR / LDS / scratch figures, before -> after; exit status 1 if any
kernel differs or exists on one side only (a refactor lists the instantiations it removed on purpose)."""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def srcs(csrc):
    for line in open(os.path.join(csrc, 'Makefile')):
        if line.startswith('SRCS'):
            return line.split('=', 1)[1].split()
    raise SystemExit(f'no SRCS in {csrc}/Makefile')


def compile_cmd(csrc, src):
    """the hipcc line `make` would run for src, up to its -c"""
    obj = src.replace('.hip', '.o')
    out = subprocess.run(['make', '-C', csrc, '-n', '-B', obj], capture_output=True, text=True, check=True).stdout
    line = next(l for l in out.splitlines() if 'hipcc' in l and f' {src} ' in l)
    toks = shlex.split(line.split(' 2>')[0])
    return toks[:toks.index('-c')]


def listing(csrc, src, work):
    dst = os.path.join(work, src.replace('.hip', '.s'))
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(('.hip', '.h')) or f == 'Makefile']
    if os.path.exists(dst) and os.path.getmtime(dst) > max(os.path.getmtime(d) for d in deps):
        return dst
    r = subprocess.run(compile_cmd(csrc, src) + ['--cuda-device-only', '-S', src, '-o', os.path.abspath(dst)], cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(f'{csrc}/{src}: {r.stderr[-2000:]}')
    return dst


def norm(line):
    line = line.split(';', 1)[0]
    line = re.sub(r'BB\d+_', 'BB_', line)
    return ' '.join(line.split())


def kernels(path):
    """{symbol: (instruction text, descriptor text)}"""
    lines = open(path).read().splitlines()
    desc, cur = {}, None
    for l in lines:
        s = l.strip()
        if s.startswith('.amdhsa_kernel '):
            cur = s.split()[1]
            desc[cur] = []
        elif s == '.end_amdhsa_kernel':
            cur = None
        elif cur is not None:
            desc[cur].append(norm(s))
    body, cur, in_desc = {}, None, False
    for l in lines:
        s = l.strip()
        if s.startswith('.amdhsa_kernel ') or s == '.end_amdhsa_kernel':      # (the descriptor may sit before the function's end label)
            in_desc = s != '.end_amdhsa_kernel'
        elif in_desc:
            pass
        elif cur is None:
            m = re.match(r'(\S+):', s)                 # "symbol:   ; @symbol"
            if m and m.group(1) in desc:
                cur = m.group(1)
                body[cur] = []
        elif re.match(r'\.Lfunc_end\d+:', s):
            cur = None
        else:
            n = norm(s)
            if n:
                body[cur].append(n)
    empty = [k for k in desc if not body.get(k)]
    if empty:
        raise SystemExit(f'{path}: no instructions found for {empty[:3]} ...: the listing format is not the one this script reads')
    return {k: ('\n'.join(body[k]), '\n'.join(desc[k])) for k in desc}


WATCHED = ('global_load_dwordx4', 'global_store_dwordx4', 'flat_load_dwordx4', 'flat_store_dwordx4')
VMEM = ('buffer_', 'global_', 'flat_', 'scratch_')          # every vector-memory instruction (what s_waitcnt vmcnt counts)
RESOURCES = ('.amdhsa_next_free_vgpr', '.amdhsa_accum_offset', '.amdhsa_group_segment_fixed_size', '.amdhsa_private_segment_fixed_size')


def counts(text):
    """instructions (labels and directives left out) and the 16-byte vector memory instructions of one kernel's text"""
    ins = [l.split()[0] for l in text.splitlines() if not l.endswith(':') and not l.startswith('.')]
    return [len(ins), sum(i.startswith(VMEM) for i in ins)] + [ins.count(w) for w in WATCHED]


def resources(desc):
    got = dict(l.split()[:2] for l in desc.splitlines() if l.split()[0] in RESOURCES)
    return [got.get(r, '-') for r in RESOURCES]


def demangle(names):
    if not names:
        return []
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else list(names)


def renamed(text, maps):
    for old, new in maps:
        text = text.replace(old, new)
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--work', default=None, help='keeps the listings (old/ and new/) for reuse')
    ap.add_argument('--jobs', type=int, default=4)
    ap.add_argument('--map', action='append', default=[], metavar='OLD_SUBSTR=NEW_SUBSTR',
                    help='pair a renamed symbol: the substring is replaced in the old side\'s (mangled) symbols and text; repeatable')
    a = ap.parse_args()
    maps = [tuple(m.split('=', 1)) for m in a.map]
    work = a.work or tempfile.mkdtemp(prefix='device_asm_diff_')
    sides = {'old': (a.old, srcs(a.old)), 'new': (a.new, srcs(a.new))}
    if sides['old'][1] != sides['new'][1]:
        print(f'SRCS differ: only before {sorted(set(sides["old"][1]) - set(sides["new"][1]))}, only after '
              f'{sorted(set(sides["new"][1]) - set(sides["old"][1]))}: a kernel is looked for in every file of the other side')
    for side in sides:
        os.makedirs(os.path.join(work, side), exist_ok=True)
    jobs = [(side, csrc, f) for side, (csrc, fs) in sides.items() for f in fs]
    with ThreadPoolExecutor(a.jobs) as ex:
        paths = dict(zip([(s, f) for s, _, f in jobs], ex.map(lambda j: listing(j[1], j[2], os.path.join(work, j[0])), jobs)))
    per = {(s, f): kernels(p) for (s, f), p in paths.items()}
    per.update({('old', f): {renamed(k, maps): (renamed(t, maps), d) for k, (t, d) in per[('old', f)].items()} for f in sides['old'][1]})
    home = {s: {k: f for f in fs for k in per[(s, f)]} for s, (_, fs) in sides.items()}      # symbol -> its file
    bad = total = 0
    for f in sorted(set(sides['old'][1]) | set(sides['new'][1]), key=(sides['old'][1] + sides['new'][1]).index):
        # a file's kernels: those it holds on either side; one that moved is compared where it lives now and reported there
        ko = {k: per[('old', home['old'][k])][k] for k in home['old'] if home['new'].get(k, home['old'][k]) == f}
        kn = per.get(('new', f), {})
        moved = sorted(k for k in ko if home['old'][k] != f)
        gone, added = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
        text = [k for k in sorted(set(ko) & set(kn)) if ko[k][0] != kn[k][0]]
        dsc = [k for k in sorted(set(ko) & set(kn)) if ko[k][1] != kn[k][1]]
        same = len(set(ko) & set(kn)) - len(set(text) | set(dsc))
        print(f'{f}: {len(ko)} kernels before, {len(kn)} after, {same} identical (text and descriptor), '
              f'{len(gone)} removed, {len(added)} added, {len(text)} text differs, {len(dsc)} descriptor differs'
              + (f', {len(moved)} came from another file' if moved else ''))
        for k, name in zip(moved, demangle(moved)):
            print(f'    moved from {home["old"][k]}: {name}')
        for tag, ks in (('removed', gone), ('added', added), ('TEXT DIFFERS', text), ('DESCRIPTOR DIFFERS', dsc)):
            for k in demangle(ks):
                print(f'    {tag}: {k}')
        for k, name in zip(sorted(set(text) | set(dsc)), demangle(sorted(set(text) | set(dsc)))):
            o, n = counts(ko[k][0]), counts(kn[k][0])
            print(f'    counts: {name}: ' + ', '.join(f'{w} {a} -> {b}' for w, a, b in zip(('instructions', 'vector-memory') + WATCHED, o, n)) + '; '
                  + ', '.join(f'{r[8:]} {a} -> {b}' for r, a, b in zip(RESOURCES, resources(ko[k][1]), resources(kn[k][1]))))
        bad += len(gone) + len(added) + len(set(text) | set(dsc))
        total += len(ko)
    print(f'total: {total} kernels before; {bad} removed, added or different')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
