#!/usr/bin/env python3
"""
Compare two gfx950 assembly listings of one source of pyremap_amd/csrc kernel
by kernel: what a refactor of the device code has to show.

    KERNEL_REGS=--keep python tools/kernel_regs.py      # writes /tmp/spmm.s
    python tools/kernel_diff.py parent.s new.s spmm_groupshare spmm_cellshare

The names given are the kernels the change touches (substrings of the
demangled name).  Every OTHER kernel must have the same normalised
instruction stream in both listings (comments, .p2align / .loc / .cfi lines
and .Ltmp labels removed, the function number dropped from .LBB<n>_<m>), and
the two sets of kernel symbols must be equal.  For each touched kernel the
registers, spills and scratch are printed side by side, and the number of
instructions per class that decides the speed of these kernels: memory and
LDS opcodes, s_barrier, each distinct s_waitcnt line, v_readlane_b32, float64
VALU -- in the whole kernel and inside the innermost loop around its
`ds_read_b64 ; s_barrier` (the step loop of the shared form, if it has one).

``--alias 'regex=replacement'`` rewrites demangled names of the FIRST listing
before pairing (a template parameter list that changed).  Exit status 1 if an
untouched kernel differs, a symbol is unpaired, a touched kernel spills or
loses waves per SIMD, or a listed class differs.
"""
import collections
import re
import sys

from kernel_regs import demangle

MEM = ('global_', 'buffer_', 'flat_', 'scratch_', 'ds_', 's_load')
META = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
        'private_segment_fixed_size')


def short(name):
    name = name.replace('remap::(anonymous namespace)::', '')
    return name.replace('void ', '', 1).split('(')[0]


def parse(path, aliases):
    """{demangled name: (normalised instruction lines, metadata dict)}"""
    text = open(path).read()
    bodies = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text,
                         re.M | re.S):
        lines = []
        for ln in m.group(2).split('\n'):
            ln = ln.split(';')[0].strip()
            if not ln or ln.startswith(('.p2align', '.loc', '.cfi', '.Ltmp')):
                continue
            lines.append(re.sub(r'\.LBB\d+_', '.LBB_', ln))
        bodies[m.group(1)] = lines
    names = re.findall(r'^\s+\.name:\s+(_Z\S+)$', text, re.M)
    meta = {k: re.findall(rf'^\s+\.{k}:\s+(\d+)$', text, re.M) for k in META}
    out = {}
    for i, (sym, dem) in enumerate(zip(names, demangle(names))):
        dem = short(dem)
        for pat, rep in aliases:
            dem = re.sub(pat, rep, dem)
        out[dem] = (bodies[sym], {k: int(meta[k][i]) for k in META})
    return out


def classes(lines):
    c = collections.Counter()
    for ln in lines:
        op = ln.split()[0]
        base = re.sub(r'_(e32|e64|dpp|sdwa)$', '', op)
        if op == 's_waitcnt':
            c[' '.join(ln.split())] += 1
        elif op.startswith(MEM) or op in ('s_barrier', 'v_readlane_b32') or \
                (base.startswith('v_') and base.endswith('_f64')):
            c[op] += 1
    return c


def step_loop(lines):
    """The innermost loop around the first `ds_read_b64 ; s_barrier`."""
    at = next((i for i in range(1, len(lines)) if lines[i] == 's_barrier' and
               lines[i - 1].startswith('ds_read_b64')), None)
    if at is None:
        return []
    label = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(':')}
    for i in range(at, len(lines)):
        w = lines[i].split()
        if w[0].startswith(('s_cbranch', 's_branch')) and \
                label.get(w[-1], len(lines)) <= at:
            return lines[label[w[-1]]:i + 1]
    return []


def waves(vgprs):
    return min(8, 512 // max((vgprs + 7) // 8 * 8, 8))


def n_instr(lines):
    return sum(1 for ln in lines if not ln.endswith(':'))


def main():
    args = sys.argv[1:]
    aliases = []
    while '--alias' in args:
        i = args.index('--alias')
        aliases.append(tuple(args[i + 1].split('=', 1)))
        del args[i:i + 2]
    old, new = parse(args[0], aliases), parse(args[1], [])
    touched = args[2:]
    bad = 0
    for n in sorted(set(old) ^ set(new)):
        print(f'UNPAIRED ({"parent" if n in old else "new"} only): {n}')
        bad += 1
    same = 0
    for n in sorted(set(old) & set(new)):
        (lo, mo), (ln, mn) = old[n], new[n]
        if not any(t in n for t in touched):
            if lo == ln:
                same += 1
            else:
                print(f'DIFFERS (untouched kernel): {n}')
                bad += 1
            continue
        print(f'{n}\n  instructions {n_instr(lo)} -> {n_instr(ln)}'
              + (' (identical stream)' if lo == ln else ''))
        for k in META:
            print(f'  {k:28s} {mo[k]:>4} -> {mn[k]:>4}')
        wo, wn = waves(mo['vgpr_count']), waves(mn['vgpr_count'])
        print(f'  {"waves/SIMD":28s} {wo:>4} -> {wn:>4}')
        if wn < wo or any(mn[k] for k in META[2:]):
            print('  FAIL: occupancy lost, spill or scratch')
            bad += 1
        for what, a, b in (('kernel', lo, ln),
                           ('step loop', step_loop(lo), step_loop(ln))):
            ca, cb = classes(a), classes(b)
            diff = [k for k in sorted(set(ca) | set(cb)) if ca[k] != cb[k]]
            print(f'  {what}: {sum(ca.values())} instructions in the listed '
                  f'classes of {n_instr(a)} -> {sum(cb.values())} of '
                  f'{n_instr(b)}' + ('' if diff else ', every class equal'))
            for k in diff:
                print(f'    FAIL {k}: {ca[k]} -> {cb[k]}')
            bad += len(diff)
    print(f'{same} untouched kernels identical; '
          f'{"OK" if not bad else f"{bad} finding(s)"}')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
