#!/usr/bin/env python3
"""Is the device code of two checkouts the same?  Compiles the named csrc/*.hip of both with each checkout's own Makefile flags
plus `--cuda-device-only -S` and compares the gfx950 assembly text function by function - the proof a refactor that only moves
source text owes: identical instruction streams need no benchmark.

    python tools/device_asm_diff.py <old checkout> <new checkout> gn.hip fbp.hip      # named files (default: all of the old one)
    python tools/device_asm_diff.py --md <old> <new> gn_multi.hip                      # a markdown table

Lines containing `__hip_cuid` are dropped: that symbol is a hash of the source text, the one thing that differs when code only
moves; so is the ordinal a function's local labels carry (its position in the file: removing one instantiation renumbers every
function behind it).  Everything else - instructions, kernel descriptors, metadata - is compared as whole text.  Exit status 1 if anything
differs.
"""
import difflib
import os
import re
import subprocess
import sys

CSRC = os.path.join('dex-ct-sim_amd', 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def makefile_flags(root):
    """HIPFLAGS of the checkout's Makefile, $(ARCH) filled in."""
    text = open(os.path.join(root, CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    return re.search(r'^HIPFLAGS\s*\?=\s*(.*)$', text, re.M).group(1).replace('$(ARCH)', arch).split()


def assembly(root, src):
    p = subprocess.run([HIPCC, *makefile_flags(root), '--cuda-device-only', '-S', '-o', '-', src],
                       cwd=os.path.join(root, CSRC), capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f'{root}: {src}\n{p.stderr[-3000:]}')
    return [l for l in p.stdout.splitlines() if '__hip_cuid' not in l]


# local labels carry the ordinal of their function in the file (.LBB35_12, .Lfunc_end35, "Header=BB35_1"): it changes for every
# function behind one that was added or removed, and it says nothing about the function itself
_ORDINAL = re.compile(r'(?<![A-Za-z0-9_])((?:\.L)?(?:BB|func_begin|func_end))\d+')


def sections(lines):
    """{name: lines}: the text before the first function, every function from the directives that open its section (those
    that name it, in front of its `.type name,@function` line) to the next one's (its kernel descriptor included), and the
    metadata note at the end.  Function ordinals in local labels are blanked."""
    out, name = {'(preamble)': []}, '(preamble)'
    for l in lines:
        m = re.match(r'\s*\.type\s+([^,\s]+),@function', l)
        if m:
            prev, k = out[name], len(out[name])
            while k > 0 and (m.group(1) in prev[k - 1] or re.match(r'\s*\.p2align', prev[k - 1])):
                k -= 1
            name, head = m.group(1), prev[k:]
            del prev[k:]
            out.setdefault(name, []).extend(head)
        elif re.match(r'\s*\.amdgpu_metadata', l):
            name = '(metadata)'
        l = _ORDINAL.sub(r'\1#', l)
        if l.startswith('.LBB'):       # a label line: the column of its comment moves with the number of digits
            l = re.sub(r':\s+;', ': ;', l, count=1)
        out.setdefault(name, []).append(l)
    return out


def demangle(names):
    try:
        out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.splitlines()
    except OSError:
        return dict(zip(names, names))
    short = [n if n.startswith('(') else re.sub(r'^(void )?dexct::', '', n.replace('(anonymous namespace)::', '')).split('(')[0]
             for n in out]
    return dict(zip(names, short))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    md = '--md' in sys.argv
    if len(args) < 2:
        raise SystemExit(__doc__)
    old, new = args[0], args[1]
    files = args[2:] or sorted(f for f in os.listdir(os.path.join(old, CSRC)) if f.endswith('.hip'))
    if md:
        print('| file | function | lines | device code |\n|---|---|---|---|')
    differs = False
    for f in files:
        a, b = sections(assembly(old, f)), sections(assembly(new, f))
        names = demangle([n for n in list(a) + [n for n in b if n not in a]])
        for n, shown in names.items():
            la, lb = a.get(n), b.get(n)
            if la == lb:
                verdict, detail = 'identical', []
            elif la is None or lb is None:
                verdict, detail = ('only in new' if la is None else 'only in old'), []
            else:
                detail = [l for l in difflib.unified_diff(la, lb, 'old', 'new', n=0, lineterm='')][2:14]
                verdict = f'DIFFERS ({len(la)} -> {len(lb)} lines)'
            differs = differs or verdict != 'identical'
            if md:
                print(f'| `{f}` | `{shown}` | {len(la or lb)} | {verdict} |')
            else:
                print(f'{f}: {shown}: {verdict}')
            for l in ([] if md else detail):
                print('    ' + l)
    return 1 if differs else 0


if __name__ == '__main__':
    sys.exit(main())
