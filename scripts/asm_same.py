#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  Compares assembly files (hipcc -S --cuda-device-only; the Makefile's asm*
targets) pairwise: the sets of .amdhsa_kernel names must be equal, and for every kernel the .amdhsa_kernel .. .end_amdhsa_kernel
block and the text from its label to its .Lfunc_end must be equal once the labels that depend on the ORDER in which the
functions were emitted are normalised (.LBB<n>_, .Lfunc_end<n>, .LJTI<n>_ lose the function's number; .Ltmp<n> are renumbered
by first appearance inside the kernel).
Usage: asm_same.py parent_dir branch_dir file.s [file.s ...]    (exit status 1 when anything differs)"""
import os
import re
import sys


def kernels(path):
    """name -> (normalised code, descriptor block) of every kernel in the file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel', text, re.M | re.S):
        name = m.group(1)
        a = re.search(r'^%s:' % re.escape(name), text, re.M).start()
        b = re.compile(r'^\.Lfunc_end\d+:', re.M).search(text, a).start()
        code = re.sub(r'\.(LBB|LJTI|Lfunc_end|Lfunc_begin)\d+', r'.\1', text[a:b])
        code = re.sub(r'\bBB\d+_', 'BB_', code)                 # (the loop comments name blocks without the .L ...
        code = re.sub(r'[ \t]+;', ' ;', code)                   # ... and stand at a column that follows the label's width)
        tmp = {}
        code = re.sub(r'\.Ltmp(\d+)', lambda t: '.Ltmp#%d' % tmp.setdefault(t.group(1), len(tmp)), code)
        out[name] = (code, m.group(0))
    return out


def main():
    parent, branch, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    for f in files:
        p, b = kernels(os.path.join(parent, f)), kernels(os.path.join(branch, f))
        only_p, only_b = sorted(set(p) - set(b)), sorted(set(b) - set(p))
        differ = sorted(n for n in set(p) & set(b) if p[n] != b[n])
        fam = lambda stem: sum(1 for n in b if re.match(r'_Z\d+%sI' % stem, n))
        print('%-20s kernels %3d / %3d (k_sweep %d, k_events %d, k_resident %d)  only in parent %d  only in branch %d  differing %d'
              % (f, len(p), len(b), fam('k_sweep'), fam('k_events'), fam('k_resident'), len(only_p), len(only_b), len(differ)))
        for n in only_p: print('    only in parent: ' + n)
        for n in only_b: print('    only in branch: ' + n)
        for n in differ: print('    differs: %s (%s)' % (n, 'code' if p[n][0] != b[n][0] else 'descriptor'))
        bad += len(only_p) + len(only_b) + len(differ)
    print('SAME' if not bad else 'DIFFERENT: %d' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
