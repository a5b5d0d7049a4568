#!/usr/bin/env python3
"""Which functions of two hipcc -S listings of the same source are the same code (refactoring aid).

  python tools/isa_identity.py parent.s new.s [name-substring ...]
Listings: hipcc <FLAGS of dafs_amd/build.py> --cuda-device-only -S file.hip.  A function is the text from its label to its
.Lfunc_end, comments stripped and local labels (.LBB..., .Ltmp..., .Lfunc_...) renumbered in order of appearance.  With
name substrings, only the functions that contain one of them are listed, and the exit status is 1 when one of those differs.
"""
import re
import sys


def funcs(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur:
            if ln.startswith('.Lfunc_end'):
                cur = None
                continue
            t = ln.split(';')[0].rstrip()
            if t.strip():
                out[cur].append(t)
    return out


def norm(lines):
    ids = {}
    return [re.sub(r'\.L(BB|tmp|func_)\w*', lambda m: ids.setdefault(m.group(0), '.L%d' % len(ids)), l) for l in lines]


a, b = funcs(sys.argv[1]), funcs(sys.argv[2])
sel = sys.argv[3:]
bad = 0
for k in a:
    if sel and not any(s in k for s in sel):
        continue
    same = norm(a[k]) == norm(b.get(k, []))
    bad += (not same) and bool(sel)
    print('%-8s %6d %s' % ('same' if same else 'DIFFERS', len(a[k]), k))
sys.exit(1 if bad else 0)
