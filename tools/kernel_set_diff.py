#!/usr/bin/env python3
"""Are two builds the same set of kernels?  Compares, over the whole library, the multiset of (mangled name, SGPRs, VGPRs, AGPRs,
scratch, occupancy, LDS) read from the .remarks files disco_amd/build.py leaves beside the objects -- whichever unit a kernel sits in.
Usage: tools/kernel_set_diff.py OBJ_DIR_A LABEL_A OBJ_DIR_B LABEL_B      (a label: the commit the build is of)"""
import collections
import os
import re
import sys

FIELDS = ('SGPRs', 'VGPRs', 'AGPRs', 'ScratchSize', 'Occupancy', 'LDS')
PAT = re.compile(r'remark: (?:.*?:\d+:\d+: )?\s*(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]|SGPRs): (\S+)')


def kernel_set(obj_dir):
    rows, cur = [], None
    for f in sorted(os.listdir(obj_dir)):
        if not f.endswith('.default.remarks'):
            continue
        for line in open(os.path.join(obj_dir, f)):
            m = PAT.search(line)
            if not m:
                continue
            k, v = m.group(1).split(' ')[0], m.group(2)
            if k == 'Function':
                cur = {'name': v}
                rows.append(cur)
            elif cur is not None:
                cur[k] = v
    return collections.Counter((r['name'],) + tuple(r.get(k, '?') for k in FIELDS) for r in rows)


if __name__ == '__main__':
    dir_a, label_a, dir_b, label_b = sys.argv[1:5]
    a, b = kernel_set(dir_a), kernel_set(dir_b)
    print(f'A: {label_a}: {sum(a.values())} kernels\nB: {label_b}: {sum(b.values())} kernels')
    print('compared: mangled name, ' + ', '.join(FIELDS))
    if a == b:
        print('identical')
    for tag, only in (('only in A', a - b), ('only in B', b - a)):
        for row, n in sorted(only.items()):
            print(f'{tag}: {" ".join(row)}' + (f' x{n}' if n > 1 else ''))
    sys.exit(0 if a == b else 1)
