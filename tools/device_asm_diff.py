#!/usr/bin/env python3
"""Do two source trees compile to the same device code?  Compiles every csrc/api_*.hip of both trees to device assembly (the flags of
disco_amd/build.py plus -S --cuda-device-only), drops the lines naming the per-compile __hip_cuid_ symbol and compares the rest as plain
text, unit by unit: `identical`, or the first differing line and the kernel (the last label before it) it sits in.  The listing carries
no source line numbers, so a change that only removes or moves text the front end discards leaves it byte-identical; nothing inside
the assembly is interpreted.  Exit status 1 on any difference.  The sibling of tools/kernel_set_diff.py, which compares resource usage.
Usage: tools/device_asm_diff.py TREE_A LABEL_A TREE_B LABEL_B [--out DIR]     (a label: the commit the tree is of; DIR keeps the listings)"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from disco_amd.build import FLAGS  # noqa: E402

JOBS = 16
LABEL = re.compile(r'^([A-Za-z_$][\w$.]*):')


def units(tree):
    csrc = os.path.join(tree, 'disco_amd', 'csrc')
    return {f[:-4]: os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.startswith('api_') and f.endswith('.hip')}


def listing(src, out):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    p = subprocess.run([hipcc] + FLAGS + ['-S', '--cuda-device-only', '-o', out, src], stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise RuntimeError(f'hipcc failed ({p.returncode}) on {src}')
    return [ln for ln in open(out) if '__hip_cuid_' not in ln]


def first_difference(a, b):
    """None, or (kernel, line number, line of A, line of B) of the first line that differs."""
    kernel = '(before the first label)'
    for i in range(max(len(a), len(b))):
        la, lb = (a[i] if i < len(a) else '<end>\n'), (b[i] if i < len(b) else '<end>\n')
        if la != lb:
            return kernel, i + 1, la.rstrip('\n'), lb.rstrip('\n')
        m = LABEL.match(la)
        if m:
            kernel = m.group(1)
    return None


if __name__ == '__main__':
    args = sys.argv[1:]
    keep = args.pop(args.index('--out') + 1) if '--out' in args else None
    tree_a, label_a, tree_b, label_b = [a for a in args if a != '--out'][:4]
    out = keep or tempfile.mkdtemp(prefix='device_asm_diff_')
    ua, ub = units(tree_a), units(tree_b)
    jobs = [(side, name, src) for side, us in (('a', ua), ('b', ub)) for name, src in us.items()]
    for side in 'ab':
        os.makedirs(os.path.join(out, side), exist_ok=True)
    with ThreadPoolExecutor(max_workers=JOBS) as ex:
        texts = dict(zip([(s, n) for s, n, _ in jobs], ex.map(lambda j: listing(j[2], os.path.join(out, j[0], j[1] + '.s')), jobs)))
    print(f'A: {label_a}: {len(ua)} units\nB: {label_b}: {len(ub)} units')
    print('compared: device assembly for gfx950 (' + ' '.join(FLAGS) + ' -S --cuda-device-only), lines naming __hip_cuid_ dropped')
    n_bad = 0
    for name in sorted(set(ua) | set(ub)):
        if name not in ua or name not in ub:
            print(f'{name}: only in {"A" if name in ua else "B"}')
            n_bad += 1
            continue
        d = first_difference(texts['a', name], texts['b', name])
        if d is None:
            print(f'{name}: identical ({len(texts["a", name])} lines)')
        else:
            print(f'{name}: DIFFERS in {d[0]}, line {d[1]}\n  A: {d[2]}\n  B: {d[3]}')
            n_bad += 1
    print('identical' if n_bad == 0 else f'{n_bad} of {len(set(ua) | set(ub))} units differ')
    sys.exit(0 if n_bad == 0 else 1)
