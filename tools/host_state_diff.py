#!/usr/bin/env python3
"""Do two builds of the host layer size a context alike?  Loads two hipemu test libraries (tests/emu_build.py of two trees) and prints, for a
grid of contexts, disco_owned_bytes / disco_workspace_bytes / disco_reference_workspace_bytes after disco_create (with and without
DISCO_FLAG_LAZY_SCRATCH), after disco_reserve(0 | 1 | 2), disco_set_tuning, every disco_set_option, and with the half-batch children
(overlap_solves = 2) -- a return code where a call fails.  The grid reaches every branch of reserve_scratch; nothing launches a kernel.
Every number must be equal.  Exit status 1 on any difference.  The sibling of tools/device_asm_diff.py.
Usage: tools/host_state_diff.py LIB_A LABEL_A LIB_B LABEL_B"""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from disco_amd import _lib  # noqa: E402

# (nodes, mics, n_fft): P2 <= 8; 9..16; 17..32 with M <= 8; M = 7 (float64 chunks); 1024 points with M > 6
SHAPES = [(4, 4, 512), (1, 4, 512), (2, 8, 512), (8, 8, 512), (12, 8, 512), (2, 7, 512), (3, 7, 1024), (2, 8, 1024)]
ROOMS = (1, 3, 1200)                     # 1200 x nodes >= 1024: the default overlap applies
OPTIONS = ('room_cov', 'solve_dpp', 'solve_thread', 'fuse_wide_istft', 'online_sq32', 'packed_x')
LENGTH = 16 * 256


def table(lib):
    rows = []

    def sizes(ctx):
        return (lib.disco_owned_bytes(ctx), lib.disco_workspace_bytes(ctx), lib.disco_reference_workspace_bytes(ctx))

    for K, M, n_fft in SHAPES:
        for R in ROOMS:
            for shard in ((False, True) if K > 1 and R == 3 else (False,)):
                for lazy in (0, 1):
                    def create():
                        cfg = _lib.DiscoCfg(rooms=R, nodes=K, mics=M, length=LENGTH, n_fft=n_fft, hop=n_fft // 2, flags=2 * lazy)
                        ctx = C.c_void_p()
                        assert lib.disco_create(C.byref(ctx), C.byref(cfg)) == 0, lib.disco_last_error(None)
                        if shard:
                            assert lib.disco_set_node_shard(ctx, 1, K - 1) == 0
                        return ctx
                    key = f'K{K} M{M} N{n_fft} R{R}{" shard" if shard else ""}{" lazy" if lazy else ""}'
                    for how in (0, 1, 2):
                        ctx = create()
                        rows.append((key, 'create') + sizes(ctx))
                        rows.append((key, f'reserve({how})', lib.disco_reserve(ctx, how)) + sizes(ctx))
                        lib.disco_destroy(ctx)
                    ctx = create()
                    t1 = (2, 10, 10, 4) if R < 1200 else (2, 3, 2, 4)      # (more chunks than the heuristic's: the blocks grow)
                    steps = [(f'set_tuning{t1}', lambda: lib.disco_set_tuning(ctx, *t1))]
                    steps += [(f'{k}=0', lambda k=k: lib.disco_set_option(ctx, k.encode(), 0)) for k in OPTIONS]
                    steps += [('overlap_solves=2', lambda: lib.disco_set_option(ctx, b'overlap_solves', 2)),
                              ('set_tuning(0,2,1,0)', lambda: lib.disco_set_tuning(ctx, 0, 2, 1, 0)),
                              ('room_cov=1', lambda: lib.disco_set_option(ctx, b'room_cov', 1)),
                              ('reserve(2)', lambda: lib.disco_reserve(ctx, 2)),
                              ('overlap_solves=0', lambda: lib.disco_set_option(ctx, b'overlap_solves', 0))]
                    for name, call in steps:
                        rows.append((key, name, call()) + sizes(ctx))
                    lib.disco_destroy(ctx)
    return ['  '.join(str(v) for v in row) for row in rows]


if __name__ == '__main__':
    lib_a, label_a, lib_b, label_b = sys.argv[1:5]
    ta, tb = (table(_lib.bind(C.CDLL(os.path.abspath(p)))) for p in (lib_a, lib_b))
    diff = [(a, b) for a, b in zip(ta, tb) if a != b]
    print(f'A: {label_a}\nB: {label_b}\ncontext, step[, return code], owned bytes, workspace bytes, reference workspace bytes (table of B):')
    print('\n'.join(tb))
    for a, b in diff[:20]:
        print(f'DIFFERS\n  A: {a}\n  B: {b}')
    print(f'{len(tb)} rows; sha1 of the table A {hashlib.sha1(chr(10).join(ta).encode()).hexdigest()}, B {hashlib.sha1(chr(10).join(tb).encode()).hexdigest()}')
    bad = len(diff) + abs(len(ta) - len(tb))
    print('identical' if not bad else f'{bad} rows differ')
    sys.exit(1 if bad else 0)
