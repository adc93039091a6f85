#!/usr/bin/env python
"""Per-phase times of the fused BB iteration's kernels, from a library built
with -DBSLS_PHASE_STAMPS (csrc/bb.hip: wave 0 of every workgroup of bb_k2t,
bb_k3, bb_k1t and bb_k1_sum keeps s_memrealtime, 100 MHz, at its phase
boundaries).

    make -C block-simplex-least-squares_amd/csrc VAR=_ph DEFS=-DBSLS_PHASE_STAMPS
    BSLS_LIB=.../lib/libbsls_hip_ph.so python tools/phase_times.py [--iters 200]

Builds C3, runs 20 warm iterations, then `--iters` iterations one
bsls_bb_iterate call each, reading the stamps after each.  Per kernel it
prints, for every phase, the median over iterations of (a) the median over
workgroups of the phase's span inside a workgroup and (b) the time from the
kernel's first entry stamp to the workgroups' median / last stamp of the
phase's end.  The stamp buffer holds the first 4096 workgroups of a launch
(bb_k3 at C3 launches 4.2k: the later ones are not in its figures, and the
output says how many were read).  Slot 2 of the walks is taken where the LDS
clear starts: the dealt walk's first loads are issued by then (tiles.hpp
tile_walk_dealt).  The stamps cost a few scalar instructions each; the build's
iteration is timed against nothing here -- the figures attribute, they do not
benchmark.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'block-simplex-least-squares_amd'))

import numpy as np  # noqa: E402

KERNELS = ['bb_k2t', 'bb_k3', 'bb_k1t', 'bb_k1_sum']
# slot -> what has happened when the stamp is taken
PHASES = {
    'bb_k2t': ['entry', 'stop flag read', 'LDS clear starts (walk prefilled)', 'LDS clear + barrier',
               'walk end (wave 0)', 'barrier (all waves)', 'epilogue end', 'reduction tail'],
    'bb_k1t': ['entry', 'stop flag read', 'LDS clear starts (walk prefilled)', 'LDS clear + barrier',
               'walk end (wave 0)', 'barrier (all waves)', 'partials stored'],
    'bb_k3': ['entry', 'step t known', 'z, g landed', 'PAVA done', 'stores issued'],
    'bb_k1_sum': ['entry', 'stop flag read (first loads issued)', 'rows stored',
                  'reduction tail'],
}
TICK_US = 0.01   # s_memrealtime: 100 MHz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--config', default='C3')
    args = ap.parse_args()
    import torch
    import _native
    from synthetic import make_shard, add_noise, CONFIGS, SEED
    from device import BBEngine
    L = _native.lib()
    if not hasattr(L, 'bsls_phase_read'):
        sys.exit('phase_times: %s was not built with -DBSLS_PHASE_STAMPS' % _native.LIB_PATH)
    shape = (ctypes.c_int * 3)()
    L.bsls_phase_shape(shape)
    shape = tuple(shape)
    L.bsls_phase_read.restype = ctypes.c_int
    L.bsls_phase_read.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    c = CONFIGS[args.config]
    sh = make_shard(c['n'], c['p'], c['m'], c['per_col'], seed=SEED)
    b = add_noise(sh['Ax'], 0.02, seed=SEED)
    eng = BBEngine(sh['A'], b, sh['block_sizes'], options={'max_iter': 10 ** 9, 'opt_tol': 1e-30},
                   AT=sh['AT'], colv=sh.get('colv'))
    eng.set_z0(torch.zeros(eng.nz, dtype=torch.float64))
    eng.prologue()
    eng.iterate(1, 20)
    torch.cuda.synchronize()
    buf = np.zeros(shape, dtype=np.uint64)
    span = {k: [] for k in KERNELS}     # per iteration: median over workgroups of each span
    med_at = {k: [] for k in KERNELS}   # ... of each stamp since the kernel's first entry
    last_at = {k: [] for k in KERNELS}  # ... the last workgroup's
    nwg = {k: 0 for k in KERNELS}
    for it in range(21, 21 + args.iters):
        buf[:] = 0
        eng.iterate(it, 1)
        torch.cuda.synchronize()
        _native.check(L.bsls_phase_read(buf.ctypes.data, buf.size), 'bsls_phase_read')
        for ki, k in enumerate(KERNELS):
            ns = len(PHASES[k])
            t = buf[ki][:, :ns].astype(np.int64)
            t = t[(t[:, 0] > 0) & (t[:, ns - 1] > 0)]     # workgroups that ran every phase
            nwg[k] = len(t)
            if not len(t):
                continue
            rel = (t - t[:, :1].min()) * TICK_US
            span[k].append(np.median(np.diff(t, axis=1), axis=0) * TICK_US)
            med_at[k].append(np.median(rel, axis=0))
            last_at[k].append(rel.max(axis=0))
    print('%s, %d iterations, early_exit on; times in us (stamp resolution %.2f)'
          % (args.config, args.iters, TICK_US))
    for k in KERNELS:
        if not span[k]:
            print('%s: no stamps' % k)
            continue
        sp = np.median(np.array(span[k]), axis=0)
        ma = np.median(np.array(med_at[k]), axis=0)
        la = np.median(np.array(last_at[k]), axis=0)
        print('%s (%d workgroups stamped in the last iteration; the buffer holds %d)'
              % (k, nwg[k], shape[1]))
        print('  %-38s %10s %14s %12s' % ('phase ends with', 'span in WG', 'median WG at', 'last WG at'))
        for s, name in enumerate(PHASES[k]):
            print('  %-38s %10s %14.2f %12.2f'
                  % (name, '%.2f' % sp[s - 1] if s else '-', ma[s], la[s]))


if __name__ == '__main__':
    main()
