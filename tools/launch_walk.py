#!/usr/bin/env python3
"""Enqueue every branch of the BB unit's launchers once, at small shapes.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/launch_walk.py
    python tools/launch_walk.py --compare OLD_kernel_trace.csv NEW_kernel_trace.csv

One process; it checks nothing numerically.  Run under a kernel trace with two
builds of the library (BSLS_LIB), the traces must agree row for row in kernel
name, grid, workgroup and LDS bytes: a refactor of the host layer launches
what it launched before, in the same order.  --compare prints the row counts,
the unit's kernel templates seen and the verdict (exit status 1 on a
difference, or when one of the unit's kernels was never dispatched).

The problems are those of tests/test_gpu_row_weights.py (a 5 000-column
incidence in 250 blocks; K1 on tiles of 192 rows in 1 / 4 / 10 column groups
or on panels) at m = 500 and 501 rows, so bb_k1_sum runs in both widths.
After the BB unit the walk enqueues what else the host layer sequences, on
the same problem and the small x-space rig of tests/test_gpu_xbb_rounds.py:
BatchBB at R = 1, 3 and 8, DeviceLSQ on every image form, XBBEngine with and
without L-BFGS, IsoPlan.apply in both modes, and BBEngine.solve /
BatchBB.solve over poll windows that the record boundaries cut.
"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), ROOT, os.path.join(ROOT, 'block-simplex-least-squares_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

# the kernels of csrc/bb.hip's translation unit (the engine's and its tenants')
UNIT = ('bb_k1', 'bb_k1t', 'bb_k1_sum', 'bb_k1_init', 'bb_r_finish', 'bb_k2', 'bb_k2t',
        'bb_shard_record', 'bb_k3', 'bb_k3_long', 'bb_plus_one', 'bb_z2x',
        'ls_begin_kernel', 'ls_armijo_kernel', 'ls_curv_kernel', 'ls_finish_kernel',
        'dore_top', 'dore_mid', 'dore_ext', 'dore_sel', 'dore_copy')
OPTS = {'max_iter': 50, 'opt_tol': 1e-30}


def engine(m, form, sizes=None, options=OPTS, **kw):
    import test_gpu_row_weights as rw
    from device import BBEngine
    sh, b = rw.small(m)
    return BBEngine(sh['A'], b, sh['block_sizes'] if sizes is None else sizes, options=options,
                    **dict(rw.FORMS[form], **kw))


def run(eng, iters=2):
    """The prologue and `iters` iterations."""
    import torch
    eng.set_z0(torch.zeros(eng.nz, dtype=torch.float64))
    eng.prologue()
    eng.iterate(1, iters)
    torch.cuda.synchronize()


def walk():
    import numpy as np
    import torch
    import _native as N
    import test_gpu_row_weights as rw
    import DORE

    for m in (500, 501):
        # the plain forms: K1 on tiles with 1 / 4 / 10 groups and on panels
        for form in sorted(rw.FORMS):
            run(engine(m, form))
        # the thread-stream tiles and panels, every sum in a fixed order
        run(engine(m, 'tiles4', deterministic=True))
        run(engine(m, 'tiles1', deterministic=True))
        # fixed-point row sums with one and with several groups
        run(engine(m, 'tiles1', fixed_sums=True))
        run(engine(m, 'tiles4', fixed_sums=True))
        # row weights on panels, on one group and on several
        for form in ('panels', 'tiles1', 'tiles4', 'tiles10'):
            run(engine(m, form, row_weights=rw.mixed_weights(m)))
        # stored values (general A), dealt and thread-stream tiles and panels
        run(engine(m, 'tiles4', general=True))
        run(engine(m, 'tiles4', general=True, deterministic=True))
        run(engine(m, 'panels', general=True))

    m = 500
    sh, _ = rw.small(m)
    n = sh['A'].shape[1]
    # column scales exact in f16 (colv_codec 2), only in f32 (1), in neither (0):
    # dealt (K2 MODE 3) and thread-stream (MODE 2) tiles, and panels
    for colv, codec in ((np.full(n, 3.0), 2), (np.full(n, 1.0 + 2.0 ** -20), 1),
                        (np.full(n, 0.1), 0)):
        for kw in (dict(form='tiles4'), dict(form='tiles4', deterministic=True),
                   dict(form='panels')):
            eng = engine(m, colv=colv, **kw)
            assert eng.colv_codec == codec, (eng.colv_codec, codec)
            run(eng)
        os.environ['BSLS_K3_MERGE'] = '1'        # (two packs per wave at this codec too)
        run(engine(m, 'tiles4', colv=colv))
        del os.environ['BSLS_K3_MERGE']

    # K3: one and two packs per wave, and a block longer than a wave (bb_k3_long)
    for merge in ('0', '1'):
        os.environ['BSLS_K3_MERGE'] = merge
        run(engine(m, 'tiles4'))
    del os.environ['BSLS_K3_MERGE']
    sizes = np.asarray(sh['block_sizes'], dtype=np.int64)
    k = int(np.searchsorted(np.cumsum(sizes), 100)) + 1        # the first blocks as one of > 64
    long_sizes = np.concatenate(([sizes[:k].sum()], sizes[k:]))
    eng = engine(m, 'tiles4', sizes=long_sizes)
    assert eng.long_packs is not None
    run(eng)

    # a column shard's stages: the atomic K1 on several dealt groups (its init
    # alone and folded into K3), the r finishes, the fused K2 forms
    for role in (1, 2):
        for mm in (500, 501):
            eng = engine(mm, 'tiles4')
            eng.set_z0(torch.zeros(eng.nz, dtype=torch.float64))
            eng.prologue()
            eng.set_shard_role(role)
            eng.set_rr_slice(0, mm // 2)
            for stage, it in ((N.STAGE_RESET, 0), (N.STAGE_K1_PARTIAL, 0),
                              (N.STAGE_R_FINISH_TARGET, 0), (N.STAGE_R_FINISH, 0),
                              (N.STAGE_K2_RR_SLICE, 1), (N.STAGE_RECORD, 1),
                              (N.STAGE_K3_RECORD, 1), (N.STAGE_K1_PARTIAL, 1),
                              (N.STAGE_R_FINISH_TARGET, 1), (N.STAGE_K2_R_FINISH, 2),
                              (N.STAGE_K3, 2), (N.STAGE_K1_PARTIAL, 2), (N.STAGE_R_FINISH, 2),
                              (N.STAGE_K2_RR_SLICE, 3), (N.STAGE_K3_RECORD_INIT, 3),
                              (N.STAGE_K1_PARTIAL_INITED, 3), (N.STAGE_R_FINISH, 3)):
                eng.stage(stage, it)
            torch.cuda.synchronize()
    # the same stages without the atomics (one group; panels), and the atomic
    # K1 with its reduction on one GCD (BSLS_K1_ATOMIC=1)
    for form in ('tiles1', 'panels'):
        eng = engine(m, form)
        eng.set_z0(torch.zeros(eng.nz, dtype=torch.float64))
        eng.prologue()
        eng.set_shard_role(1)
        for stage, it in ((N.STAGE_K1_PARTIAL, 0), (N.STAGE_K2_RR_SLICE, 1),
                          (N.STAGE_K3_RECORD_INIT, 1), (N.STAGE_K1_PARTIAL_INITED, 1),
                          (N.STAGE_K2_R_FINISH, 2), (N.STAGE_K3, 2), (N.STAGE_K1_PARTIAL, 2)):
            eng.stage(stage, it)
        torch.cuda.synchronize()
    os.environ['BSLS_K1_ATOMIC'] = '1'
    run(engine(m, 'tiles4'))
    del os.environ['BSLS_K1_ATOMIC']

    # the link-part pipeline's pieces on a link_parts=2 engine
    for role in (1, 2):
        eng = engine(m, 'tiles4', link_parts=2)
        eng.set_z0(torch.zeros(eng.nz, dtype=torch.float64))
        eng.prologue()
        eng.set_shard_role(role)
        eng.set_rr_slice(0, m // 2)
        pb = [int(v) for v in eng.k1_part_bounds]
        for q in range(2):
            eng.residual_rows(0, pb[q], pb[q + 1])
        for q in range(2):
            eng.k2_part(1, q)
        eng.stage(N.STAGE_K3_RECORD_INIT, 1)
        for q in range(2):
            eng.k1_rows(1, pb[q], pb[q + 1])
        for q in range(2):
            eng.residual_rows(1, pb[q], pb[q + 1])
        torch.cuda.synchronize()

    # the tenants: two DORE steps and one line search, on fixed-order engines
    # (what the device decides along the way then repeats run to run)
    for form in ('tiles4', 'panels'):
        eng = engine(m, form, deterministic=True)
        DORE.solve_engine(eng, np.zeros(eng.nz), 1.0, eng.target, log=lambda i, x, t: 0.0,
                          options={'max_iter': 2})
        rs = np.random.RandomState(7)
        x = eng.proj(torch.from_numpy(rs.rand(eng.nz)).cuda())
        gx = eng.nabla_f(x)
        fx = torch.tensor([eng.f(x)], dtype=torch.float64, device='cuda')
        d = -gx / max(1.0, float(gx.abs().max()))
        eng.line_search().search(x, d.contiguous(), gx, fx)
        torch.cuda.synchronize()

    walk_host_layer()


def walk_host_layer():
    """What the host layer launches beside the BB unit: the batched engine,
    the x-space operator pair and engine, the isotonic plan, and the solve
    loops' poll windows."""
    import numpy as np
    import torch
    import test_gpu_row_weights as rw
    import test_gpu_xbb_rounds as xr
    from device import BatchBB, BlockLayout, DeviceLSQ

    m = 500
    sh, b = rw.small(m)

    def batch(R, weighted, options=OPTS):
        wts = [rw.mixed_weights(m) if weighted and j == 0 else None for j in range(R)]
        return BatchBB(sh['A'], [b * (1.0 + 0.125 * j) for j in range(R)], sh['block_sizes'],
                       row_weights=wts, options=options)

    # the batched engine at every interleave width, one problem weighted or none
    for R in (1, 3, 8):
        for weighted in (False, True):
            eng = batch(R, weighted)
            eng.set_z0(None)
            eng.prologue()
            eng.iterate(1, 2)
            torch.cuda.synchronize()

    # the x-space operator pair on each image form: one residual, one gradient
    A = xr.problem('Podd')[0].tocsr()
    for k1, k2 in (('panels', 'panels'), ('tiles', 'panels'), ('tiles_fixed', 'panels'),
                   ('panels', 'tiles'), ('tiles', 'tiles'), ('tiles_fixed', 'tiles')):
        op = DeviceLSQ(A, A.T.tocsr(), k1=k1, k2=k2)
        x = torch.full((op.n,), 0.5, dtype=torch.float64, device='cuda')
        r = torch.empty(op.m, dtype=torch.float64, device='cuda')
        g = torch.empty(op.n, dtype=torch.float64, device='cuda')
        sq = torch.zeros(1, dtype=torch.float64, device='cuda')
        op.residual(x, r, sq=sq)
        op.gradient(r, g)
        torch.cuda.synchronize()

    # the x-space engine: BB rounds and L-BFGS rounds (3 corrections)
    for C in (0, 3):
        R = xr.Rig('Podd', 'tiles_fixed', C=C)
        R.start(R.x_start, R.params())
        R.eng.rounds(2)
        R.eng.rounds(2)
        torch.cuda.synchronize()

    # the isotonic plan of the z-layout, bit-exact and prefix-sum
    lay = BlockLayout(sh['block_sizes'])
    y = torch.from_numpy(np.random.RandomState(11).rand(lay.nz)).cuda()
    for fast in (False, True):
        lay.iso_plan().apply(y.clone(), fast=fast)
    torch.cuda.synchronize()

    # the solve loops: windows of 2 cut at the record boundaries 3 and 6, then 7
    opts = {'max_iter': 7, 'opt_tol': 1e-30}
    engine(m, 'tiles4', options=opts, deterministic=True).solve(record_every=3, poll=2)
    batch(3, True, options=opts).solve(record_every=3, poll=2)
    torch.cuda.synchronize()


def trace_rows(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: (int(r['Start_Timestamp']), int(r['Dispatch_Id'])))
    cols = ('Kernel_Name', 'Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z', 'Workgroup_Size_X',
            'Workgroup_Size_Y', 'Workgroup_Size_Z', 'LDS_Block_Size')
    return [tuple(r[c] for c in cols) for r in rows]


def template_of(name):
    """bb_k1t of `void bsls::bb_k1t<1, true, ...>(...)`; None outside the unit."""
    words = name.replace('(anonymous namespace)::', '').split('(')[0].split('<')[0].split()
    base = words[-1].split('::')[-1] if words else None
    return base if base in UNIT else None


def compare(old, new):
    a, b = trace_rows(old), trace_rows(new)
    print('dispatches: old %d, new %d' % (len(a), len(b)))
    seen = sorted({t for t in (template_of(r[0]) for r in b) if t})
    unit_rows = sum(1 for r in b if template_of(r[0]))
    print('of the BB unit: %d dispatches of %d of its %d kernel templates'
          % (unit_rows, len(seen), len(UNIT)))
    print('distinct instantiations of the unit dispatched: %d'
          % len({r[0] for r in b if template_of(r[0])}))
    missing = [t for t in UNIT if t not in seen]
    if missing:
        print('never dispatched: ' + ', '.join(missing))
    diff = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
    for i in diff[:20]:
        print('row %d differs:\n  old %s\n  new %s' % (i, a[i], b[i]))
    ok = len(a) == len(b) and not diff and not missing
    print('verdict: %s' % ('the same launches in the same order (kernel name, grid, workgroup, '
                           'LDS bytes), row for row' if ok else 'DIFFERENT'))
    return 0 if ok else 1


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--compare', nargs=2, metavar=('OLD', 'NEW'))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    walk()
    print('launch walk done')
