"""What the link metrics cost on the device (bsls_link_metrics, csrc/metrics.hip)
against a torch-on-device restatement of the same table, and what
metrics=True adds to a 5-fold cross-validation.

  python tools/link_metrics_time.py [--out FILE] [--config C3] [--skip-kfold]

The config's m rows (C3: 100 000), 6 link classes by flow (7 edges), one mask
(every fifth row held out), nstates 1 and 8.  The restatement is what a user
of the engine without this kernel would write with torch on the device:
elementwise GEH, torch.bucketize for the classes, index_add_ for the sums per
cell and scatter_reduce_ for the max.  Each side is warmed up, then ten windows
of CALLS calls between device synchronises, the two sides alternated window by
window in one process; the median window is reported with the spread.  The two
tables are compared once before anything is timed.

Then cross_validation.kfold(k=5) on one engine of the config, max_iter 500,
with metrics=False and metrics=True alternated five times: the median wall
time of each."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'block-simplex-least-squares_amd')
sys.path[:0] = [ROOT, PKG]

CALLS, WINDOWS, WARMUP = 50, 10, 5
KFOLD_ITERS, KFOLD_REPEATS = 500, 5


def median(v):
    v = sorted(v)
    return 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]) if len(v) % 2 == 0 else v[len(v) // 2]


def torch_table(torch, ax, b, w, edges):
    """[state][set][class][9] with torch ops on the device."""
    ns, m = ax.shape
    ncls = edges.numel() + 1
    diff, plus = ax - b, ax + b
    d2 = diff * diff
    geh = torch.sqrt(2 * d2 / plus)
    cell = (w == 0).long() * ncls + torch.bucketize(b, edges, right=True)
    one = torch.ones_like(geh)
    vals = torch.stack([one, d2, geh, (geh < 5).double(), (geh < 1).double(),
                        (geh < 0.5).double(), (geh < 0.05).double(), b.expand(ns, m)], dim=1)
    sums = torch.zeros(ns, 8, 2 * ncls, dtype=torch.float64, device=ax.device)
    sums.index_add_(2, cell, vals)
    mx = torch.zeros(ns, 2 * ncls, dtype=torch.float64, device=ax.device)
    mx.scatter_reduce_(1, cell.expand(ns, m), geh, 'amax')
    out = torch.cat([sums[:, :3], mx[:, None], sums[:, 3:]], dim=1)      # the kernel's value order
    return out.permute(0, 2, 1).reshape(ns, 2, ncls, 9)


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'link_metrics_C3.txt'))
    ap.add_argument('--config', default='C3')
    ap.add_argument('--skip-kfold', action='store_true')
    a = ap.parse_args()
    import numpy as np
    import torch
    import _native
    import synthetic
    from dev_metrics import link_classes
    if not torch.cuda.is_available():
        raise SystemExit('link_metrics_time needs a HIP device: nothing is timed without one')
    L = _native.lib()
    sh = synthetic.make_problem(a.config)
    b_h = np.ascontiguousarray(sh['b'], dtype=np.float64)
    m = b_h.size
    edges_h = link_classes(b_h, 6)
    rs = np.random.RandomState(29)
    f64 = dict(dtype=torch.float64, device='cuda')
    b = torch.from_numpy(b_h).cuda()
    w = torch.from_numpy((np.arange(m) % 5 != 0).astype(np.float64)).cuda()
    edges = torch.from_numpy(edges_h).cuda()
    ne = edges_h.size
    lines = ['# %s: m = %d rows, %d classes (%d edges), one mask, one MI355X; %d warm-up calls, '
             'then %d windows of %d calls,' % (a.config, m, ne - 1, ne, WARMUP, WINDOWS, CALLS),
             '# kernel and torch restatement alternated window by window in one process; median '
             'window (tools/link_metrics_time.py)',
             '# nstates   bsls_link_metrics us/call (min .. max)   torch us/call (min .. max)   '
             'torch / kernel   kernel GB/s   max |table difference| / max(1, |.|)']
    for ns in (1, 8):
        ax = torch.from_numpy(np.abs(b_h * (1 + 0.05 * rs.randn(ns, m)))).cuda()
        out = torch.empty(ns * 2 * (ne + 1) * 9, **f64)
        work = torch.empty(L.bsls_link_metrics_work_size(m, ns, ne), dtype=torch.uint8,
                           device='cuda')
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        st = _native.stream_handle()

        def kernel():
            _native.check(L.bsls_link_metrics(vp(ax), m, vp(b), vp(w), 0, vp(edges), ne, m, ns,
                                              vp(out), vp(work), st), 'bsls_link_metrics')

        def restated():
            return torch_table(torch, ax, b, w, edges)
        kernel()
        ref = restated().reshape(-1)
        torch.cuda.synchronize()
        diff = float(((out - ref).abs() / ref.abs().clamp(min=1.0)).max().item())
        sides = {'kernel': kernel, 'torch': restated}
        for fn in sides.values():
            for _ in range(WARMUP):
                fn()
        times = {k: [] for k in sides}
        for _ in range(WINDOWS):
            for name, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(CALLS):
                    fn()
                torch.cuda.synchronize()
                times[name].append(1e6 * (time.perf_counter() - t0) / CALLS)
        k, t = median(times['kernel']), median(times['torch'])
        gbs = (ns * m * 24 + work.numel()) / (k * 1e-6) / 1e9     # ax, b and w per state; the partials
        lines.append('%-9d %10.1f (%.1f .. %.1f) %24.1f (%.1f .. %.1f) %12.1f %14.1f %18.1e'
                     % (ns, k, min(times['kernel']), max(times['kernel']), t, min(times['torch']),
                        max(times['torch']), t / k, gbs, diff))
    if not a.skip_kfold:
        from cross_validation import kfold
        from bsls_utils import particular_x0
        from main import build_engine
        A, sizes = sh['A'], np.asarray(sh['block_sizes'])
        x0 = particular_x0(sizes)
        opts = {'max_iter': KFOLD_ITERS, 'opt_tol': 1e-30}
        eng = build_engine(A, b_h, x0, sizes, options=opts, row_weights=np.ones(m))
        kfold(A, b_h, x0, None, sizes, 5, options=opts, engine=eng, metrics=True)    # warm-up
        wall = {False: [], True: []}
        for _ in range(KFOLD_REPEATS):
            for flag in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kfold(A, b_h, x0, None, sizes, 5, options=opts, engine=eng, metrics=flag)
                torch.cuda.synchronize()
                wall[flag].append(time.perf_counter() - t0)
        off, on = median(wall[False]), median(wall[True])
        lines += ['',
                  '# cross_validation.kfold(k=5) on one engine, %d iterations a fold, metrics=False '
                  'and metrics=True alternated %d times; median wall time'
                  % (KFOLD_ITERS, KFOLD_REPEATS),
                  '# metrics=False   %.4f s (%.4f .. %.4f)' % (off, min(wall[False]),
                                                              max(wall[False])),
                  '# metrics=True    %.4f s (%.4f .. %.4f)' % (on, min(wall[True]), max(wall[True])),
                  '# metrics add     %.2f %%' % (100.0 * (on - off) / off)]
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main_()
