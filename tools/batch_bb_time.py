"""What a BB iteration costs per problem when R problems run in lockstep
(device.BatchBB, csrc/bbm.hip), against the fused single-problem engine.

  python tools/batch_bb_time.py [--out FILE] [--config C3] [--widths 1,2,4,8]

C3 (synthetic.make_problem), early exits off, one process: for each engine 20
warm-up iterations, then ten windows of 200 iterations, each window between
device synchronises; the median window is reported, with the spread.  The
engines are timed alternately (BatchBB at every width, then the default
BBEngine, window by window), so drift in the machine falls on all of them
alike.  The default BBEngine is the parent commit's code path unchanged.
--profile-only R runs one warm-up and one window of BatchBB at that width
and nothing else: the run to put under a kernel trace."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'block-simplex-least-squares_amd')
sys.path[:0] = [ROOT, PKG]

STEPS, WARMUP, WINDOWS = 200, 20, 10


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_bb_C3.txt'))
    ap.add_argument('--config', default='C3')
    ap.add_argument('--widths', default='1,2,4,8')
    ap.add_argument('--profile-only', type=int, default=None, metavar='R')
    a = ap.parse_args()
    import numpy as np
    import torch
    import synthetic
    from device import BatchBB, BBEngine
    if not torch.cuda.is_available():
        raise SystemExit('batch_bb_time needs a HIP device: nothing is timed without one')
    sh = synthetic.make_problem(a.config)
    A, sizes = sh['A'], np.asarray(sh['block_sizes'])
    opts = {'max_iter': 10 ** 9, 'opt_tol': 1e-30}
    widths = [a.profile_only] if a.profile_only else [int(v) for v in a.widths.split(',')]
    engines = []
    for R in widths:
        bs = [synthetic.add_noise(sh['Ax'], 0.02, seed=100 + j) for j in range(R)]
        eng = BatchBB(A, bs, sizes, options=opts, early_exit=False)
        eng.set_z0(None)
        engines.append(('BatchBB R=%d' % R, R, eng))
    if not a.profile_only:
        eng = BBEngine(A, sh['b'], sizes, options=opts, early_exit=False)
        eng.set_z0(np.zeros(eng.nz))
        engines.append(('BBEngine (default)', 1, eng))
    at = {}
    for name, R, eng in engines:
        eng.prologue()
        eng.iterate(1, WARMUP)
        at[name] = WARMUP
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in engines}
    for _ in range(1 if a.profile_only else WINDOWS):
        for name, R, eng in engines:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.iterate(at[name] + 1, STEPS)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
            at[name] += STEPS
    if a.profile_only:
        print('profiled window: BatchBB R=%d, %.1f us per iteration'
              % (a.profile_only, 1e6 * times[engines[0][0]][0] / STEPS))
        return
    lines = ['# %s, one MI355X, early exits off: %d warm-up iterations, then %d windows of %d '
             'iterations,' % (a.config, WARMUP, WINDOWS, STEPS),
             '# the engines alternated window by window in one process; median window '
             '(tools/batch_bb_time.py)',
             '# engine                 us/iteration   us/(iteration problem)   spread (min .. max us)']
    per = {}
    for name, R, eng in engines:
        v = sorted(1e6 * t / STEPS for t in times[name])
        med = 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]) if len(v) % 2 == 0 else v[len(v) // 2]
        per[name] = med / R
        s = np.asarray(eng.scalars()).reshape(-1, 16)
        ok = bool(np.all(np.isfinite(s[:, 4])) and np.all(s[:, 0] == 0))
        lines.append('%-24s %10.1f %18.1f            %.1f .. %.1f%s'
                     % (name, med, med / R, v[0], v[-1], '' if ok else '   (f not finite!)'))
    base = per['BBEngine (default)']
    lines.append('')
    for name, R, eng in engines[:-1]:
        lines.append('# %s: %.2f x the fused engine\'s time per problem'
                     % (name, per[name] / base))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main_()
