"""What the weighted L2 regulariser (bsls_bb_problem.reg_w) costs on C3, and what
one engine for every (lambda, fold) saves.

  python tools/reg_ab.py [--parent LIB] [--out FILE] [--rounds 3]

Four configurations, alternated, `--rounds` runs each, a fresh process per run
(the library is chosen when _native is imported), 200-iteration windows after
20 warm-up iterations:
  parent    the parent commit's library through BSLS_LIB (--parent; skipped
            without it), no regulariser
  plain     this build, no regulariser
  ones      this build, lambda = 100, unit weights
  random    this build, lambda = 100, d = 0.5 + 1.5 U(0, 1)
then bb_reg alone (200 launches, its bytes over its time), and in one more
process cross_validation.kfold_path over 5 lambda x 5 folds on one engine
against 25 engine builds + solves (100 iterations a fit).  Every child runs
under its own time limit; the first that fails ends the job."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'block-simplex-least-squares_amd')
sys.path[:0] = [ROOT, PKG]

STEPS, WARMUP, FIT_ITERS = 200, 20, 100
LAMBDA = 100.0
PATH = (1.0, 10.0, 100.0, 1.0e3, 1.0e4)
CHILD_LIMIT = 300           # seconds, per child process


def problem():
    import synthetic
    return synthetic.make_problem('C3')


def weights(n):
    import numpy as np
    return 0.5 + 1.5 * np.random.RandomState(11).rand(n)


def child_window(config):
    import numpy as np
    import torch
    from device import BBEngine
    sh = problem()
    n = sh['A'].shape[1]
    kw = {'parent': {}, 'plain': {}, 'ones': {'reg_lambda': LAMBDA},
          'random': {'reg_lambda': LAMBDA, 'reg_weights': weights(n)}}[config]
    eng = BBEngine(sh['A'], sh['b'], sh['block_sizes'],
                   options={'max_iter': 10 ** 9, 'opt_tol': 1e-30}, **kw)
    eng.set_z0(np.zeros(eng.nz))
    eng.prologue()
    eng.iterate(1, WARMUP)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.iterate(WARMUP + 1, STEPS)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = eng.scalars()
    print('RESULT %s %.1f it/s (%d iterations in %.4f s, f %.6e, stop flag %d)'
          % (config, STEPS / dt, STEPS, dt, s[4], int(s[0])), flush=True)


def child_kernel():
    """bb_reg alone: xz (4 B) + reg_w (8 B) per route read, z read and reg_g
    written per z entry (8 B each; z's gathers are two adjacent entries, so
    each line is read once)."""
    import numpy as np
    import torch
    import _native
    from _native import stream_handle
    from device import BBEngine
    sh = problem()
    eng = BBEngine(sh['A'], sh['b'], sh['block_sizes'], reg_lambda=LAMBDA,
                   reg_weights=weights(sh['A'].shape[1]))
    eng.set_z0(np.zeros(eng.nz))
    L, st = _native.lib(), stream_handle()
    for _ in range(20):
        L.bsls_bb_reg(eng.P, 0, 0, st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        L.bsls_bb_reg(eng.P, 0, 0, st)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / STEPS
    nbytes = 12 * eng.n + 16 * eng.nz
    print('RESULT kernel bb_reg %.2f us a launch (%d back to back), %.1f MB: %.0f GB/s'
          % (1e6 * dt, STEPS, nbytes / 1e6, nbytes / dt / 1e9), flush=True)


def child_path():
    import numpy as np
    import torch
    import main
    from bsls_utils import particular_x0, x2z
    from cross_validation import kfold_masks, kfold_path
    sh = problem()
    A, b, sizes = sh['A'], sh['b'], np.asarray(sh['block_sizes'])
    x0 = particular_x0(sizes)
    d = weights(A.shape[1])
    opts = {'max_iter': FIT_ITERS, 'opt_tol': 1e-30}
    # warm the process (kernel loads, allocator) outside both timings
    main.build_engine(A, b, x0, sizes, options=opts, reg_lambda=LAMBDA, reg_weights=d).solve()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    path = kfold_path(A, b, x0, None, sizes, 5, PATH, reg_weights=d, options=opts)
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    t0 = time.perf_counter()
    z0 = x2z(x0, sizes)
    for lam in PATH:
        for w in kfold_masks(A.shape[0], 5):
            eng = main.build_engine(A, b, x0, sizes, options=opts, row_weights=w, reg_lambda=lam,
                                    reg_weights=d)
            eng.solve(z0=z0)
            torch.cuda.synchronize()
    many = time.perf_counter() - t0
    print('RESULT path kfold_path(%d lambda x 5 folds, %d iterations a fit) on one engine %.3f s '
          '(solves %.3f s), best lambda %g; 25 engine builds + solves %.3f s; ratio %.2f'
          % (len(PATH), FIT_ITERS, one,
             sum(f['seconds'] for fs in path['folds'] for f in fs), path['best'], many,
             many / one), flush=True)


def run_child(arg, lib=None):
    env = dict(os.environ)
    env.pop('BSLS_LIB', None)
    if lib:
        env['BSLS_LIB'] = lib
    out = subprocess.run(['timeout', '-k', '10', str(CHILD_LIMIT), sys.executable,
                          os.path.abspath(__file__), '--child', arg], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')]
    if out.returncode != 0 or not lines:
        # nothing more is started on the GPU after a child that failed
        raise SystemExit('child %s failed (%d):\n%s' % (arg, out.returncode, out.stdout[-2000:]))
    return lines[-1][len('RESULT '):]


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--parent', help="the parent commit's libbsls_hip.so")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reg_C3.txt'))
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if a.child == 'path':
        return child_path()
    if a.child == 'kernel':
        return child_kernel()
    if a.child:
        return child_window(a.child)
    configs = (['parent'] if a.parent else []) + ['plain', 'ones', 'random']
    rates = {c: [] for c in configs}
    lines = ['# C3 (1M routes / 50k blocks / 100k links), one MI355X: %d-iteration windows after %d '
             'warm-up iterations,' % (STEPS, WARMUP),
             '# a fresh process per run, the configurations alternated, %d rounds '
             '(tools/reg_ab.py); lambda = %g' % (a.rounds, LAMBDA)]
    for rnd in range(1, a.rounds + 1):
        for c in configs:
            res = run_child(c, a.parent if c == 'parent' else None)
            rates[c].append(float(res.split()[1]))
            lines.append('== %s %d\n%s' % (c, rnd, res))
            print(lines[-1], flush=True)
    lines.append('')
    med = {}
    for c in configs:
        v = sorted(rates[c])
        med[c] = v[len(v) // 2]
        lines.append('# %-6s median %.0f it/s (%.1f us), spread %.2f %% (min %.0f, max %.0f)'
                     % (c, med[c], 1e6 / med[c], 100.0 * (v[-1] - v[0]) / med[c], v[0], v[-1]))
    if 'parent' in med:
        lines.append('# plain / parent = %.4f' % (med['plain'] / med['parent']))
    for c in ('ones', 'random'):
        lines.append('# %s / plain = %.4f (%+.2f us per iteration)'
                     % (c, med[c] / med['plain'], 1e6 / med[c] - 1e6 / med['plain']))
    lines.append('')
    lines.append('# ' + run_child('kernel'))
    lines.append('# ' + run_child('path'))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main_()
