"""What per-link weights (bsls_bb_problem.roww) cost on C3, and what one engine
for every fold saves.

  python tools/row_weights_ab.py [--parent LIB] [--out FILE] [--rounds 3]

Four configurations, alternated, `--rounds` runs each, a fresh process per run
(the library is chosen when _native is imported), 200-iteration windows after
20 warm-up iterations:
  parent    the parent commit's library through BSLS_LIB (--parent; skipped
            without it), unweighted
  plain     this build, unweighted
  ones      this build, all-ones weights
  mask      this build, a 1-in-5 mask (fold 0 of kfold_masks(m, 5))
then, in one more process, cross_validation.kfold(k=5) on one engine against
five engine builds + solves (100 iterations a fold)."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'block-simplex-least-squares_amd')
sys.path[:0] = [ROOT, PKG]

STEPS, WARMUP, FOLD_ITERS = 200, 20, 100


def problem():
    import synthetic
    return synthetic.make_problem('C3')


def child_window(config):
    import numpy as np
    import torch
    from device import BBEngine
    from cross_validation import kfold_masks
    sh = problem()
    m = sh['A'].shape[0]
    w = {'parent': None, 'plain': None, 'ones': np.ones(m), 'mask': kfold_masks(m, 5)[0]}[config]
    kw = {} if w is None else {'row_weights': w}
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


def child_folds():
    import numpy as np
    import torch
    import main
    from bsls_utils import particular_x0, x2z
    from cross_validation import kfold, kfold_masks
    sh = problem()
    A, b, sizes = sh['A'], sh['b'], np.asarray(sh['block_sizes'])
    x0 = particular_x0(sizes)
    opts = {'max_iter': FOLD_ITERS, 'opt_tol': 1e-30}
    # warm the process (kernel loads, allocator) outside both timings
    main.build_engine(A, b, x0, sizes, options=opts).solve()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    folds = kfold(A, b, x0, None, sizes, 5, options=opts)
    torch.cuda.synchronize()
    one = time.perf_counter() - t0
    t0 = time.perf_counter()
    z0 = x2z(x0, sizes)
    for w in kfold_masks(A.shape[0], 5):
        eng = main.build_engine(A, b, x0, sizes, options=opts, row_weights=w)
        eng.solve(z0=z0)
        torch.cuda.synchronize()
    five = time.perf_counter() - t0
    print('RESULT folds kfold(k=5, %d iterations a fold) on one engine %.3f s (solves %.3f s); '
          'five engine builds + solves %.3f s; ratio %.2f'
          % (FOLD_ITERS, one, sum(f['seconds'] for f in folds), five, five / one), flush=True)


def run_child(arg, lib=None):
    env = dict(os.environ)
    env.pop('BSLS_LIB', None)
    if lib:
        env['BSLS_LIB'] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', arg], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = [l for l in out.stdout.splitlines() if l.startswith('RESULT ')]
    if out.returncode != 0 or not lines:
        raise RuntimeError('child %s failed (%d):\n%s' % (arg, out.returncode, out.stdout[-2000:]))
    return lines[-1][len('RESULT '):]


def main_():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--parent', help="the parent commit's libbsls_hip.so")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'row_weights_C3.txt'))
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    if a.child == 'folds':
        return child_folds()
    if a.child:
        return child_window(a.child)
    configs = (['parent'] if a.parent else []) + ['plain', 'ones', 'mask']
    rates = {c: [] for c in configs}
    lines = ['# C3 (1M routes / 50k blocks / 100k links), one MI355X: %d-iteration windows after %d '
             'warm-up iterations,' % (STEPS, WARMUP),
             '# a fresh process per run, the configurations alternated, %d rounds '
             '(tools/row_weights_ab.py)' % a.rounds]
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
    for c in ('ones', 'mask'):
        lines.append('# %s / plain = %.4f (%+.2f us per iteration)'
                     % (c, med[c] / med['plain'], 1e6 / med[c] - 1e6 / med['plain']))
    lines.append('')
    lines.append('# ' + run_child('folds'))
    text = '\n'.join(lines) + '\n'
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text)


if __name__ == '__main__':
    main_()
