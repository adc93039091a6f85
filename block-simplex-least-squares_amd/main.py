#!/usr/bin/env python
"""Entry point and z-space problem build (reference: python/main.py).

    python main.py --file X.mat --method BB [--log INFO] [--eq CP] [--noise 0.02]

solve_in_z(A, b, x0, N, block_sizes, method) keeps the reference's signature
and return value (iters, times, states); the z-space closures f / nabla_f /
proj of python/main.py:53-65 become the device engine (device.BBEngine): the
6 SciPy SpMVs + PAVA of each reference BB iteration become three fused HIP
kernels.  LS_postprocess returns the reference's output dict with the same keys
(python/main.py:81-136), its matrix work done on the device.
"""
import argparse
import logging
import sys

import numpy as np

from bsls_utils import particular_x0, x2z
from gradient_descent import GradientDescent

ACCEPTED_LOG_LEVELS = ['CRITICAL', 'ERROR', 'WARNING', 'INFO', 'DEBUG', 'WARN']


def parser():
    p = argparse.ArgumentParser()
    p.add_argument('--file', help='Data file (*.mat)', default='route_assignment_matrices_ntt.mat')
    p.add_argument('--log', dest='log', nargs='?', const='INFO', default='WARN',
                   help='Set log level (default: WARN)')
    p.add_argument('--method', dest='method', type=str, default='BB', help='Least squares method')
    p.add_argument('--init', dest='init', action='store_true', default=False,
                   help='Initial solution from data')
    p.add_argument('--eq', dest='eq', type=str, default='CP',
                   help='Type of equality constraint (CP or OD)')
    p.add_argument('--noise', dest='noise', type=float, default=None, help='Noise level')
    p.add_argument('--device', dest='device', choices=['gpu', 'cpu'], default=None,
                   help='gpu (default: the MI355X engine) or cpu (the reference\'s own path: '
                        'SciPy closures + the host c_extensions library; also BSLS_DEVICE=cpu)')
    how = p.add_mutually_exclusive_group()
    how.add_argument('--deterministic', dest='deterministic', action='store_true', default=None,
                     help='fixed-order SpMV sums (bit-reproducible runs and exit iterations); '
                          'also BSLS_DETERMINISTIC=1')
    how.add_argument('--reproducible', dest='reproducible', action='store_true', default=None,
                     help='the default engine\'s dealt tiles with order-free fixed-point row '
                          'sums (bit-reproducible runs and exit iterations, method BB only); '
                          'also BSLS_FIXED_SUMS=1')
    p.add_argument('--cv', dest='cv', type=int, default=None, metavar='K',
                   help='after the run, K-fold cross-validation over the links on the same '
                        'engine (cross_validation.kfold; method BB only): output[\'cv\']')
    p.add_argument('--cv-batch', dest='cv_batch', type=int, default=None, metavar='R',
                   help='with --cv: run the folds R (1..8) at a time in lockstep on one batched '
                        'engine (device.BatchBB) instead of one after another')
    p.add_argument('--cv-metrics', dest='cv_metrics', action='store_true', default=False,
                   help='with --cv (and with --cv-batch too): each fold\'s GEH / RMSE link '
                        'metrics over its train and held-out links and per link class by flow '
                        '(CrossValidation.py:186-274), reduced on the device: '
                        'output[\'cv\'][i][\'train\' | \'test\' | \'train_bin\' | \'test_bin\']')
    p.add_argument('--cv-bins', dest='cv_bins', type=int, default=6, metavar='N',
                   help='with --cv-metrics: the number of link classes by flow (default 6, as '
                        'the reference; 1..14)')
    p.add_argument('--reg', dest='reg', type=float, default=None, metavar='LAMBDA',
                   help='the reference\'s L2 regulariser, + 0.5 LAMBDA ||N z + x0||^2 '
                        '(CrossValidation.py:145-148, ISTTT.py:88-92; method BB only; per-route '
                        'weights through the API: build_engine(reg_weights=))')
    return p


def deterministic_default():
    """BSLS_DETERMINISTIC=1 selects the fixed-order engine where no explicit
    choice was made."""
    import os
    return os.environ.get('BSLS_DETERMINISTIC', '0') not in ('', '0')


def build_engine(A, b, x0, block_sizes, options=None, deterministic=None, reproducible=None,
                 row_weights=None, reg_lambda=0.0, reg_weights=None):
    """The device engine of solve_in_z's closures.  deterministic=True keeps
    every SpMV row sum in a fixed order (panels / thread-stream tiles): runs are
    bit-reproducible, so the exact-zero exit of BB.py:22 and the exit iteration
    repeat run to run; the default (dealt tiles, LDS atomic row sums) is faster
    and reproducible to ~1e-16.  reproducible=True keeps the dealt tiles and
    sums their rows in fixed point instead (order-free: bit-reproducible too;
    BB only); None leaves it to BSLS_FIXED_SUMS (BBEngine(fixed_sums=None)).
    row_weights: per-link weights w, f = 0.5 sum w_i r_i^2 (BB only; not with
    reproducible).  reg_lambda / reg_weights: the weighted L2 regulariser, f +
    0.5 lambda ||d o (N z + x0)||^2 (BB only; not with reproducible; x0 the
    particular solution)."""
    from device import BBEngine, reg_lambda_check
    if deterministic is None:
        deterministic = deterministic_default() and not reproducible
    plain = (row_weights is None and not reg_lambda_check(reg_lambda)
             and reg_weights is None)
    return BBEngine(A, b, block_sizes, options=options, x0=x0, deterministic=bool(deterministic),
                    fixed_sums=(True if reproducible else (None if plain else False)),
                    row_weights=row_weights, reg_lambda=reg_lambda, reg_weights=reg_weights)


def solve_in_z(A, b, x0, N, block_sizes, method, options=None, engine=None, deterministic=None,
               row_weights=None, reg_lambda=0.0, reg_weights=None):
    """python/main.py:41-79 on the device.  N is accepted for signature
    compatibility and never used: the engine applies N / N' as per-block
    differences without materialising it.  row_weights and reg_lambda /
    reg_weights (BB only) go to the engine built here; an engine passed in
    keeps its own."""
    if block_sizes is not None and len(block_sizes) == A.shape[1]:
        logging.error('Trivial example: nblocks == nroutes, exiting solver')
        sys.exit()
    block_sizes = np.asarray(block_sizes)
    # the reference's proj asserts strictly increasing z-block starts
    # (c_extensions.pyx:78 through main.py:64): every block needs >= 2 routes
    assert np.all(block_sizes >= 2)
    z0 = x2z(x0, block_sizes)
    eng = engine or build_engine(A, b, x0, block_sizes, deterministic=deterministic,
                                 row_weights=row_weights, reg_lambda=reg_lambda,
                                 reg_weights=reg_weights)
    gd = GradientDescent(z0=z0, method=method, options=options, engine=eng)
    iters, times, states = gd.run()
    import torch
    zl = torch.from_numpy(np.ascontiguousarray(states[-1], dtype=np.float64)).cuda()
    x = eng.n_apply(zl, with_x0=True).cpu().numpy()   # particular_x0 + N z
    assert np.all(x >= 0), "x shouldn't have negative entries after projection"
    return iters, times, states


def solve_many(A, bs, x0, N, block_sizes, options=None, row_weights=None, batch=8):
    """solve_in_z's BB fit for many right-hand sides over one network (the
    --noise draws of python/main.py:164-166, the same links at several times
    of day): the problems run `batch` (1..8) at a time in lockstep on
    device.BatchBB, in balanced groups.  bs: a sequence of vectors or an m x K
    array; row_weights: None or one entry (None or a weight vector) per b.
    Returns [(iters, stop, z)] in the order of bs, stop the message of
    _native.STOP_TEXT.  N is accepted for the signature and never used."""
    import _native
    from device import BatchBB, batch_groups, batch_width
    batch_width(batch)
    block_sizes = np.asarray(block_sizes)
    if hasattr(bs, 'ndim') and bs.ndim == 2:
        bs = [np.asarray(bs)[:, j] for j in range(bs.shape[1])]
    bs = list(bs)
    if row_weights is None:
        row_weights = [None] * len(bs)
    if len(row_weights) != len(bs):
        raise ValueError('row_weights has %d entries for %d problems' % (len(row_weights), len(bs)))
    z0 = x2z(x0, block_sizes)
    out, eng, lo = [], None, 0
    for size in batch_groups(len(bs), batch):
        chunk, wts = bs[lo:lo + size], list(row_weights[lo:lo + size])
        lo += size
        if eng is None or eng.R != size:
            eng = BatchBB(A, chunk, block_sizes, row_weights=wts, options=options, x0=x0)
        else:
            for j in range(size):
                eng.set_b(j, chunk[j])
                eng.set_row_weights(j, wts[j])
        zs = eng.solve(z0=[z0] * size)
        out += [(int(eng.iterations[j]), _native.STOP_TEXT[int(eng.stop_reasons[j])], zs[j])
                for j in range(size)]
    return out


def host_closures(A, N, target, x0, row_weights=None, reg_lambda=0.0, reg_weights=None):
    """(f, nabla_f) of the host path over SciPy: main.py:53-54; with
    row_weights w the engine's weighted objective; with reg_lambda the
    reference's regularised one as written at CrossValidation.py:141-144, D =
    sqrt(lambda) d and D2 = lambda d^2 (d None: ones)."""
    import numpy.linalg as la
    from device import reg_lambda_check, reg_weights_check, row_weights_check
    AT = A.T.tocsr()
    NT = N.T.tocsr()
    w = row_weights_check(row_weights, A.shape[0])
    lam = reg_lambda_check(reg_lambda)
    if w is not None:
        def f0(z):
            r = A.dot(N.dot(z)) + target
            return 0.5 * np.sum(w * r * r)

        def g0(z):
            r = A.dot(N.dot(z)) + target
            return NT.dot(AT.dot(w * r))
    else:
        f0 = lambda z: 0.5 * la.norm(A.dot(N.dot(z)) + target) ** 2
        g0 = lambda z: NT.dot(AT.dot(A.dot(N.dot(z)) + target))
    if not lam:
        return f0, g0
    d = reg_weights_check(reg_weights, A.shape[1])
    if d is None:
        d = np.ones(A.shape[1])
    D, D2 = np.sqrt(lam) * d, lam * d * d
    x0 = np.asarray(x0, dtype=np.float64)
    f = lambda z: f0(z) + 0.5 * la.norm(D * (N.dot(z) + x0)) ** 2
    nabla_f = lambda z: g0(z) + NT.dot(D2 * (N.dot(z) + x0))
    return f, nabla_f


def solve_in_z_cpu(A, b, x0, N, block_sizes, method, options=None, row_weights=None,
                   reg_lambda=0.0, reg_weights=None, record_every=None):
    """python/main.py:41-79 on the host (BASELINE configs[0]): the reference's
    closures over SciPy csr_matvec, proj = the host c_extensions library's
    isotonic_regression_multi (include/bsls_cpu.h) + clip, the solver loops of
    BB.py / LBFGS.py / DORE.py over them.  row_weights w (BB only): the
    engine's weighted objective, f = 0.5 sum w r^2, nabla_f = N'A'(w r).
    reg_lambda / reg_weights (BB only): the reference's regularised closures
    (host_closures).  record_every (BB only): BB.solve's, None for its 500."""
    from bsls_utils import particular_x0
    from c_extensions import _cpu
    from device import reg_lambda_check
    if block_sizes is not None and len(block_sizes) == A.shape[1]:
        logging.error('Trivial example: nblocks == nroutes, exiting solver')
        sys.exit()
    block_sizes = np.asarray(block_sizes)
    assert np.all(block_sizes >= 2)
    z0 = x2z(x0, block_sizes)
    target = A.dot(x0) - b
    if row_weights is not None and method != 'BB':
        raise ValueError('row_weights cover method BB only (got %r)' % method)
    if reg_lambda_check(reg_lambda) and method != 'BB':
        raise ValueError('a regulariser covers method BB only (got %r)' % method)
    f, nabla_f = host_closures(A, N, target, x0, row_weights, reg_lambda, reg_weights)
    cum_blocks = np.concatenate(([0], np.cumsum(block_sizes - 1)))

    def proj(x):
        _cpu.isotonic(1, x, cum_blocks[:-1], x.shape[0], None, 1)
        return np.maximum(np.minimum(x, 1.), 0.)
    kw = dict(A=A, N=N, target=target) if method == 'DORE' else {}
    gd = GradientDescent(z0=z0, f=f, nabla_f=nabla_f, proj=proj, method=method, options=options,
                         record_every=record_every, **kw)
    iters, times, states = gd.run()
    x = particular_x0(block_sizes) + N.dot(states[-1])
    assert np.all(x >= 0), "x shouldn't have negative entries after projection"
    return iters, times, states


def LS_postprocess_cpu(states, x0, A, b, x_true, scaling=None, block_sizes=None, output=None,
                       N=None, is_x=False):
    """python/main.py:81-136 on the host (NumPy / SciPy)."""
    import numpy.linalg as la
    if x_true is None:
        return [], [], output
    if scaling is None:
        scaling = np.ones(x_true.shape)
    if output is None:
        output = {}
    d = len(states)
    if not is_x and N.size > 0:
        x_hat = N.dot(np.array(states).T) + np.tile(x0, (d, 1)).T
    else:
        x_hat = np.array(states).T
    x_last = x_hat[:, -1]
    n = x_hat.shape[1]
    output['AA'] = A.shape
    output['x_hat'] = x_hat.shape
    output['blocks'] = block_sizes.shape if block_sizes is not None else None
    starting_error = 0.5 * la.norm(A.dot(x0) - b) ** 2
    opt_error = 0.5 * la.norm(A.dot(x_true) - b) ** 2
    diff = A.dot(x_hat) - np.tile(b, (d, 1)).T
    error = 0.5 * np.diag(diff.T.dot(diff))
    output['0.5norm(Ax-b)^2'], output['0.5norm(Ax_init-b)^2'] = error, starting_error
    output['0.5norm(Ax*-b)^2'] = opt_error
    x_true_block = np.tile(x_true, (n, 1))
    x_diff = x_true_block - x_hat.T
    scaling_block = np.tile(scaling, (n, 1))
    x_diff_scaled = scaling_block * x_diff
    x_true_scaled = scaling_block * x_true_block
    output['max|f * (x-x_true)|'] = np.max(x_diff_scaled, axis=1)
    output['incorrect x entries'] = np.bincount(np.where(x_diff > 1e-3)[0])
    output['percent flow allocated incorrectly'] = (np.sum(np.abs(x_diff_scaled), axis=1)
                                                    / np.sum(x_true_scaled, axis=1))
    output['max|f * (x_init-x_true)|'] = np.max(scaling * np.abs(x_true - x0))
    return x_last, error, output


def LS_postprocess(states, x0, A, b, x_true, scaling=None, block_sizes=None, output=None, N=None,
                   is_x=False, engine=None):
    """python/main.py:81-136: objective and route-flow error metrics per logged
    state.  X_hat = x0 + N Z and A X_hat are formed on the device."""
    import torch
    if x_true is None:
        return [], [], output
    if scaling is None:
        scaling = np.ones(x_true.shape)
    if output is None:
        output = {}
    d = len(states)
    from device import DeviceCSR, BlockLayout
    bt = torch.from_numpy(np.asarray(b, dtype=np.float64)).cuda()
    if engine is not None:
        # A x on the engine's K1 image (no general CSR copy of A)
        def a_minus_b(x):
            return engine.apply_A_x(x) - bt
    else:
        Ad = DeviceCSR(A)

        def a_minus_b(x):
            return Ad.matvec(x, add=-bt)
    cols = []
    if not is_x and (N is None or N.size > 0):
        lay = engine.layout if engine is not None else BlockLayout(block_sizes)
        from c_extensions.c_extensions import z2x_c  # noqa: F401  (same kernel family)
        import _native
        from _native import ptr, stream_handle, check
        x0d = torch.from_numpy(np.asarray(x0, dtype=np.float64)).cuda()
        for s in states:
            zd = torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).cuda()
            xd = torch.empty(lay.n, dtype=torch.float64, device='cuda')
            check(_native.lib().bsls_n_apply(ptr(xd), ptr(zd), ptr(lay.xstarts), lay.p, lay.n,
                                             0, stream_handle()), 'bsls_n_apply')
            cols.append(xd + x0d)
    else:
        cols = [torch.from_numpy(np.asarray(s, dtype=np.float64)).cuda() for s in states]
    X = torch.stack(cols, dim=1)                       # n x d
    x_last = X[:, -1].cpu().numpy()
    output['AA'] = A.shape
    output['x_hat'] = tuple(X.shape)
    output['blocks'] = block_sizes.shape if block_sizes is not None else None
    x0d = torch.from_numpy(np.asarray(x0, dtype=np.float64)).cuda()
    xtd = torch.from_numpy(np.asarray(x_true, dtype=np.float64)).cuda()
    r0 = a_minus_b(x0d)
    rs = a_minus_b(xtd)
    starting_error = 0.5 * float(r0.norm()) ** 2
    opt_error = 0.5 * float(rs.norm()) ** 2
    err = np.array([0.5 * float(a_minus_b(X[:, k].contiguous()).square().sum())
                    for k in range(d)])
    output['0.5norm(Ax-b)^2'], output['0.5norm(Ax_init-b)^2'] = err, starting_error
    output['0.5norm(Ax*-b)^2'] = opt_error
    sc = torch.from_numpy(np.asarray(scaling, dtype=np.float64)).cuda()
    xdiff = xtd[None, :] - X.T                          # d x n
    xds = sc[None, :] * xdiff
    xts = sc[None, :] * xtd[None, :].expand_as(xdiff)
    output['max|f * (x-x_true)|'] = xds.max(dim=1).values.cpu().numpy()
    wrong = torch.nonzero(xdiff > 1e-3)[:, 0].cpu().numpy()
    output['incorrect x entries'] = np.bincount(wrong)
    output['percent flow allocated incorrectly'] = (xds.abs().sum(dim=1) /
                                                    xts.sum(dim=1)).cpu().numpy()
    output['max|f * (x_init-x_true)|'] = float(np.max(scaling * np.abs(x_true - x0)))
    return x_last, err, output


def main(args=None, plot=False):
    if args is None:
        args = parser().parse_args()
    reproducible = getattr(args, 'reproducible', None)
    if reproducible and args.method != 'BB':
        raise ValueError('--reproducible covers --method BB only (got %r)' % args.method)
    if reproducible and getattr(args, 'deterministic', None):
        raise ValueError('--reproducible and --deterministic exclude each other')
    cv = getattr(args, 'cv', None)
    if cv is not None and args.method != 'BB':
        raise ValueError('--cv covers --method BB only (got %r)' % args.method)
    if cv is not None and reproducible:
        raise ValueError('--cv and --reproducible exclude each other')
    reg = getattr(args, 'reg', None)
    if reg is not None and args.method != 'BB':
        raise ValueError('--reg covers --method BB only (got %r)' % args.method)
    if reg is not None and reproducible:
        raise ValueError('--reg and --reproducible exclude each other')
    cv_batch = getattr(args, 'cv_batch', None)
    if cv_batch is not None and cv is not None and reg:
        raise ValueError('--cv-batch does not cover --reg')
    if cv_batch is not None and cv is None:
        raise ValueError('--cv-batch needs --cv')
    if cv_batch is not None and not 1 <= cv_batch <= 8:
        raise ValueError('--cv-batch takes 1..8 (got %r)' % (cv_batch,))
    cv_metrics = bool(getattr(args, 'cv_metrics', False))
    cv_bins = getattr(args, 'cv_bins', 6)
    if cv_metrics and cv is None:
        raise ValueError('--cv-metrics needs --cv')
    if cv_metrics and not 1 <= cv_bins <= 14:
        raise ValueError('--cv-bins takes 1..14 (got %r)' % (cv_bins,))
    if args.log in ACCEPTED_LOG_LEVELS:
        logging.basicConfig(level=getattr(logging, args.log))
    config = {'full': True, 'L': True, 'OD': True, 'CP': True, 'LP': True,
              'eq': args.eq, 'init': args.init}
    from bsls_matrices import BSLSMatrices
    bm = BSLSMatrices(fname=args.file, **config)
    bm.degree_reduced_form()
    AA, bb, N, block_sizes, x_split, nz, scaling, rsort_index, x0 = bm.get_LS()
    output = bm.info
    if reg and not np.array_equal(np.asarray(x0, dtype=np.float64).reshape(-1),
                                  particular_x0(block_sizes)):
        # the device adds the particular x0 to N z itself; the host path would
        # take any x0, so the same command is refused on both
        raise ValueError('--reg needs the particular x0 (1 at each block\'s last route) as the '
                         'initial solution: not with --init data that gives another')
    if args.noise:
        delta = np.random.normal(scale=bb * args.noise)
        bb = bb + delta
    device = getattr(args, 'device', None)
    if device is None:
        import _native
        device = 'cpu' if _native.device_mode() == 'cpu' else 'gpu'
    if device == 'cpu':
        iters, times, states = solve_in_z_cpu(AA, bb, x0, N, block_sizes, args.method,
                                              reg_lambda=reg or 0.0)
        x_last, error, output = LS_postprocess_cpu(states, x0, AA, bb, x_split, scaling=scaling,
                                                   block_sizes=block_sizes, N=N, output=output)
        if cv is not None:
            from cross_validation import kfold
            output['cv'] = kfold(AA, bb, x0, N, block_sizes, cv, device='cpu', batch=cv_batch,
                                 reg_lambda=reg or 0.0, metrics=cv_metrics, nbins=cv_bins)
        return iters, times, states, output
    eng = build_engine(AA, bb, x0, block_sizes,
                       deterministic=getattr(args, 'deterministic', None),
                       reproducible=reproducible, reg_lambda=reg or 0.0)
    iters, times, states = solve_in_z(AA, bb, x0, N, block_sizes, args.method, engine=eng)
    x_last, error, output = LS_postprocess(states, x0, AA, bb, x_split, scaling=scaling,
                                           block_sizes=block_sizes, N=N, output=output,
                                           engine=eng)
    if cv is not None:
        from cross_validation import kfold
        output['cv'] = kfold(AA, bb, x0, N, block_sizes, cv, engine=eng, batch=cv_batch,
                             reg_lambda=reg or 0.0, metrics=cv_metrics, nbins=cv_bins)
    if plot:
        import matplotlib.pyplot as plt
        plt.figure(); plt.hist(x_last)
        plt.figure(); plt.loglog(np.cumsum(times), error); plt.show()
    return iters, times, states, output


if __name__ == '__main__':
    iters, times, states, output = main()
    print(output)
