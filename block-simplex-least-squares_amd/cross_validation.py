"""K-fold cross-validation over the links (reference: python/CrossValidation.py).

The reference's fold loop (CrossValidation.py:126-183) takes the train rows
A[train, :], b[train], runs z-space BB on them and scores the fit on the
held-out links.  Here a fold is a 0/1 vector of per-link weights on ONE device
engine (device.BBEngine.set_row_weights): the matrix images are the whole
problem's, built once, the weights act in K1's row finish, and the same pass
that forms f over the train rows sums the held-out error.  Label-grouped folds
and the regularised objectives of the reference are not carried.
"""
import logging
import time

import numpy as np


def kfold_masks(m, k, shuffle=False, seed=0):
    """k float64 0/1 vectors of length m; every row is 0 (held out) in exactly
    one of them.  Without shuffle the folds are contiguous index ranges whose
    sizes differ by at most one, the first m % k one longer -- sklearn's
    KFold(n, n_folds=k) as the reference calls it; shuffle permutes the rows
    first (numpy RandomState(seed))."""
    m, k = int(m), int(k)
    if k < 2:
        raise ValueError('k-fold cross-validation needs k >= 2 (got %d)' % k)
    if k > m:
        raise ValueError('more folds (%d) than rows (%d)' % (k, m))
    idx = np.arange(m)
    if shuffle:
        idx = np.random.RandomState(seed).permutation(m)
    sizes = np.full(k, m // k, dtype=np.int64)
    sizes[:m % k] += 1
    ends = np.cumsum(sizes)
    masks = []
    for lo, hi in zip(ends - sizes, ends):
        w = np.ones(m, dtype=np.float64)
        w[idx[lo:hi]] = 0.0
        masks.append(w)
    return masks


class _StopText(logging.Handler):
    """The message solvers.stopping logs when it ends a host run."""

    def __init__(self):
        logging.Handler.__init__(self, level=logging.WARNING)
        self.text = None

    def emit(self, record):
        msg = record.getMessage()
        if msg.startswith('Exiting...'):
            self.text = msg


def _kfold_cpu(A, b, x0, N, block_sizes, masks, options):
    from main import solve_in_z_cpu
    out = []
    target = A.dot(x0) - b
    max_iter = options.get('max_iter') if options else None
    for w in masks:
        catch = _StopText()
        root = logging.getLogger()
        root.addHandler(catch)
        t0 = time.time()
        try:
            iters, _, states = solve_in_z_cpu(A, b, x0, N, block_sizes, 'BB', options=options,
                                              row_weights=w)
        finally:
            root.removeHandler(catch)
        dt = time.time() - t0
        z = np.asarray(states[-1], dtype=np.float64)
        r = A.dot(N.dot(z)) + target
        if max_iter is not None and iters[-1] >= max_iter:
            stop = 'max_iter'
        else:
            # (BB.py:22's exact-zero sum(delta_g) exit prints the same text
            # as the stopping rule's last test)
            stop = catch.text or 'Exiting... no change in gradient'
        out.append({'iters': int(iters[-1]), 'stop': stop,
                    'f_train': 0.5 * float(np.sum(w * r * r)),
                    'held_out': 0.5 * float(np.sum(r[w == 0.0] ** 2)),
                    'z': z, 'seconds': dt})
    return out


def _kfold_batch(A, b, x0, block_sizes, masks, options, batch):
    """The folds `batch` at a time on one device.BatchBB (balanced chunks,
    device.batch_groups); a fold's seconds is its chunk's time divided by the
    chunk's size."""
    import _native
    from bsls_utils import x2z
    from device import BatchBB, batch_groups
    z0 = x2z(x0, block_sizes)
    out = []
    eng, lo = None, 0
    for size in batch_groups(len(masks), batch):
        chunk = masks[lo:lo + size]
        lo += size
        t0 = time.time()
        if eng is None or eng.R != size:
            eng = BatchBB(A, [b] * size, block_sizes, row_weights=chunk, options=options, x0=x0)
        else:
            for j, w in enumerate(chunk):
                eng.set_row_weights(j, w)
        zs = eng.solve(z0=[z0] * size)
        S, held = eng.scalars(), eng.held_out()
        dt = (time.time() - t0) / size
        for j in range(size):
            out.append({'iters': int(eng.iterations[j]),
                        'stop': _native.STOP_TEXT[int(eng.stop_reasons[j])],
                        'f_train': float(S[j, _native.S_FX]), 'held_out': held[j],
                        'z': zs[j], 'seconds': dt})
    return out


def kfold(A, b, x0, N, block_sizes, k, options=None, device='gpu', engine=None, shuffle=False,
          seed=0, deterministic=None, batch=None):
    """K-fold cross-validation of the z-space BB fit: fold i holds out the rows
    where kfold_masks(m, k)[i] is 0, fits the rest from z0 = x2z(x0) and scores
    0.5 ||A_test x - b_test||^2 on the held-out rows.  Returns one dict per
    fold: iters, stop (the message), f_train, held_out, z (host array), seconds.

    device='gpu': one engine serves every fold -- `engine` (its weights are
    put back afterwards) or one built here -- and held_out is the engine's own
    (BBEngine.held_out), not recomputed.  device='cpu': main.solve_in_z_cpu
    per fold over SciPy.  options: the solver's (max_iter, opt_tol); None keeps
    the engine's on 'gpu' and GradientDescent's defaults on 'cpu'.

    batch: None (the sequential path above), or an int in 1..8: the folds run
    `batch` at a time in lockstep on one device.BatchBB (plain CSR images of A
    and A', every sum in a fixed order; `engine` and `deterministic` are not
    used).  Same keys; seconds is the chunk's time divided by its size.
    device='cpu' accepts and ignores it.  Measured on C3 (profiles/batch_bb_C3.txt): the batch costs
    147.9 us per iteration and problem at batch = 8 (342.6 at 1) against the
    fused engine's 73.5 us, so the sequential path is the faster one and stays
    the default; batch buys lockstep fits that repeat bit for bit."""
    if batch is not None:
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) \
                or not 1 <= batch <= 8:
            raise ValueError('batch must be None or an int in 1..8 (got %r)' % (batch,))
    from bsls_utils import x2z
    block_sizes = np.asarray(block_sizes)
    masks = kfold_masks(A.shape[0], k, shuffle=shuffle, seed=seed)
    if device == 'cpu':
        return _kfold_cpu(A, b, x0, N, block_sizes, masks, options)
    if device != 'gpu':
        raise ValueError("device must be 'gpu' or 'cpu' (got %r)" % (device,))
    if batch is not None:
        return _kfold_batch(A, b, x0, block_sizes, masks, options, int(batch))
    import torch
    import _native
    from main import build_engine
    eng = engine
    if eng is None:
        eng = build_engine(A, b, x0, block_sizes, options=options, deterministic=deterministic,
                           row_weights=masks[0])
    before = eng.row_weights
    keep = (eng.P.max_iter, eng.P.opt_tol)
    if options is not None:
        eng.P.max_iter = int(options.get('max_iter', 300000))
        eng.P.opt_tol = float(options.get('opt_tol', 1e-6))
    z0 = x2z(x0, block_sizes)
    out = []
    try:
        for w in masks:
            t0 = time.time()
            eng.set_row_weights(w)
            z = eng.solve(z0=z0).cpu().numpy().copy()
            torch.cuda.synchronize()
            s = eng.scalars()
            out.append({'iters': int(eng.iterations),
                        'stop': _native.STOP_TEXT[int(eng.stop_reason)],
                        'f_train': float(s[_native.S_FX]), 'held_out': eng.held_out(),
                        'z': z, 'seconds': time.time() - t0})
    finally:
        eng.set_row_weights(before)
        eng.P.max_iter, eng.P.opt_tol = keep
    return out
