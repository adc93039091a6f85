"""K-fold cross-validation over the links (reference: python/CrossValidation.py).

The reference's fold loop (CrossValidation.py:126-183) takes the train rows
A[train, :], b[train], runs z-space BB on them and scores the fit on the
held-out links.  Here a fold is a 0/1 vector of per-link weights on ONE device
engine (device.BBEngine.set_row_weights): the matrix images are the whole
problem's, built once, the weights act in K1's row finish, and the same pass
that forms f over the train rows sums the held-out error.  The reference's
label-grouped folds are label_masks; its regularised objective (reg = 'L2',
with or without weights, CrossValidation.py:140-148) is the engine's
set_regulariser, and kfold_path picks lambda over every (lambda, fold) on one
engine.  Its post_process (CrossValidation.py:186-285: GEH, RMSE and error over
the train and held-out links and per link class by flow) is kfold's
metrics=True, reduced on the device by dev_metrics / csrc/metrics.hip.  Loading
the reference's travel-time and label pickles is not carried.
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


def label_masks(labels, k=None):
    """Folds that keep the rows of one label together, as float64 0/1 vectors
    (0 = held out; every row in exactly one fold).  k=None: one fold per
    distinct label, in sorted label order -- sklearn's LeaveOneLabelOut as the
    reference calls it for taz_ids / city_ids (CrossValidation.py:75-91).  An
    int k: KFold(k) over the sorted distinct labels, the first (labels % k)
    folds one label longer (the street_names form, :92-110)."""
    labels = np.asarray(labels).reshape(-1)
    if labels.size == 0:
        raise ValueError('label_masks needs one label per row')
    uniq, inv = np.unique(labels, return_inverse=True)
    nl = int(uniq.size)
    if k is None:
        if nl < 2:
            raise ValueError('leave-one-label-out needs at least 2 distinct labels')
        groups = [[j] for j in range(nl)]
    else:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
            raise ValueError('label folds need an int k >= 2 (got %r)' % (k,))
        if k > nl:
            raise ValueError('more folds (%d) than distinct labels (%d)' % (k, nl))
        sizes = np.full(int(k), nl // int(k), dtype=np.int64)
        sizes[:nl % int(k)] += 1
        ends = np.cumsum(sizes)
        groups = [list(range(lo, hi)) for lo, hi in zip(ends - sizes, ends)]
    masks = []
    for grp in groups:
        w = np.ones(labels.size, dtype=np.float64)
        w[np.isin(inv.reshape(-1), grp)] = 0.0
        masks.append(w)
    return masks


def _fold_masks(m, k, shuffle, seed, masks):
    """kfold's folds: the caller's masks (each m values, 0 = held out), or
    kfold_masks(m, k)."""
    if masks is None:
        return kfold_masks(m, k, shuffle=shuffle, seed=seed)
    from device import row_weights_check
    masks = [row_weights_check(w, m) for w in masks]
    if not masks:
        raise ValueError('masks is empty')
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


def _cells_numpy(ax, b, w, edges):
    """dev_metrics.link_metrics' table with NumPy: per state, over the train
    rows (w != 0) and the held-out ones (w == 0) of each class
    np.digitize(b, edges), the sums of CrossValidation.py:193-214 on A[rows],
    b[rows]."""
    ax = np.atleast_2d(np.asarray(ax, dtype=np.float64))
    b = np.asarray(b, dtype=np.float64)
    cls = np.digitize(b, edges) if edges.size else np.zeros(b.size, dtype=np.int64)
    held = np.zeros(b.size, dtype=bool) if w is None else (np.asarray(w) == 0)
    cells = np.zeros((ax.shape[0], 2, edges.size + 1, 9))
    with np.errstate(all='ignore'):
        for s in range(ax.shape[0]):
            diff, plus = ax[s] - b, ax[s] + b
            d2 = diff ** 2
            geh = np.sqrt(2 * d2 / plus)
            for st in (0, 1):
                for c in range(edges.size + 1):
                    rows = (held == bool(st)) & (cls == c)
                    if not rows.any():
                        continue
                    g = geh[rows]
                    cells[s, st, c] = [rows.sum(), d2[rows].sum(), g.sum(), g.max(),
                                       (g < 5).sum(), (g < 1).sum(), (g < 0.5).sum(),
                                       (g < 0.05).sum(), b[rows].sum()]
    return cells


def _metrics_cpu(A, b, x0, N, w, states, edges, many):
    """The metric dicts of one fold on the host: x_hat = N z + x0 per state."""
    from dev_metrics import metrics_from_cells
    ax = np.stack([A.dot(N.dot(np.asarray(z, dtype=np.float64)) + x0) for z in states])
    cells = _cells_numpy(ax, b, w, edges)
    return metrics_from_cells(cells if many else cells[0])


def _kfold_cpu(A, b, x0, N, block_sizes, masks, options, reg_lambda=0.0, reg_weights=None,
               edges=None, record_every=None):
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
                                              row_weights=w, reg_lambda=reg_lambda,
                                              reg_weights=reg_weights, record_every=record_every)
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
        f_train = 0.5 * float(np.sum(w * r * r))
        if reg_lambda:
            d = np.ones(A.shape[1]) if reg_weights is None else np.asarray(reg_weights)
            xh = N.dot(z) + x0
            f_train += 0.5 * float(np.sum(reg_lambda * d * d * xh * xh))
        out.append({'iters': int(iters[-1]), 'stop': stop,
                    'f_train': f_train,
                    'held_out': 0.5 * float(np.sum(r[w == 0.0] ** 2)),
                    'z': z, 'seconds': dt})
        if edges is not None:
            many = record_every is not None
            out[-1].update(_metrics_cpu(A, b, x0, N, w, states if many else [z], edges, many))
            if many:
                out[-1]['logged'] = [int(i) for i in iters]
    return out


def _batch_metrics(A_dev, layout, x0, b_dev, edges, chunk, states, many):
    """The metric dicts of a chunk's problems from one launch per 1024 states:
    states[j] are problem j's (host) states, each under its own mask
    (roww_ld = m)."""
    import torch
    from dev_metrics import MAX_STATES, fitted_flows, launch, metrics_from_cells
    m = A_dev.m
    owner = [j for j, zs in enumerate(states) for _ in zs]
    flat = [z for zs in states for z in zs]
    wd = torch.stack([torch.from_numpy(w).cuda() for w in chunk])
    cells = []
    for lo in range(0, len(flat), MAX_STATES):
        part = slice(lo, lo + MAX_STATES)
        ax = fitted_flows(A_dev, layout, x0, flat[part])
        roww = wd[torch.as_tensor(owner[part], device='cuda')].contiguous()
        cells.append(launch(ax, m, b_dev, roww, m, edges, m, ax.shape[0]))
    cells = np.concatenate(cells)
    out, at = [], 0
    for zs in states:
        mine = cells[at:at + len(zs)]
        at += len(zs)
        out.append(metrics_from_cells(mine if many else mine[0]))
    return out


def _kfold_batch(A, b, x0, block_sizes, masks, options, batch, edges=None, record_every=None):
    """The folds `batch` at a time on one device.BatchBB (balanced chunks,
    device.batch_groups); a fold's seconds is its chunk's time divided by the
    chunk's size.  edges: the link metrics too, a chunk's problems in one
    launch."""
    import _native
    from bsls_utils import x2z
    from device import BatchBB, batch_groups
    z0 = x2z(x0, block_sizes)
    out = []
    eng, lo = None, 0
    A_dev = b_dev = None
    many = record_every is not None
    for size in batch_groups(len(masks), batch):
        chunk = masks[lo:lo + size]
        lo += size
        t0 = time.time()
        if eng is None or eng.R != size:
            eng = BatchBB(A, [b] * size, block_sizes, row_weights=chunk, options=options, x0=x0)
        else:
            for j, w in enumerate(chunk):
                eng.set_row_weights(j, w)
        logs = [([], []) for _ in range(size)]

        def log(j, i, z, dt):
            logs[j][0].append(int(i))
            logs[j][1].append(z)
            return time.time()
        zs = eng.solve(z0=[z0] * size, **(dict(log=log, record_every=int(record_every))
                                          if many else {}))
        S, held = eng.scalars(), eng.held_out()
        dt = (time.time() - t0) / size
        for j in range(size):
            out.append({'iters': int(eng.iterations[j]),
                        'stop': _native.STOP_TEXT[int(eng.stop_reasons[j])],
                        'f_train': float(S[j, _native.S_FX]), 'held_out': held[j],
                        'z': zs[j], 'seconds': dt})
        if edges is not None:
            import torch
            from device import DeviceCSR
            if A_dev is None:
                A_dev = DeviceCSR(A)
                b_dev = torch.from_numpy(np.ascontiguousarray(b, dtype=np.float64)).cuda()
            states = [logs[j][1] if many else [zs[j]] for j in range(size)]
            dicts = _batch_metrics(A_dev, eng.layout, np.asarray(x0, dtype=np.float64), b_dev,
                                   edges, chunk, states, many)
            for j in range(size):
                out[j - size].update(dicts[j])
                if many:
                    out[j - size]['logged'] = logs[j][0]
    return out


def kfold(A, b, x0, N, block_sizes, k, options=None, device='gpu', engine=None, shuffle=False,
          seed=0, deterministic=None, batch=None, reg_lambda=0.0, reg_weights=None, masks=None,
          metrics=False, nbins=6, record_every=None):
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
    the default; batch buys lockstep fits that repeat bit for bit.

    reg_lambda / reg_weights: the reference's weighted L2 regulariser on every
    fold's fit (BBEngine.set_regulariser; main.solve_in_z_cpu on 'cpu');
    f_train is then the regularised objective, held_out stays the plain error
    of the held-out rows.  Not with batch (ValueError).  masks: the folds as
    0/1 vectors instead of kfold_masks(m, k) -- label_masks' -- k is then not
    used.

    metrics=True: each fold dict gains the reference's link metrics of its fit
    (CrossValidation.post_process, python/CrossValidation.py:186-274; device.
    metrics_from_cells): 'train' and 'test', {figure: value} for the figures
    of device.KEYS over the fold's train and held-out links, and 'train_bin' /
    'test_bin', {figure: [value per link class]} for the nbins + 1 classes by
    flow of device.link_classes(b, nbins) (edges from the whole b, as the
    reference).  On 'gpu' A x_hat and the sums stay on the device
    (BBEngine.link_metrics; with batch a chunk's problems in one launch, each
    under its own mask); on 'cpu' NumPy forms the same table.  With
    record_every=R as well the states BB.solve logs every R iterations are
    kept (on the device) and evaluated in one launch: every figure is then an
    array over them, and 'logged' lists their iterations -- the last entry is
    the final state's, what metrics=True alone reports."""
    from device import reg_lambda_check, reg_weights_check
    edges = None
    if metrics:
        from device import link_classes
        edges = link_classes(b, nbins)
    if record_every is not None:
        if not metrics:
            raise ValueError('record_every logs states for the metrics: it needs metrics=True')
        if isinstance(record_every, bool) or not isinstance(record_every, (int, np.integer)) \
                or record_every < 1:
            raise ValueError('record_every must be None or an int >= 1 (got %r)'
                             % (record_every,))
    reg_lambda = reg_lambda_check(reg_lambda)
    reg_weights = reg_weights_check(reg_weights, A.shape[1])
    if batch is not None and reg_lambda:
        raise ValueError('batch does not cover a regulariser: run the folds on one engine '
                         '(batch=None)')
    if batch is not None:
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) \
                or not 1 <= batch <= 8:
            raise ValueError('batch must be None or an int in 1..8 (got %r)' % (batch,))
    from bsls_utils import x2z
    block_sizes = np.asarray(block_sizes)
    masks = _fold_masks(A.shape[0], k, shuffle, seed, masks)
    if device == 'cpu':
        return _kfold_cpu(A, b, x0, N, block_sizes, masks, options, reg_lambda, reg_weights,
                          edges, record_every)
    if device != 'gpu':
        raise ValueError("device must be 'gpu' or 'cpu' (got %r)" % (device,))
    if batch is not None:
        return _kfold_batch(A, b, x0, block_sizes, masks, options, int(batch), edges,
                            record_every)
    import torch
    import _native
    from main import build_engine
    eng = engine
    if eng is None:
        eng = build_engine(A, b, x0, block_sizes, options=options, deterministic=deterministic,
                           row_weights=masks[0])
    before = eng.row_weights
    keep = (eng.P.max_iter, eng.P.opt_tol)
    reg_before, d_before = eng.reg_lambda, eng.reg_d
    if options is not None:
        eng.P.max_iter = int(options.get('max_iter', 300000))
        eng.P.opt_tol = float(options.get('opt_tol', 1e-6))
    z0 = x2z(x0, block_sizes)
    out = []
    try:
        if reg_lambda or reg_before:
            eng.set_regulariser(reg_lambda, reg_weights)
        for w in masks:
            t0 = time.time()
            eng.set_row_weights(w)
            logged, states = [], []
            if record_every is None:
                z = eng.solve(z0=z0).cpu().numpy().copy()
            else:
                def log(i, state, dt):
                    logged.append(int(i))
                    states.append(state)
                    return time.time()
                z = eng.solve(z0=z0, log=log, record_every=int(record_every),
                              to_host=False).cpu().numpy().copy()
            torch.cuda.synchronize()
            s = eng.scalars()
            out.append({'iters': int(eng.iterations),
                        'stop': _native.STOP_TEXT[int(eng.stop_reason)],
                        'f_train': float(s[_native.S_FX]), 'held_out': eng.held_out(),
                        'z': z, 'seconds': time.time() - t0})
            if metrics:
                out[-1].update(eng.link_metrics(states if states else None, edges=edges))
                if states:
                    out[-1]['logged'] = logged
    finally:
        eng.set_row_weights(before)
        eng.P.max_iter, eng.P.opt_tol = keep
        if reg_lambda or reg_before or eng.reg_d is not d_before:
            # an engine passed in gets its own lambda and d back
            eng.reg_d = d_before
            eng.set_regulariser(reg_before)
    return out


def kfold_path(A, b, x0, N, block_sizes, k, lambdas, reg_weights=None, options=None,
               device='gpu', engine=None, shuffle=False, seed=0, deterministic=None, masks=None,
               select='held_out'):
    """Choose lambda by cross-validation: kfold(..., reg_lambda=lam) for every
    lam of `lambdas`, all (lambda, fold) fits on ONE engine on 'gpu' (`engine`
    or one built here; changing lambda is one elementwise device op).  Returns
    {'lambdas', 'folds' (per lambda the fold dicts), 'held_out' (per lambda the
    mean held-out error), 'best' (the arg-min lambda, the first on a tie),
    'best_index', 'score', 'select'}.

    select: what 'best' is chosen by.  'held_out' (the default): the mean
    held-out error, 'score' = 'held_out'.  A figure of device.KEYS ('mean_GEH',
    'GEH_under_5', 'RMSE', ..): the folds run with metrics=True (nbins=6) and
    'score' is per lambda the folds' mean of test[select] at the final state --
    maximised for the GEH_under_* shares, minimised otherwise, the first on a
    tie."""
    from device import KEYS, reg_lambda_check
    from dev_metrics import MAXIMISED
    if select != 'held_out' and select not in KEYS:
        raise ValueError("select must be 'held_out' or one of %r (got %r)" % (KEYS, select))
    lams = [reg_lambda_check(l) for l in lambdas]
    if not lams:
        raise ValueError('kfold_path needs at least one lambda')
    block_sizes = np.asarray(block_sizes)
    masks = _fold_masks(A.shape[0], k, shuffle, seed, masks)
    eng = engine
    if device == 'gpu' and eng is None:
        from main import build_engine
        eng = build_engine(A, b, x0, block_sizes, options=options, deterministic=deterministic,
                           row_weights=masks[0], reg_weights=reg_weights)
    folds = [kfold(A, b, x0, N, block_sizes, k, options=options, device=device, engine=eng,
                   reg_lambda=lam, reg_weights=reg_weights, masks=masks,
                   metrics=select != 'held_out') for lam in lams]
    held = [float(np.mean([f['held_out'] for f in fs])) for fs in folds]
    score = list(held)
    if select != 'held_out':
        if any(f['test'] is None for fs in folds for f in fs):
            raise ValueError('select=%r needs held-out links in every fold' % (select,))
        score = [float(np.mean([f['test'][select] for f in fs])) for fs in folds]
    best = int(np.argmax(score) if select in MAXIMISED else np.argmin(score))
    return {'lambdas': lams, 'folds': folds, 'held_out': held, 'best': lams[best],
            'best_index': best, 'score': score, 'select': select}
