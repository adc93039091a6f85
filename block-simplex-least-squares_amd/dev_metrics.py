"""Link metrics of a fit by set (train / held out) and link class by flow:
CrossValidation.post_process's metrics() (python/CrossValidation.py:193-214)
and its by-class table (:119-121, 246-274).

The device reduces (A x_hat, b, mask, class edges) to one table of sums per
state (bsls_link_metrics, csrc/metrics.hip): cells[state][set][class][value]
with the values V_*; metrics_from_cells turns the table into the reference's
dicts on the host.  Importing this module needs neither a GPU nor torch.
"""
import numpy as np

import _native
from _native import check, ptr, stream_handle

# the reference's figures, in its spelling (CrossValidation.py:15)
KEYS = ['mean_GEH', 'RMSE', 'GEH_under_5', 'GEH_under_1', 'GEH_under_0.05', 'GEH_under_0.5',
        'max_GEH', 'pRMSE', 'error']
# the figures a larger value of is the better fit (kfold_path's select)
MAXIMISED = ('GEH_under_5', 'GEH_under_1', 'GEH_under_0.5', 'GEH_under_0.05')

# cells[..., v] (enum BSLS_LM_*, include/bsls_hip.h)
(V_COUNT, V_SSQ, V_SUM_GEH, V_MAX_GEH, V_UNDER_5, V_UNDER_1, V_UNDER_0_5, V_UNDER_0_05,
 V_SUM_B) = range(9)
NV = 9
MAX_EDGES = 15           # BSLS_LM_MAX_EDGES
MAX_STATES = 1024


def _host(a):
    """a (host or device array) as a host float64 ndarray."""
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def _b_check(b):
    b = np.ascontiguousarray(_host(b).reshape(-1))
    if b.size < 1:
        raise ValueError('link metrics need at least one link')
    if not np.all(np.isfinite(b)):
        raise ValueError('b must be finite (no NaN or inf)')
    return b


def edges_check(edges):
    """The class edges as a host float64 vector: None is none (one class); at
    most 15, finite and non-decreasing, else ValueError."""
    if edges is None:
        return np.zeros(0)
    e = np.ascontiguousarray(_host(edges).reshape(-1))
    if e.size > MAX_EDGES:
        raise ValueError('at most %d class edges (got %d)' % (MAX_EDGES, e.size))
    if not np.all(np.isfinite(e)):
        raise ValueError('class edges must be finite (no NaN or inf)')
    if np.any(np.diff(e) < 0):
        raise ValueError('class edges must be non-decreasing')
    return e


def link_classes(b, nbins=6):
    """The nbins + 1 edges of the link classes by flow: np.histogram(b,
    bins=nbins)[1] (CrossValidation.py:119-121).  Row i's class is then
    np.digitize(b_i, edges): 1..nbins inside, nbins + 1 for b == max."""
    if isinstance(nbins, bool) or not isinstance(nbins, (int, np.integer)) \
            or not 1 <= nbins <= MAX_EDGES - 1:
        raise ValueError('nbins must be an int in 1..%d (got %r)' % (MAX_EDGES - 1, nbins))
    return np.histogram(_b_check(b), bins=int(nbins))[1]


def launch(ax, ax_ld, b, roww, roww_ld, edges, m, nstates):
    """bsls_link_metrics on device tensors (edges: a checked host vector);
    returns the (nstates, 2, nedges + 1, NV) table as a host ndarray."""
    from dev_images import _torch
    torch = _torch()
    L = _native.lib()
    ne = int(edges.size)
    if not 1 <= nstates <= MAX_STATES:
        raise ValueError('1..%d states to a launch (got %d)' % (MAX_STATES, nstates))
    e_dev = torch.from_numpy(edges).cuda() if ne else None
    out = torch.empty(nstates * 2 * (ne + 1) * NV, dtype=torch.float64, device='cuda')
    work = torch.empty(max(1, L.bsls_link_metrics_work_size(m, nstates, ne)), dtype=torch.uint8,
                       device='cuda')
    check(L.bsls_link_metrics(ptr(ax), int(ax_ld), ptr(b), ptr(roww), int(roww_ld), ptr(e_dev),
                              ne, int(m), int(nstates), ptr(out), ptr(work), stream_handle()),
          'bsls_link_metrics')
    return out.cpu().numpy().reshape(nstates, 2, ne + 1, NV)


def fitted_flows(A_dev, layout, x0, zs):
    """A (x0 + N z) for every z of zs as a (len(zs), m) device tensor, on the
    general CSR kernel (device.DeviceCSR A_dev) and the block layout's N: what
    an engine without BBEngine.apply_A_x (device.BatchBB) hands to launch()."""
    from dev_images import _torch
    torch = _torch()
    L = _native.lib()
    x0 = torch.as_tensor(x0, dtype=torch.float64).cuda().reshape(-1)
    ax = torch.empty(len(zs), A_dev.m, dtype=torch.float64, device='cuda')
    xh = torch.empty(layout.n, dtype=torch.float64, device='cuda')
    for s, z in enumerate(zs):
        z = torch.as_tensor(z, dtype=torch.float64).cuda().reshape(-1)
        if z.numel() != layout.nz:
            raise ValueError('z has %d entries, expected %d' % (z.numel(), layout.nz))
        check(L.bsls_n_apply(ptr(xh), ptr(z), ptr(layout.xstarts), layout.p, layout.n, 0,
                             stream_handle()), 'bsls_n_apply')
        xh += x0
        A_dev.matvec(xh, out=ax[s])
    return ax


def link_metrics(ax, b, row_weights=None, edges=None):
    """The table of sums behind the reference's metrics, on the device.

    ax: A x_hat, (m,) or (nstates, m); b: (m,); row_weights: None (every link
    is train), (m,) (one mask for all states) or (nstates, m); a link is held
    out where its weight is 0.  edges: None (one class) or at most 15
    non-decreasing values, link_classes(b)'s.  Host or device arrays.  Returns
    cells[set][class][value] for a 1-D ax, else cells[state][set][class][value]
    (host ndarray; the values are V_*; class = np.digitize(b, edges)).
    ValueError before anything is launched: b or edges not finite, edges
    decreasing or more than 15, shapes that do not agree."""
    bh = _b_check(b)
    m = int(bh.size)
    e = edges_check(edges)
    shape = tuple(getattr(ax, 'shape', np.shape(ax)))
    if len(shape) not in (1, 2) or shape[-1] != m:
        raise ValueError('ax must be (m,) or (nstates, m) with m = %d links (got %r)'
                         % (m, shape))
    nstates = 1 if len(shape) == 1 else int(shape[0])
    if not 1 <= nstates <= MAX_STATES:
        raise ValueError('1..%d states to a launch (got %d)' % (MAX_STATES, nstates))
    wshape = None if row_weights is None else tuple(getattr(row_weights, 'shape',
                                                            np.shape(row_weights)))
    if wshape is not None and wshape not in ((m,), (nstates, m)):
        raise ValueError('row_weights must be None, (m,) or (nstates, m) = (%d, %d) (got %r)'
                         % (nstates, m, wshape))
    from dev_images import _torch
    torch = _torch()

    def dev(a):
        return torch.as_tensor(a, dtype=torch.float64).cuda().contiguous()
    axd = dev(ax)
    wd = None if row_weights is None else dev(row_weights)
    # (a (1, m) mask of a one-state launch is the shared form)
    roww_ld = m if wd is not None and wd.dim() == 2 and nstates > 1 else 0
    cells = launch(axd, m, dev(bh), wd, roww_ld, e, m, nstates)
    return cells[0] if len(shape) == 1 else cells


def _figures(v):
    """The reference's metrics() (CrossValidation.py:193-214) from one cell of
    sums v[..., NV]; the count must be positive."""
    cnt = v[..., V_COUNT]
    with np.errstate(all='ignore'):
        error = 0.5 * v[..., V_SSQ]
        rmse = np.sqrt(error / cnt)
        den = v[..., V_SUM_B] / np.sqrt(cnt)
        out = {'error': error, 'RMSE': rmse, 'pRMSE': rmse / den,
               'mean_GEH': v[..., V_SUM_GEH] / cnt, 'max_GEH': v[..., V_MAX_GEH] + 0.0,
               'GEH_under_5': v[..., V_UNDER_5] / cnt, 'GEH_under_1': v[..., V_UNDER_1] / cnt,
               'GEH_under_0.5': v[..., V_UNDER_0_5] / cnt,
               'GEH_under_0.05': v[..., V_UNDER_0_05] / cnt}
    if v.ndim == 1:
        out = {k: float(x) for k, x in out.items()}
    return out


def _empty(cnt):
    """Whether a cell holds no link; the states of one table share that."""
    cnt = np.atleast_1d(cnt)
    if np.any((cnt == 0) != (cnt[0] == 0)):
        raise ValueError('the states of one table must share their masks: a cell is empty at '
                         'some states only (convert such states one at a time)')
    return bool(cnt[0] == 0)


def metrics_from_cells(cells):
    """The reference's dicts from a table of link_metrics: {'train', 'test',
    'train_bin', 'test_bin'}.  train / test: {key: figure} for every key of
    KEYS over all links of the set -- the classes added in class order, class 0
    (b below the first edge) included -- or None for an empty set.  *_bin:
    {key: [figure per class 1..nedges]}, an entry None for both sets wherever
    either set has no link of that class (CrossValidation.py:253-262).
    error = 0.5 sum d2, RMSE = sqrt(error / count), pRMSE = RMSE / (sum b /
    sqrt(count)), mean_GEH, max_GEH, GEH_under_* = counts / count.  A table of
    one state (3-D) gives floats; one with a states axis (4-D) arrays over the
    states, as the reference's over its logged iterations."""
    cells = np.asarray(cells, dtype=np.float64)
    if cells.ndim not in (3, 4) or cells.shape[-1] != NV or cells.shape[-3] != 2:
        raise ValueError('cells must be ([nstates,] 2, classes, %d) (got %r)'
                         % (NV, cells.shape))
    if cells.ndim == 3:
        sets = [cells[0], cells[1]]
    else:
        sets = [cells[:, 0], cells[:, 1]]
    ncls = cells.shape[-2]
    out = {}
    for name, S in zip(('train', 'test'), sets):
        # (S: [..., class, value]) the set's totals, the classes in order
        tot = np.array(S[..., 0, :], dtype=np.float64, copy=True)
        for c in range(1, ncls):
            x = S[..., c, :]
            mx = np.maximum(tot[..., V_MAX_GEH], x[..., V_MAX_GEH])    # (NaN propagates)
            tot = tot + x
            tot[..., V_MAX_GEH] = mx
        out[name] = None if _empty(tot[..., V_COUNT]) else _figures(tot)
    bins = {'train': {k: [] for k in KEYS}, 'test': {k: [] for k in KEYS}}
    for c in range(1, ncls):
        either = any(_empty(S[..., c, V_COUNT]) for S in sets)
        for name, S in zip(('train', 'test'), sets):
            fig = None if either else _figures(S[..., c, :])
            for k in KEYS:
                bins[name][k].append(None if fig is None else fig[k])
    out['train_bin'], out['test_bin'] = bins['train'], bins['test']
    return out
