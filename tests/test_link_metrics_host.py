"""Host side of the link metrics (dev_metrics.py, cross_validation.kfold's
metrics=True, kfold_path's select): metrics_from_cells against a NumPy
restatement of the reference's metrics() (python/CrossValidation.py:193-214)
and its by-class table (:246-274), link_classes, every refusal, and the 'cpu'
device of kfold / kfold_path.  No GPU."""
import numpy as np
import pytest

from test_reg_host import small

EXACT = ('max_GEH', 'GEH_under_5', 'GEH_under_1', 'GEH_under_0.5', 'GEH_under_0.05')
FOLD_KEYS = {'iters', 'stop', 'f_train', 'held_out', 'z', 'seconds'}


# ---- the restatement --------------------------------------------------------------
def restate(ax, b):
    """metrics() of CrossValidation.py:193-214 on the rows given: ax (d, rows)
    holds A.dot(X) transposed, one state per row; every figure is an array
    over the d states."""
    ax = np.atleast_2d(np.asarray(ax, dtype=np.float64))
    with np.errstate(all='ignore'):
        diff = ax - b
        error = 0.5 * np.sum(diff * diff, axis=1)
        RMSE = np.sqrt(error / b.size)
        den = np.sum(b) / np.sqrt(b.size)
        plus = ax + b
        GEH = np.sqrt(2 * diff ** 2 / plus)
        return {'error': error, 'RMSE': RMSE, 'pRMSE': RMSE / den,
                'mean_GEH': np.mean(GEH, axis=1), 'max_GEH': np.max(GEH, axis=1),
                'GEH_under_5': np.mean(GEH < 5, axis=1), 'GEH_under_1': np.mean(GEH < 1, axis=1),
                'GEH_under_0.5': np.mean(GEH < 0.5, axis=1),
                'GEH_under_0.05': np.mean(GEH < 0.05, axis=1)}


def restate_all(ax, b, w, edges):
    """The four dicts of post_process for one fold: train / test over the rows
    with w != 0 / w == 0, and per class j = 1 .. len(edges) of np.digitize
    (:246-274) with None for both sets where either has no row."""
    from dev_metrics import KEYS
    ax = np.atleast_2d(np.asarray(ax, dtype=np.float64))
    tr, te = np.nonzero(w != 0)[0], np.nonzero(w == 0)[0]
    out = {'train': restate(ax[:, tr], b[tr]) if tr.size else None,
           'test': restate(ax[:, te], b[te]) if te.size else None}
    inds, indts = np.digitize(b[tr], edges), np.digitize(b[te], edges)
    train_bin, test_bin = {k: [] for k in KEYS}, {k: [] for k in KEYS}
    for j in range(1, len(edges) + 1):
        ind, indt = inds == j, indts == j
        if not ind.any() or not indt.any():
            for k in KEYS:
                train_bin[k].append(None)
                test_bin[k].append(None)
            continue
        for dst, m in ((train_bin, restate(ax[:, tr[ind]], b[tr[ind]])),
                       (test_bin, restate(ax[:, te[indt]], b[te[indt]]))):
            for k in KEYS:
                dst[k].append(m[k])
    out['train_bin'], out['test_bin'] = train_bin, test_bin
    return out


def recipe(m, seed=29):
    """(ax, b): flows b in [0.5, 50.5) and fitted flows whose GEH spreads over
    all four thresholds."""
    rs = np.random.RandomState(seed)
    b = 50 * rs.rand(m) ** 2 + 0.5
    ax = np.abs(b * (1 + 2 * rs.randn(m) * rs.rand(m) ** 3))
    return ax, b


def numpy_cells(ax, b, w, edges):
    """The table bsls_link_metrics defines, by NumPy: [state][set][class][9]."""
    ax = np.atleast_2d(np.asarray(ax, dtype=np.float64))
    edges = np.asarray(edges, dtype=np.float64)
    w = np.broadcast_to(np.ones(b.size) if w is None else w, ax.shape)
    cls = np.digitize(b, edges) if edges.size else np.zeros(b.size, dtype=np.int64)
    cells = np.zeros((ax.shape[0], 2, edges.size + 1, 9))
    with np.errstate(all='ignore'):
        for s in range(ax.shape[0]):
            diff = ax[s] - b
            d2 = diff ** 2
            geh = np.sqrt(2 * d2 / (ax[s] + b))
            for st in (0, 1):
                for c in range(edges.size + 1):
                    rows = ((w[s] == 0) == bool(st)) & (cls == c)
                    if rows.any():
                        g = geh[rows]
                        cells[s, st, c] = [rows.sum(), d2[rows].sum(), g.sum(), g.max(),
                                           (g < 5).sum(), (g < 1).sum(), (g < 0.5).sum(),
                                           (g < 0.05).sum(), b[rows].sum()]
    return cells


def same(got, ref, key, what='', exact=EXACT):
    """Counts and max_GEH exactly, sums to 1e-12 max(1, |ref|); arrays or floats."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, key, got.shape, ref.shape)
    if key in exact:
        assert np.array_equal(got, ref, equal_nan=True), (what, key, got, ref)
    else:
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(got), nan), (what, key, got, ref)
        with np.errstate(invalid='ignore'):                  # (inf - inf, settled below)
            ok = np.abs(got - ref)[~nan] <= 1e-12 * np.maximum(1.0, np.abs(ref[~nan]))
        inf = np.isinf(ref)
        assert np.all(ok | (got[~nan] == ref[~nan])) and np.array_equal(got[inf], ref[inf]), \
            (what, key, got, ref)


def same_dicts(got, ref, scalar, what='', exact=EXACT):
    """The four dicts against restate_all's; scalar: got holds floats (one
    state) where the restatement holds arrays of one entry."""
    from dev_metrics import KEYS
    assert {'train', 'test', 'train_bin', 'test_bin'} <= set(got)
    pick = (lambda v: v[0]) if scalar else (lambda v: v)
    for name in ('train', 'test'):
        if ref[name] is None:
            assert got[name] is None, (what, name)
            continue
        assert set(got[name]) == set(KEYS)
        for k in KEYS:
            if scalar:
                assert isinstance(got[name][k], float), (what, name, k)
            same(got[name][k], pick(ref[name][k]), k, what + name, exact)
    for name in ('train_bin', 'test_bin'):
        assert set(got[name]) == set(KEYS)
        for k in KEYS:
            assert len(got[name][k]) == len(ref[name][k])
            for j, (g, r) in enumerate(zip(got[name][k], ref[name][k])):
                if r is None:
                    assert g is None, (what, name, k, j)
                else:
                    assert g is not None, (what, name, k, j)
                    same(g, pick(r), k, '%s%s[%d]' % (what, name, j), exact)


# ---- metrics_from_cells ------------------------------------------------------------
def test_recipe_splits_every_threshold():
    """The input recipe's counts, as stated with it."""
    want = {64: (59, 43, 36, 24), 257: (248, 175, 141, 73), 1319: (1253, 901, 754, 362)}
    for m, counts in want.items():
        ax, b = recipe(m)
        geh = np.sqrt(2 * (ax - b) ** 2 / (ax + b))
        assert tuple(int(np.sum(geh < t)) for t in (5, 1, 0.5, 0.05)) == counts
        cls = np.digitize(b, np.histogram(b, 6)[1])
        w = np.arange(m) % 3 != 0
        assert np.sum(cls == 0) == 0 and np.sum(cls == 7) == 1
        for c in range(1, 7):
            assert np.any(cls[w] == c) and np.any(cls[~w] == c)


@pytest.mark.parametrize('states', [1, 3])
def test_metrics_from_cells(states):
    from dev_metrics import KEYS, link_classes, metrics_from_cells
    ax, b = recipe(257)
    m = b.size
    axs = np.stack([ax * (1 + 0.01 * s) for s in range(states)])
    w = (np.arange(m) % 3 != 0).astype(np.float64)
    edges = link_classes(b)
    got = metrics_from_cells(numpy_cells(axs, b, w, edges))
    ref = restate_all(axs, b, w, edges)
    same_dicts(got, ref, scalar=False)
    assert all(np.shape(got['test'][k]) == (states,) for k in KEYS)
    # class 7 (b == max) holds one row: None for both sets; classes 1..6 are filled
    assert all(got[n][k][6] is None for n in ('train_bin', 'test_bin') for k in KEYS)
    assert all(got[n][k][j] is not None for n in ('train_bin', 'test_bin') for k in KEYS
               for j in range(6))
    # a table of one state without the states axis gives floats
    one = metrics_from_cells(numpy_cells(axs[:1], b, w, edges)[0])
    same_dicts(one, restate_all(axs[:1], b, w, edges), scalar=True)


def test_metrics_from_cells_class0_and_empty_set():
    from dev_metrics import KEYS, link_classes, metrics_from_cells
    ax, b = recipe(257)
    w = (np.arange(b.size) % 3 != 0).astype(np.float64)
    # without the first two edges the rows of the first two bins are class 0:
    # in the totals, in no by-class entry
    edges = link_classes(b)[2:]
    cells = numpy_cells(ax, b, w, edges)[0]
    assert cells[0, 0, 0] > 50 and cells[1, 0, 0] > 25
    got = metrics_from_cells(cells)
    same_dicts(got, restate_all(ax, b, w, edges), scalar=True)
    assert len(got['train_bin']['RMSE']) == edges.size == 5
    assert got['train']['error'] > sum(v for v in got['train_bin']['error'] if v is not None)
    # no held-out row at all: test is None, and so is every by-class entry of both sets
    ones = np.ones(b.size)
    got = metrics_from_cells(numpy_cells(ax, b, ones, edges)[0])
    same_dicts(got, restate_all(ax, b, ones, edges), scalar=True)
    assert got['test'] is None and got['train'] is not None
    assert all(v is None for n in ('train_bin', 'test_bin') for k in KEYS for v in got[n][k])
    # ... and no train row
    got = metrics_from_cells(numpy_cells(ax, b, 0 * ones, edges)[0])
    assert got['train'] is None and got['test']['RMSE'] > 0
    with pytest.raises(ValueError, match='cells must be'):
        metrics_from_cells(np.zeros((2, 3, 8)))
    # states whose masks differ cannot share one dict
    mixed = np.stack([numpy_cells(ax, b, ones, edges)[0], numpy_cells(ax, b, w, edges)[0]])
    with pytest.raises(ValueError, match='share their masks'):
        metrics_from_cells(mixed)


def test_metrics_from_cells_nonfinite():
    """A NaN / inf cell gives NaN / inf figures as NumPy's, and stays in its class."""
    from dev_metrics import metrics_from_cells
    b = np.array([1.0, 1.0, 5.0, 5.0, 9.0, 9.0, 0.0, -1.0])
    ax = np.array([1.5, 0.5, 5.5, 4.0, 9.5, 8.0, 0.0, 1.0])
    w = np.array([1.0, 0, 1, 0, 1, 0, 1, 0])
    edges = np.array([-2.0, 0.5, 3.0, 7.0])
    got = metrics_from_cells(numpy_cells(ax, b, w, edges)[0])
    same_dicts(got, restate_all(ax, b, w, edges), scalar=True)
    assert np.isnan(got['train_bin']['mean_GEH'][0]) and np.isinf(got['test_bin']['max_GEH'][0])
    assert np.isfinite(got['train_bin']['mean_GEH'][1]) and np.isnan(got['train']['max_GEH'])


def test_link_classes():
    from device import KEYS, link_classes
    _, b = recipe(1319)
    assert np.array_equal(link_classes(b), np.histogram(b, bins=6)[1])
    assert np.array_equal(link_classes(b, 3), np.histogram(b, bins=3)[1])
    assert link_classes(b, 14).size == 15
    assert KEYS == ['mean_GEH', 'RMSE', 'GEH_under_5', 'GEH_under_1', 'GEH_under_0.05',
                    'GEH_under_0.5', 'max_GEH', 'pRMSE', 'error']
    for bad in (0, 15, 2.0, True):
        with pytest.raises(ValueError, match='nbins'):
            link_classes(b, bad)
    with pytest.raises(ValueError, match='finite'):
        link_classes(np.array([1.0, np.nan]))


def test_link_metrics_refusals(monkeypatch):
    """Every ValueError of link_metrics comes before the device is touched."""
    import _native
    import dev_images
    from device import link_metrics
    monkeypatch.setattr(_native, 'lib', lambda: pytest.fail('the library was touched'))
    monkeypatch.setattr(dev_images, '_torch', lambda: pytest.fail('torch was touched'))
    ax, b = recipe(64)
    for bad in (np.inf, -np.inf, np.nan):
        b2 = b.copy()
        b2[5] = bad
        with pytest.raises(ValueError, match='b must be finite'):
            link_metrics(ax, b2)
    with pytest.raises(ValueError, match='edges must be finite'):
        link_metrics(ax, b, edges=[1.0, np.nan])
    with pytest.raises(ValueError, match='edges must be finite'):
        link_metrics(ax, b, edges=[1.0, np.inf])
    with pytest.raises(ValueError, match='non-decreasing'):
        link_metrics(ax, b, edges=[1.0, 3.0, 2.0])
    with pytest.raises(ValueError, match='at most 15'):
        link_metrics(ax, b, edges=np.arange(16.0))
    with pytest.raises(ValueError, match='ax must be'):
        link_metrics(ax[:-1], b)
    with pytest.raises(ValueError, match='ax must be'):
        link_metrics(np.zeros((2, 2, 64)), b)
    with pytest.raises(ValueError, match='ax must be'):
        link_metrics(np.zeros((64, 2)), b)
    with pytest.raises(ValueError, match='states'):
        link_metrics(np.zeros((1025, 64)), b)
    with pytest.raises(ValueError, match='row_weights must be'):
        link_metrics(ax, b, row_weights=np.ones(63))
    with pytest.raises(ValueError, match='row_weights must be'):
        link_metrics(np.zeros((3, 64)), b, row_weights=np.ones((2, 64)))
    with pytest.raises(ValueError, match='at least one link'):
        link_metrics(np.zeros(0), np.zeros(0))


# ---- kfold / kfold_path on the cpu device ----------------------------------------------
OPTS = {'max_iter': 5, 'opt_tol': 1e-30}


@pytest.fixture(scope='module')
def tiny(orc):
    A, b, sizes, _ = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    return A, b, sizes, P['x0'], P['N']


def test_kfold_cpu_metrics(tiny):
    from cross_validation import kfold, kfold_masks
    from device import link_classes
    A, b, sizes, x0, N = tiny
    plain = kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu')
    assert all(set(f) == FOLD_KEYS for f in plain)           # today's dicts, nothing more
    folds = kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', metrics=True)
    edges = link_classes(b)
    for f, f0, w in zip(folds, plain, kfold_masks(500, 2)):
        assert set(f) == FOLD_KEYS | {'train', 'test', 'train_bin', 'test_bin'}
        assert np.array_equal(f['z'], f0['z']) and f['held_out'] == f0['held_out']
        ax = A.dot(N.dot(f['z']) + x0)
        same_dicts(f, restate_all(ax, b, w, edges), scalar=True)
        # the reference's test error is the fold's held-out error
        assert abs(f['test']['error'] - f['held_out']) <= 1e-12 * f['held_out']
    # other classes
    f3 = kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', metrics=True, nbins=3)[0]
    assert len(f3['test_bin']['RMSE']) == 4
    same_dicts(f3, restate_all(A.dot(N.dot(f3['z']) + x0), b, kfold_masks(500, 2)[0],
                               link_classes(b, 3)), scalar=True)


def test_kfold_cpu_logged_states(tiny):
    from cross_validation import kfold
    from dev_metrics import KEYS
    A, b, sizes, x0, N = tiny
    last = kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', metrics=True)
    folds = kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', metrics=True,
                  record_every=2)
    for f, f1 in zip(folds, last):
        assert f['logged'] == [0, 2, 4, 5]                   # BB.solve's log, python/BB.py:10,40-44
        for k in KEYS:
            assert np.shape(f['test'][k]) == (4,) and f['test'][k][-1] == f1['test'][k]
            assert f['train_bin'][k][0][-1] == f1['train_bin'][k][0]
        assert f['train']['error'][0] > f['train']['error'][-1]
    with pytest.raises(ValueError, match='needs metrics=True'):
        kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', record_every=2)
    with pytest.raises(ValueError, match='record_every must be'):
        kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', metrics=True, record_every=0)
    with pytest.raises(ValueError, match='nbins'):
        kfold(A, b, x0, N, sizes, 2, options=OPTS, device='cpu', metrics=True, nbins=15)


def test_kfold_path_select(tiny):
    from cross_validation import kfold_path
    A, b, sizes, x0, N = tiny
    lams = [3.7e5, 0.0, 100.0, 0.0]
    base = kfold_path(A, b, x0, N, sizes, 2, lams, options=OPTS, device='cpu')
    assert base['select'] == 'held_out' and base['score'] == base['held_out']
    assert base['best_index'] == int(np.argmin(base['held_out']))
    assert all(set(f) == FOLD_KEYS for fs in base['folds'] for f in fs)
    for select, arg in (('mean_GEH', np.argmin), ('RMSE', np.argmin), ('GEH_under_1', np.argmax),
                        ('GEH_under_0.05', np.argmax)):
        path = kfold_path(A, b, x0, N, sizes, 2, lams, options=OPTS, device='cpu',
                          select=select)
        score = [float(np.mean([f['test'][select] for f in fs])) for fs in path['folds']]
        assert path['select'] == select and path['score'] == score
        assert score[1] == score[3]                          # the two lambda = 0 tie
        assert path['best_index'] == int(arg(score)) and path['best'] == lams[path['best_index']]
        assert path['held_out'] == base['held_out']
        assert all(np.array_equal(f['z'], f0['z']) for fs, fs0 in zip(path['folds'], base['folds'])
                   for f, f0 in zip(fs, fs0))
    # the first on a tie, for a minimised and a maximised figure
    for select in ('max_GEH', 'GEH_under_5'):
        tie = kfold_path(A, b, x0, N, sizes, 2, [0.0, 0.0], options=OPTS, device='cpu',
                         select=select)
        assert tie['score'][0] == tie['score'][1] and tie['best_index'] == 0
    with pytest.raises(ValueError, match='select must be'):
        kfold_path(A, b, x0, N, sizes, 2, lams, options=OPTS, device='cpu', select='GEH')


def test_main_flags():
    import argparse
    import main
    args = main.parser().parse_args(['--cv', '3', '--cv-metrics', '--cv-bins', '4'])
    assert args.cv == 3 and args.cv_metrics is True and args.cv_bins == 4
    args = main.parser().parse_args([])
    assert args.cv_metrics is False and args.cv_bins == 6
    base = dict(noise=0, file='unused.mat', log='WARN', init=False, eq='CP', method='BB')
    with pytest.raises(ValueError, match='--cv-metrics needs --cv'):
        main.main(args=argparse.Namespace(cv_metrics=True, **base))
    with pytest.raises(ValueError, match='--cv-bins'):
        main.main(args=argparse.Namespace(cv=3, cv_metrics=True, cv_bins=15, **base))
