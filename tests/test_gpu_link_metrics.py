"""The link metrics on the device (bsls_link_metrics, csrc/metrics.hip;
BBEngine.link_metrics; cross_validation.kfold(metrics=True)) against the NumPy
restatement of python/CrossValidation.py:193-214, 246-274 kept in
test_link_metrics_host.py.  Counts and max_GEH are compared exactly, sums to
1e-12 max(1, |ref|) (the project's bound for reordered sums).

Where A x_hat comes from the device (the engine and kfold tests) a GEH within
rounding of a threshold could fall on either side, so those tests first assert,
on the NumPy side, that no row's GEH lies within 1e-9 relative of a threshold,
and that no b lies within 1e-9 relative of a class edge without being that
edge: b is the same double on both sides, so a b equal to an edge (the
smallest and the largest always are, the edges being np.histogram's) is
classified alike; no row is left out.  max_GEH is a function of A x_hat like
the sums, so against SciPy's A x_hat it is held to the sums' bound; it is
compared exactly, with the counts, where NumPy is given the A x_hat the kernel
read (the C ABI tests, and test_engine through apply_A_x, whose A x_hat is in
turn held to 1e-12 of SciPy's).  Needs an MI355X."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sps

from test_gpu_row_weights import small
from test_link_metrics_host import (FOLD_KEYS, numpy_cells, recipe, restate_all, same_dicts)

pytestmark = pytest.mark.gpu

GUARD = 16
ROWS = 512                      # rows of a workgroup (csrc/metrics.hip LM_ROWS)
COUNTS = [0, 4, 5, 6, 7]        # BSLS_LM_COUNT, UNDER_*
SUMS = [1, 2, 8]                # SSQ, SUM_GEH, SUM_B
MAX = 3
THRESHOLDS = (5.0, 1.0, 0.5, 0.05)
# exact against SciPy's A x_hat when the kernel read the device's: the counts
SHARES = ('GEH_under_5', 'GEH_under_1', 'GEH_under_0.5', 'GEH_under_0.05')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def launch(ax, b, roww=None, edges=(), ax_ld=None, roww_ld=0, repeat=1):
    """bsls_link_metrics through the C ABI on host arrays: ax (nstates, m) is
    laid out with leading dimension ax_ld, roww (m,) or (nstates, m) with
    roww_ld; out and work sit between GUARD entries of 7.5, checked after
    every launch.  Returns the list of `repeat` tables [state][set][class][9]."""
    import torch
    import _native
    L = _native.lib()
    ax = np.atleast_2d(np.asarray(ax, dtype=np.float64))
    ns, m = ax.shape
    edges = np.asarray(edges, dtype=np.float64)
    ne = edges.size
    ax_ld = m if ax_ld is None else ax_ld
    buf = np.full(ns * ax_ld, -777.0)
    for s in range(ns):
        buf[s * ax_ld:s * ax_ld + m] = ax[s]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    d_ax, d_b = dev(buf), dev(b)
    d_w = None
    if roww is not None:
        roww = np.atleast_2d(np.asarray(roww, dtype=np.float64))
        ld = max(roww_ld, m)
        wb = np.full(roww.shape[0] * ld, 1.0)
        for s in range(roww.shape[0]):
            wb[s * ld:s * ld + m] = roww[s]
        d_w = dev(wb)
    d_e = dev(edges) if ne else None
    nout = ns * 2 * (ne + 1) * 9
    wbytes = L.bsls_link_metrics_work_size(m, ns, ne)
    assert wbytes == -(-m // ROWS) * ns * 2 * (ne + 1) * 9 * 8
    out = torch.full((nout + 2 * GUARD,), 7.5, dtype=torch.float64, device='cuda')
    work = torch.full((wbytes // 8 + 2 * GUARD,), 7.5, dtype=torch.float64, device='cuda')
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 8 * off) if t is not None else None
    res = []
    for _ in range(repeat):
        rc = L.bsls_link_metrics(P(d_ax), ax_ld, P(d_b), P(d_w), roww_ld, P(d_e), ne, m, ns,
                                 P(out, GUARD), P(work, GUARD), _native.stream_handle())
        assert rc == 0, rc
        torch.cuda.synchronize()
        o, w = out.cpu().numpy(), work.cpu().numpy()
        for g in (o[:GUARD], o[-GUARD:], w[:GUARD], w[-GUARD:]):
            assert np.all(g == 7.5)
        assert not np.any(w[GUARD:-GUARD] == 7.5)          # work is written in full
        res.append(o[GUARD:-GUARD].reshape(ns, 2, ne + 1, 9).copy())
    return res


def compare(got, ref, parity, tag):
    """Counts and the max exactly, the sums to 1e-12; an empty cell is nine +0.0."""
    assert got.shape == ref.shape
    assert np.array_equal(got[..., COUNTS], ref[..., COUNTS]), tag
    assert np.array_equal(got[..., MAX], ref[..., MAX], equal_nan=True), tag
    g, r = got[..., SUMS], ref[..., SUMS]
    fin = np.isfinite(r)
    assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(g[~fin & ~np.isnan(r)],
                                                                       r[~fin & ~np.isnan(r)])
    err = float(np.max(np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))))
    parity(tag, err, 1e-12)
    empty = ref[..., 0] == 0
    assert np.all(bits(got[empty]) == 0), tag
    return err


def edge_sets(b):
    """nedges 0, 1, 7 and 15."""
    return [np.zeros(0), np.array([np.median(b)]), np.histogram(b, 6)[1], np.histogram(b, 14)[1]]


# ---- 1. the kernel through the C ABI ----------------------------------------------
# m = 1, one wave, 257 (a second segment of 32 rows, partly used), 1319 (three
# workgroups), ROWS + 1 (a last workgroup of one row) and 5 ROWS + 39 (a partly
# filled one)
@pytest.mark.parametrize('m', [1, 64, 257, 1319, ROWS + 1, 5 * ROWS + 39])
def test_kernel_abi(cuda, parity, m):
    ax, b = recipe(m)
    masks = {'none': None, 'mod3': (np.arange(m) % 3 != 0).astype(np.float64),
             'zero': np.zeros(m), 'half': np.full(m, 0.5)}
    for edges in edge_sets(b):
        for name, w in masks.items():
            runs = launch(ax, b, w, edges, repeat=3)
            assert np.array_equal(bits(runs[0]), bits(runs[1]))
            assert np.array_equal(bits(runs[0]), bits(runs[2]))
            ref = numpy_cells(ax, b, w, edges)
            compare(runs[0], ref, parity, 'lm_abi_%d_%d_%s' % (m, edges.size, name))
            want = {'none': (m, 0), 'mod3': (m - (m + 2) // 3, (m + 2) // 3), 'zero': (0, m),
                    'half': (m, 0)}[name]                   # (a weight of 0.5 is train)
            assert (runs[0][0, 0, :, 0].sum(), runs[0][0, 1, :, 0].sum()) == want


# ---- 2. boundaries ---------------------------------------------------------------------
def test_boundaries(cuda):
    edges = np.array([1.0, 2.0, 4.0])
    #          on an edge  below   last edge  GEH == 1   GEH == 5    ax == b   above all
    b = np.array([1.0,      0.25,   4.0,       0.5,       12.5,       2.0,      9.0])
    ax = np.array([1.25,    0.5,    4.5,       1.5,       37.5,       2.0,      9.5])
    cells = launch(ax, b, None, edges)[0][0]
    ref = numpy_cells(ax, b, None, edges)[0]
    assert np.array_equal(cells[..., COUNTS], ref[..., COUNTS])
    assert np.array_equal(cells[..., MAX], ref[..., MAX])
    tr = cells[0]
    assert list(tr[:, 0]) == [2.0, 1.0, 1.0, 3.0]      # classes 0 .. 3: {0.25, 0.5}, {1}, {2}, {4, 12.5, 9}
    # class 0: (0.5, 0.25) and (1.5, 0.5), whose GEH is exactly 1: under 5, not under 1
    # (the other row's GEH is 0.408)
    assert tr[0, MAX] == 1.0 and list(tr[0, 4:8]) == [2.0, 1.0, 1.0, 0.0]
    # class 2: ax == b, GEH 0, under all four
    assert tr[2, MAX] == 0.0 and list(tr[2, 4:8]) == [1.0, 1.0, 1.0, 1.0] and tr[2, 1] == 0.0
    # class 3 = nedges holds b == edges[-1], and (37.5, 12.5) with GEH exactly 5: under none
    assert tr[3, MAX] == 5.0 and tr[3, 4] == 2.0
    only = launch(np.array([37.5]), np.array([12.5]), None, edges)[0][0]
    assert list(only[0, 3, :8]) == [1.0, 625.0, 5.0, 5.0, 0.0, 0.0, 0.0, 0.0]


# ---- 3. non-finite rows stay in their cell -----------------------------------------------
def test_nonfinite_confined(cuda, parity):
    ax, b = recipe(257)
    # b of the three rows is 0, -1 and 1: with a first edge of 1.25 they are
    # all class 0, train, beside the recipe's train rows with b < 1.25
    edges = np.concatenate(([1.25], np.histogram(b, 6)[1][1:]))
    w = (np.arange(257) % 3 != 0).astype(np.float64)
    base = launch(ax, b, w, edges)[0]
    assert np.all(np.isfinite(base)) and base[0, 0, 0, 0] > 0 and base[0, 1, 0, 0] > 0
    ax2 = np.concatenate((ax, [0.0, 1.0, -3.0]))                   # NaN, +inf, NaN
    b2 = np.concatenate((b, [0.0, -1.0, 1.0]))
    w2 = np.concatenate((w, [1.0, 1.0, 1.0]))
    with np.errstate(all='ignore'):
        geh = np.sqrt(2 * (ax2[-3:] - b2[-3:]) ** 2 / (ax2[-3:] + b2[-3:]))
    assert np.isnan(geh[0]) and geh[1] == np.inf and np.isnan(geh[2])
    got = launch(ax2, b2, w2, edges)[0]
    compare(got, numpy_cells(ax2, b2, w2, edges), parity, 'lm_nonfinite')
    cell = got[0, 0, 0]
    assert cell[0] == base[0, 0, 0, 0] + 3 and np.isnan(cell[2]) and np.isnan(cell[MAX])
    assert np.all(np.isfinite(cell[[0, 1, 4, 5, 6, 7, 8]]))
    assert np.array_equal(cell[4:8], base[0, 0, 0, 4:8])           # the comparisons are false
    # every other cell is finite and has the bits of the run without those rows
    other = np.ones(got.shape[1:3], dtype=bool)
    other[0, 0] = False
    assert np.all(np.isfinite(got[0][other]))
    assert np.array_equal(bits(got[0][other]), bits(base[0][other]))


# ---- 4. several states in one launch ---------------------------------------------------------
def test_multi_state(cuda, parity):
    import torch
    import _native
    m = 1319
    ax, b = recipe(m)
    axs = np.stack([ax, ax * 1.01 + 0.125, np.abs(ax - 0.5)])
    masks = np.stack([(np.arange(m) % 3 != 0), (np.arange(m) % 2 != 0),
                      np.ones(m, dtype=bool)]).astype(np.float64)
    edges = np.histogram(b, 6)[1]
    shared = launch(axs, b, masks[0], edges, ax_ld=m + 5, roww_ld=0)[0]
    own = launch(axs, b, masks, edges, ax_ld=m + 5, roww_ld=m)[0]
    for s in range(3):
        one = launch(axs[s], b, masks[0], edges)[0]
        assert np.array_equal(bits(shared[s]), bits(one[0])), s
        one = launch(axs[s], b, masks[s], edges)[0]
        assert np.array_equal(bits(own[s]), bits(one[0])), s
    compare(shared, numpy_cells(axs, b, masks[0], edges), parity, 'lm_multi_shared')
    compare(own, numpy_cells(axs, b, masks, edges), parity, 'lm_multi_own')
    # BSLS_E_ARG
    L = _native.lib()
    t = torch.zeros(4 * m, dtype=torch.float64, device='cuda')
    p, st = ctypes.c_void_p(t.data_ptr()), _native.stream_handle()

    def rc(ax=p, ax_ld=m, b=p, roww=p, roww_ld=0, edges=p, nedges=7, m_=m, ns=1, out=p, work=p):
        return L.bsls_link_metrics(ax, ax_ld, b, roww, roww_ld, edges, nedges, m_, ns, out, work,
                                   st)
    E = _native.BSLS_E_ARG
    assert rc(m_=0) == E and rc(m_=-1) == E
    assert rc(ns=0) == E and rc(ns=1025) == E
    assert rc(nedges=-1) == E and rc(nedges=16) == E
    assert rc(ax_ld=m - 1) == E and rc(ax_ld=-m) == E
    assert rc(roww_ld=m - 1) == E and rc(roww_ld=-1) == E
    assert rc(ax=None) == E and rc(b=None) == E and rc(out=None) == E and rc(work=None) == E
    assert rc(edges=None) == E
    assert L.bsls_link_metrics_work_size(0, 1, 7) == 0
    assert L.bsls_link_metrics_work_size(m, 1025, 7) == 0
    assert L.bsls_link_metrics_work_size(m, 1, 16) == 0
    torch.cuda.synchronize()
    assert float(t.abs().max().item()) == 0.0               # a refused call writes nothing
    # the public wrapper: host or device arrays, 1-D or per-state masks
    from device import link_metrics
    got = link_metrics(torch.from_numpy(axs).cuda(), b, masks, edges)
    assert np.array_equal(bits(got), bits(own))
    got = link_metrics(ax, torch.from_numpy(b).cuda(), masks[0], edges)
    assert got.shape == (2, 8, 9) and np.array_equal(bits(got), bits(shared[0]))
    got = link_metrics(ax, b)
    assert got.shape == (2, 1, 9) and got[0, 0, 0] == m and got[1, 0, 0] == 0


# ---- 5. the engine ------------------------------------------------------------------------
M_ENG = 501


def clear_of_thresholds(ax, b, edges):
    """The condition of the module docstring, on the NumPy side."""
    ax = np.atleast_2d(ax)
    geh = np.sqrt(2 * (ax - b) ** 2 / (ax + b))
    assert np.all(np.isfinite(geh))
    for t in THRESHOLDS:
        assert np.min(np.abs(geh - t)) > 1e-9 * t, t
    for e in edges:
        d = np.abs(b - e)
        assert np.all((d == 0) | (d > 1e-9 * abs(e))), e


def eng_problem():
    sh, b = small(M_ENG)
    return sps.csr_matrix(sh['A']), b, np.asarray(sh['block_sizes'], dtype=np.int64)


def test_engine(cuda, orc):
    import _native
    from device import BBEngine, link_classes
    A, b, sizes = eng_problem()
    w = (np.arange(M_ENG) % 5 != 0).astype(np.float64)
    x0, N = orc.particular_x0(sizes), orc.block_sizes_to_N(sizes)
    edges = link_classes(b)
    opts = {'max_iter': 30, 'opt_tol': 1e-30}
    eng = BBEngine(A, b, sizes, options=opts, deterministic=True, row_weights=w)
    z = eng.solve().cpu().numpy().copy()
    assert eng.iterations == 30
    keep = [bits(t.cpu().numpy()) for t in (eng.scal, eng.z[0], eng.z[1], eng.g[0], eng.g[1])]
    held = eng.held_out()
    got = eng.link_metrics()
    after = [bits(t.cpu().numpy()) for t in (eng.scal, eng.z[0], eng.z[1], eng.g[0], eng.g[1])]
    assert all(np.array_equal(a, k) for a, k in zip(after, keep)) and eng.held_out() == held
    ax = A.dot(N.dot(z) + x0)
    clear_of_thresholds(ax, b, edges)
    same_dicts(got, restate_all(ax, b, w, edges), scalar=True, what='engine ', exact=SHARES)
    # the sums the iteration keeps: S_HELD over the held-out rows, S_RR over the train rows
    import dev_metrics
    xh = eng.n_apply(eng.current_z(eng._last_zbuf), with_x0=True)
    ax_dev = eng.apply_A_x(xh)
    cells = dev_metrics.link_metrics(ax_dev, b, w, edges)
    # NumPy on the A x_hat the kernel read: counts and max_GEH exactly
    ax_dev = ax_dev.cpu().numpy()
    assert np.max(np.abs(ax_dev - ax) / np.maximum(1.0, np.abs(ax))) <= 1e-12
    same_dicts(got, restate_all(ax_dev, b, w, edges), scalar=True, what='engine, device ax ')
    S = eng.scalars()
    assert np.array_equal(bits(S), keep[0])
    for st, slot in ((1, _native.S_HELD), (0, _native.S_RR)):
        ssq = float(np.sum(cells[st, :, 1]))
        assert abs(ssq - S[slot]) <= 1e-12 * S[slot], (st, ssq, S[slot])
    # one z, a list of z, and the next solve
    one = eng.link_metrics(z)
    many = eng.link_metrics([np.zeros_like(z), z])
    for k in dev_metrics.KEYS:
        assert one['test'][k] == got['test'][k] == many['test'][k][1]
        for a, g in zip(many['train_bin'][k], got['train_bin'][k]):
            assert (a is None and g is None) or a[1] == g
    assert many['test']['error'][0] > many['test']['error'][1]
    z2 = eng.solve().cpu().numpy().copy()
    assert np.array_equal(bits(z2), bits(z))
    # with the regulariser set the metrics are still of the plain residual
    eng.set_regulariser(100.0)
    zr = eng.solve().cpu().numpy().copy()
    assert not np.array_equal(zr, z)
    s_before = bits(eng.scalars())
    gr = eng.link_metrics()
    assert np.array_equal(bits(eng.scalars()), s_before) and eng.reg_lambda == 100.0
    axr = A.dot(N.dot(zr) + x0)
    clear_of_thresholds(axr, b, edges)
    same_dicts(gr, restate_all(axr, b, w, edges), scalar=True, what='reg ', exact=SHARES)
    # fixed_sums, unweighted: every link is train, A x by the general CSR kernel
    fx = BBEngine(A, b, sizes, options=opts, fixed_sums=True)
    zf = fx.solve().cpu().numpy().copy()
    gf = fx.link_metrics(nbins=4)
    axf = A.dot(N.dot(zf) + x0)
    clear_of_thresholds(axf, b, link_classes(b, 4))
    same_dicts(gf, restate_all(axf, b, np.ones(M_ENG), link_classes(b, 4)), scalar=True,
               what='fixed ', exact=SHARES)
    assert gf['test'] is None and len(gf['train_bin']['RMSE']) == 5
    # an engine built from a target has no b
    tg = BBEngine(A, None, sizes, options=opts, target=A.dot(x0) - b)
    with pytest.raises(ValueError, match='need b'):
        tg.link_metrics(z)
    with pytest.raises(ValueError, match='last solve'):
        BBEngine(A, b, sizes, options=opts).link_metrics()


# ---- 6. cross-validation ---------------------------------------------------------------------
def test_kfold_metrics(cuda, orc):
    from cross_validation import kfold, kfold_masks, kfold_path
    from device import KEYS, link_classes
    A, b, sizes = eng_problem()
    x0, N = orc.particular_x0(sizes), orc.block_sizes_to_N(sizes)
    edges = link_classes(b)
    opts = {'max_iter': 30, 'opt_tol': 1e-30}
    kw = dict(options=opts, deterministic=True)
    plain = kfold(A, b, x0, N, sizes, 3, **kw)
    assert all(set(f) == FOLD_KEYS for f in plain)
    seq = kfold(A, b, x0, N, sizes, 3, metrics=True, **kw)
    bat = kfold(A, b, x0, N, sizes, 3, batch=2, metrics=True, options=opts)
    for folds, name in ((seq, 'seq'), (bat, 'batch')):
        assert len(folds) == 3
        for f, w in zip(folds, kfold_masks(M_ENG, 3)):
            assert set(f) == FOLD_KEYS | {'train', 'test', 'train_bin', 'test_bin'}
            ax = A.dot(N.dot(f['z']) + x0)
            clear_of_thresholds(ax, b, edges)
            same_dicts(f, restate_all(ax, b, w, edges), scalar=True, what=name + ' ',
                       exact=SHARES)
            assert abs(f['test']['error'] - f['held_out']) <= 1e-10 * f['held_out']
    assert all(np.array_equal(f['z'], f0['z']) for f, f0 in zip(seq, plain))
    # the logged states, one launch per fold (per chunk with batch)
    for extra in (dict(kw), dict(options=opts, batch=2)):
        last = bat if 'batch' in extra else seq
        logd = kfold(A, b, x0, N, sizes, 3, metrics=True, record_every=10, **extra)
        for f, f1 in zip(logd, last):
            assert f['logged'] == [0, 10, 20, 30, 30]        # BB.solve's log, python/BB.py:10,40-44
            for k in KEYS:
                assert np.shape(f['test'][k]) == (5,) and np.shape(f['train'][k]) == (5,)
                assert f['test'][k][-1] == f1['test'][k] and f['train'][k][-2] == f1['train'][k]
                for a, g in zip(f['test_bin'][k], f1['test_bin'][k]):
                    assert (a is None and g is None) or a[-1] == g
            assert f['train']['error'][0] > f['train']['error'][-1]
    # lambda by a metric: the folds' mean of test['mean_GEH'], the smallest
    lams = [3.7e5, 0.0, 100.0]
    path = kfold_path(A, b, x0, N, sizes, 3, lams, select='mean_GEH', **kw)
    score = [float(np.mean([f['test']['mean_GEH'] for f in fs])) for fs in path['folds']]
    assert path['score'] == score and path['select'] == 'mean_GEH' and len(set(score)) == 3
    assert path['best'] == lams[int(np.argmin(score))] and path['best_index'] == int(np.argmin(score))
    assert [f['test']['mean_GEH'] for f in path['folds'][1]] == [f['test']['mean_GEH'] for f in seq]


def test_main_cv_metrics(cuda, tmp_path):
    import bsls_utils
    import main
    from test_gpu_row_weights import SEED
    np.random.seed(SEED)
    fname = os.path.join(str(tmp_path), 'test_main.mat')
    bsls_utils.generate_data(fname=fname)
    base = dict(noise=0, file=fname, log='WARN', init=False, eq='CP', method='BB',
                deterministic=True, cv=3)
    _, _, _, out0 = main.main(args=argparse.Namespace(**base))
    _, _, _, out = main.main(args=argparse.Namespace(cv_metrics=True, cv_bins=4, **base))
    _, _, _, outb = main.main(args=argparse.Namespace(cv_metrics=True, cv_batch=2, **base))
    assert all(set(f) == FOLD_KEYS for f in out0['cv'])
    for f, f0, fb in zip(out['cv'], out0['cv'], outb['cv']):
        assert np.array_equal(f['z'], f0['z'])
        for g in (f, fb):
            assert 0.0 <= g['test']['GEH_under_5'] <= 1.0 and g['train']['RMSE'] >= 0.0
        assert len(f['test_bin']['GEH_under_5']) == 5 and len(fb['test_bin']['GEH_under_5']) == 7
