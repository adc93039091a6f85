"""The weighted L2 regulariser on the host: the NumPy model of the bb_reg kernel
against SciPy's N and N', the host closures (main.host_closures /
solve_in_z_cpu(reg_*)) against the oracle's BB loop on the reference's
expressions (python/CrossValidation.py:141-144), label-grouped folds, the
continuation ramp, and every refusal that needs no device.  No GPU."""
import math

import numpy as np
import numpy.linalg as la
import pytest
import scipy.sparse as sps

U = 2.0 ** -53
LAMBDAS = (100.0, 3.7e5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


_SMALL = {}


def small(m):
    """The 5 000-route problem of test_gpu_row_weights.py, with d = 0.5 + 1.5 U(0, 1)."""
    if m not in _SMALL:
        from synthetic import make_shard, add_noise
        sh = make_shard(5_000, 250, m, per_col=16)
        d = 0.5 + 1.5 * np.random.RandomState(11).rand(5_000)
        _SMALL[m] = (sps.csr_matrix(sh['A']), add_noise(sh['Ax'], 0.02),
                     np.asarray(sh['block_sizes'], dtype=np.int64), d)
    return _SMALL[m]


def reference_closures(orc, A, b, sizes, lam, d):
    """f and nabla_f as the reference writes them (CrossValidation.py:141-144)
    with D = sqrt(lam) d, D2 = lam d^2, and the oracle's proj and z0."""
    P = orc.solve_in_z_parts(A, b, sizes)
    N, x0, target = P['N'], P['x0'], P['target']
    AT, NT = A.T.tocsr(), N.T.tocsr()
    D, D2 = np.sqrt(lam) * d, lam * d * d
    f = lambda z: 0.5 * la.norm(A.dot(N.dot(z)) + target) ** 2 + \
        0.5 * la.norm(D * (N.dot(z) + x0)) ** 2
    nabla_f = lambda z: NT.dot(AT.dot(A.dot(N.dot(z)) + target)) + \
        NT.dot(D2 * (N.dot(z) + x0))
    return P, f, nabla_f


def oracle_trace(orc, P, f, nabla_f, iters):
    rec = {}

    def log(i, state, dt):
        rec[i] = np.array(state)
        return 0.0
    orc.bb_solve(P['z0'], f, nabla_f, orc.stopping, record_every=1, proj=P['proj'], log=log,
                 options={'max_iter': iters, 'verbose': 0, 'opt_tol': 1e-30})
    return rec


# ---- the model of the kernel ---------------------------------------------------
@pytest.mark.parametrize('sizes', [[2, 3, 64, 65, 66, 1000, 2, 61], [2] * 300, [700, 3]])
def test_reg_model_matches_scipy(orc, sizes):
    from device import reg_model
    sizes = np.asarray(sizes, dtype=np.int64)
    n, nz = int(sizes.sum()), int(sizes.sum() - sizes.size)
    rs = np.random.RandomState(3)
    z = rs.rand(nz) + 0.01
    w = 100.0 * (0.5 + 1.5 * rs.rand(n)) ** 2
    w[rs.rand(n) < 0.1] = 0.0
    N = orc.block_sizes_to_N(sizes)
    NT = N.T.tocsr()
    x0 = orc.particular_x0(sizes)
    xhat = N.dot(z) + x0
    reg_g, total = reg_model(z, sizes, w)
    assert np.array_equal(bits(reg_g), bits(NT.dot(w * xhat)))
    want = math.fsum(w * xhat ** 2)
    assert abs(total - want) <= (n + 3) * U * want
    # an object with .sizes (a BlockLayout) is taken the same way
    class Lay:
        pass
    lay = Lay()
    lay.sizes = sizes
    g2, t2 = reg_model(z, lay, w)
    assert np.array_equal(bits(g2), bits(reg_g)) and t2 == total
    with pytest.raises(ValueError):
        reg_model(z[:-1], sizes, w)
    with pytest.raises(ValueError):
        reg_model(z, [1, n - 1], w)


# ---- the host closures -----------------------------------------------------------
def test_host_gradient_central_difference(orc):
    import main
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    rs = np.random.RandomState(5)
    for lam in LAMBDAS:
        for w in (None, (np.arange(500) % 5 != 0).astype(np.float64)):
            f, nabla_f = main.host_closures(A, P['N'], P['target'], P['x0'], w, lam, d)
            z = rs.rand(P['z0'].size)
            g = nabla_f(z)
            for _ in range(3):
                v = rs.randn(z.size)
                v /= la.norm(v)
                h = 1e-4
                num = (f(z + h * v) - f(z - h * v)) / (2 * h)
                # f is quadratic: the central difference is exact up to the
                # rounding of f, ~U f / h
                assert abs(num - g.dot(v)) <= 1e-6 * max(1.0, abs(g.dot(v))), (lam, num, g.dot(v))


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('lam', LAMBDAS)
def test_solve_in_z_cpu_every_iterate(orc, monkeypatch, lam, masked):
    """solve_in_z_cpu(reg_*) against the oracle's BB loop on the reference's
    expressions, every iterate of 30; with a 0/1 mask the oracle runs on the
    row subset, the way the reference holds links out.  BB.solve is made to
    log every iteration (solve_in_z_cpu's GradientDescent keeps the
    reference's record_every = 500)."""
    import BB
    import main
    A, b, sizes, d = small(501)
    P0 = orc.solve_in_z_parts(A, b, sizes)
    w = None
    Ar, br = A, b
    if masked:
        w = (np.arange(501) % 5 != 0).astype(np.float64)
        keep = np.nonzero(w)[0]
        Ar, br = A[keep], b[keep]
    P, f, nabla_f = reference_closures(orc, Ar, br, sizes, lam, d)
    ref = oracle_trace(orc, P, f, nabla_f, 30)
    assert sorted(ref) == list(range(31))
    solve = BB.solve
    monkeypatch.setattr(BB, 'solve', lambda *a, **k: solve(*a, **dict(k, record_every=1)))
    iters, times, states = main.solve_in_z_cpu(
        A, b, P0['x0'], P0['N'], sizes, 'BB', options={'max_iter': 30, 'opt_tol': 1e-30},
        row_weights=w, reg_lambda=lam, reg_weights=d)
    got = dict(zip(iters, states))
    assert sorted(got) == list(range(31))
    for i in range(31):
        err = np.max(np.abs(got[i] - ref[i]) / np.maximum(1.0, np.abs(ref[i])))
        assert err <= 1e-12, (i, err)
    # the regulariser is part of what was fitted
    plain = orc.bb_trace(Ar, br, sizes, 30)[30]
    assert np.max(np.abs(plain - ref[30])) > 1e-6


def test_kfold_cpu_regularised(orc):
    from cross_validation import kfold, kfold_path
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    opts = {'max_iter': 5, 'opt_tol': 1e-30}
    plain = kfold(A, b, P['x0'], P['N'], sizes, 2, options=opts, device='cpu')
    reg = kfold(A, b, P['x0'], P['N'], sizes, 2, options=opts, device='cpu',
                reg_lambda=LAMBDAS[1], reg_weights=d)
    assert len(reg) == 2 and np.max(np.abs(reg[0]['z'] - plain[0]['z'])) > 1e-6
    xh = P['N'].dot(reg[0]['z']) + P['x0']
    r = A.dot(xh) - b
    w = np.ones(500)
    w[:250] = 0.0
    want = 0.5 * np.sum(w * r * r) + 0.5 * LAMBDAS[1] * np.sum(d * d * xh * xh)
    assert abs(reg[0]['f_train'] - want) <= 1e-10 * want
    path = kfold_path(A, b, P['x0'], P['N'], sizes, 2, [0.0, LAMBDAS[1]], reg_weights=d,
                      options=opts, device='cpu')
    assert path['lambdas'] == [0.0, LAMBDAS[1]] and len(path['folds']) == 2
    assert np.array_equal(path['folds'][0][1]['z'], plain[1]['z'])
    assert np.array_equal(path['folds'][1][0]['z'], reg[0]['z'])
    held = [np.mean([f['held_out'] for f in fs]) for fs in path['folds']]
    assert path['held_out'] == held and path['best'] == path['lambdas'][int(np.argmin(held))]
    assert path['best_index'] == int(np.argmin(held))


# ---- label-grouped folds ---------------------------------------------------------------
def test_label_masks():
    from cross_validation import label_masks
    rs = np.random.RandomState(9)
    labels = rs.choice([3, 7, 8, 20, 21, 40, 41], size=200)
    loo = label_masks(labels)
    assert len(loo) == 7                               # the leave-one-label-out count
    for masks, k in ((loo, 7), (label_masks(labels, 3), 3), (label_masks(labels, 7), 7)):
        assert len(masks) == k
        M = np.array(masks)
        assert set(np.unique(M)) == {0.0, 1.0} and M.dtype == np.float64
        assert np.array_equal(np.sum(M == 0.0, axis=0), np.ones(200))   # held out exactly once
        for lab in np.unique(labels):
            rows = labels == lab
            assert np.all(M[:, rows] == M[:, rows][:, :1])              # a label stays together
    # leave-one-label-out: fold j is label j of the sorted distinct labels
    for j, lab in enumerate(np.unique(labels)):
        assert np.array_equal(loo[j] == 0.0, labels == lab)
    # k folds over the sorted distinct labels, the first 7 % 3 one label longer
    three = label_masks(labels, 3)
    got = [sorted(set(labels[m == 0.0])) for m in three]
    assert got == [[3, 7, 8], [20, 21], [40, 41]]
    # strings too (street names)
    names = np.array(['a', 'b', 'a', 'c', 'b', 'd'])
    two = label_masks(names, 2)
    assert [sorted(set(names[m == 0.0])) for m in two] == [['a', 'b'], ['c', 'd']]
    for bad in (dict(labels=[], k=None), dict(labels=[1, 1, 1], k=None),
                dict(labels=labels, k=1), dict(labels=labels, k=8), dict(labels=labels, k=2.5),
                dict(labels=labels, k=True)):
        with pytest.raises(ValueError):
            label_masks(bad['labels'], bad['k'])


def test_kfold_accepts_masks(orc):
    from cross_validation import kfold, label_masks
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    labels = np.arange(500) // 125
    masks = label_masks(labels)
    out = kfold(A, b, P['x0'], P['N'], sizes, None, options={'max_iter': 3, 'opt_tol': 1e-30},
                device='cpu', masks=masks)
    assert len(out) == 4
    x = P['x0'] + P['N'].dot(out[2]['z'])
    rows = np.nonzero(labels == 2)[0]
    want = 0.5 * la.norm(A[rows].dot(x) - b[rows]) ** 2
    assert abs(out[2]['held_out'] - want) <= 1e-10 * want
    with pytest.raises(ValueError):
        kfold(A, b, P['x0'], P['N'], sizes, None, device='cpu', masks=[np.ones(499)])
    with pytest.raises(ValueError):
        kfold(A, b, P['x0'], P['N'], sizes, None, device='cpu', masks=[])


# ---- continuation ------------------------------------------------------------------------
def test_continuation_solver_ramp(orc):
    import inspect
    import BB
    import continuation_solver
    import solvers
    sig = inspect.signature(continuation_solver.solve)
    assert list(sig.parameters) == ['x0', 'f', 'nabla_f', 'stopping', 'record_every', 'proj',
                                    'log', 'options', 'solve']
    assert sig.parameters['solve'].default is BB.solve
    assert sig.parameters['record_every'].default == 500
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    N, x0, target = P['N'], P['x0'], P['target']
    AT, NT = A.T.tocsr(), N.T.tocsr()
    seen = []

    def f(z, lamb):
        return 0.5 * la.norm(A.dot(N.dot(z)) + target) ** 2 + \
            0.5 * lamb * la.norm(N.dot(z) + x0) ** 2

    def nabla_f(z, lamb):
        seen.append(lamb)
        return NT.dot(AT.dot(A.dot(N.dot(z)) + target)) + lamb * NT.dot(N.dot(z) + x0)
    starts, ends = [], []

    def inner(x, f_l, g_l, stopping, record_every=500, proj=None, log=None, options=None):
        starts.append(np.array(x))
        out = BB.solve(x, f_l, g_l, stopping, record_every=record_every, proj=proj, log=log,
                       options=options)
        ends.append(np.array(out))
        return out
    z = continuation_solver.solve(P['z0'], f, nabla_f, solvers.stopping, proj=P['proj'],
                                  log=lambda i, s, dt: 0.0,
                                  options={'max_iter': 3, 'opt_tol': 1e-30}, solve=inner)
    lams = []
    for v in seen:
        if not lams or lams[-1] != v:
            lams.append(v)
    assert lams == [i / 10.0 for i in range(11)]
    assert len(starts) == 11 and np.array_equal(starts[0], P['z0'])
    for k in range(1, 11):
        assert np.array_equal(starts[k], ends[k - 1])         # warm start
    assert np.array_equal(z, ends[-1])
    # the last solve is an ordinary BB run at lambda = 1 from the tenth's end
    rec = oracle_trace(orc, dict(P, z0=ends[-2]), lambda v: f(v, 1.0),
                       lambda v: nabla_f(v, 1.0), 3)
    assert np.max(np.abs(rec[3] - z)) <= 1e-12


# ---- refusals that need no device -----------------------------------------------------
def test_refusals_host(orc):
    import main
    from cross_validation import kfold, kfold_path
    from device import reg_lambda_check, reg_weights_check
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    assert reg_lambda_check(None) == 0.0 and reg_lambda_check(0) == 0.0
    assert reg_lambda_check(np.float64(2.5)) == 2.5
    for bad in (-1.0, float('nan'), float('inf'), 'x', [1.0], True):
        with pytest.raises(ValueError):
            reg_lambda_check(bad)
    assert reg_weights_check(None, 5) is None
    assert reg_weights_check([1, 2, 0], 3).dtype == np.float64
    for bad in (np.ones(4999), -d, np.where(d > 1.9, np.nan, d), np.where(d > 1.9, np.inf, d)):
        with pytest.raises(ValueError):
            reg_weights_check(bad, 5000)
        with pytest.raises(ValueError):
            main.solve_in_z_cpu(A, b, P['x0'], P['N'], sizes, 'BB', reg_lambda=1.0,
                                reg_weights=bad)
    for method in ('LBFGS', 'DORE'):
        with pytest.raises(ValueError, match='BB only'):
            main.solve_in_z_cpu(A, b, P['x0'], P['N'], sizes, method, reg_lambda=1.0)
    with pytest.raises(ValueError):
        main.solve_in_z_cpu(A, b, P['x0'], P['N'], sizes, 'BB', reg_lambda=-1.0)
    # batch and a regulariser exclude each other, before anything is built
    for dev in ('cpu', 'gpu'):
        with pytest.raises(ValueError, match='batch'):
            kfold(A, b, P['x0'], P['N'], sizes, 2, device=dev, batch=2, reg_lambda=1.0)
    with pytest.raises(ValueError):
        kfold(A, b, P['x0'], P['N'], sizes, 2, device='cpu', reg_lambda=float('nan'))
    with pytest.raises(ValueError):
        kfold_path(A, b, P['x0'], P['N'], sizes, 2, [], device='cpu')
    with pytest.raises(ValueError):
        kfold_path(A, b, P['x0'], P['N'], sizes, 2, [1.0, -2.0], device='cpu')
    # main.py --reg: BB only, not with --reproducible, not with --cv-batch
    import argparse
    base = dict(noise=0, file='none.mat', log='WARN', init=False, eq='CP', method='BB')
    with pytest.raises(ValueError, match='reg'):
        main.main(args=argparse.Namespace(**dict(base, method='LBFGS', reg=1.0)))
    with pytest.raises(ValueError, match='reg'):
        main.main(args=argparse.Namespace(**dict(base, reproducible=True, reg=1.0)))
    with pytest.raises(ValueError, match='reg'):
        main.main(args=argparse.Namespace(**dict(base, cv=3, cv_batch=2, reg=1.0)))
    assert main.parser().parse_args(['--reg', '0.5']).reg == 0.5
    assert main.parser().parse_args([]).reg is None


def test_abi_appends_reg_fields():
    """The three fields sit after roww, in the header's order."""
    import _native
    names = [f[0] for f in _native.BBProblem._fields_]
    assert names[-4:] == ['roww', 'reg_w', 'reg_g', 'reg_work']
    assert {'bsls_bb_reg', 'bsls_bb_reg_work_size'} <= set(_native.declared_symbols())
    L = _native.load()
    assert L.bsls_bb_reg_work_size(1) >= 8 + L.bsls_ticket_bytes() + 8
    assert L.bsls_bb_reg_work_size(1000) - L.bsls_bb_reg_work_size(1) == 3 * 8
