"""Per-link weights and k-fold masks on the host: cross_validation.kfold_masks,
the weight validator, and main.solve_in_z_cpu(row_weights=...) against the
reference's way of holding links out -- the same solver on the row subset
A[train], b[train] (python/CrossValidation.py:126-183) -- and, for general
weights, on rows scaled by the weights' exact square roots.  Runs without a GPU."""
import numpy as np
import pytest
import scipy.sparse as sps


def elem_err(a, b):
    """max over elements of |a - b| / max(1, |b|) (the project's iterate contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---- kfold_masks ---------------------------------------------------------------
@pytest.mark.parametrize('m,k', [(500, 3), (7, 7), (500, 5), (11, 2)])
def test_kfold_masks_partition(m, k):
    from cross_validation import kfold_masks
    masks = kfold_masks(m, k)
    assert len(masks) == k
    for w in masks:
        assert w.dtype == np.float64 and w.shape == (m,)
        assert np.all((w == 0.0) | (w == 1.0))
    held = np.stack([w == 0.0 for w in masks])
    assert np.array_equal(held.sum(axis=0), np.ones(m, dtype=np.int64))   # exactly one fold each
    sizes = held.sum(axis=1)
    assert sizes.max() - sizes.min() <= 1 and sizes.sum() == m
    # contiguous index ranges in order, the longer folds first (KFold(n, n_folds=k))
    lo = 0
    for w, sz in zip(masks, sizes):
        assert np.array_equal(np.nonzero(w == 0.0)[0], np.arange(lo, lo + sz))
        lo += sz
    assert list(sizes) == sorted(sizes, reverse=True)


def test_kfold_masks_shuffle_repeats():
    from cross_validation import kfold_masks
    a = kfold_masks(500, 3, shuffle=True, seed=4)
    b = kfold_masks(500, 3, shuffle=True, seed=4)
    c = kfold_masks(500, 3, shuffle=True, seed=5)
    plain = kfold_masks(500, 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(not np.array_equal(x, y) for x, y in zip(a, c))
    assert any(not np.array_equal(x, y) for x, y in zip(a, plain))
    held = np.stack([w == 0.0 for w in a])
    assert np.array_equal(held.sum(axis=0), np.ones(500, dtype=np.int64))
    sizes = held.sum(axis=1)
    assert sizes.max() - sizes.min() <= 1


@pytest.mark.parametrize('m,k', [(5, 6), (500, 1), (500, 0), (3, -2)])
def test_kfold_masks_refusals(m, k):
    from cross_validation import kfold_masks
    with pytest.raises(ValueError):
        kfold_masks(m, k)


# ---- the validator ----------------------------------------------------------------
def test_row_weights_check():
    from device import row_weights_check
    assert row_weights_check(None, 5) is None
    w = row_weights_check([0, 1, 0.25, 4, 1], 5)
    assert w.dtype == np.float64 and w.flags['C_CONTIGUOUS']
    assert np.array_equal(w, [0.0, 1.0, 0.25, 4.0, 1.0])
    good = np.ones(5)
    for bad in (np.ones(4), np.ones(6), np.ones((5, 2))):
        with pytest.raises(ValueError):
            row_weights_check(bad, 5)
    for v in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
        w = good.copy()
        w[3] = v
        with pytest.raises(ValueError):
            row_weights_check(w, 5)


# ---- solve_in_z_cpu(row_weights=...) ----------------------------------------------
@pytest.fixture(scope='module')
def small(orc):
    from synthetic import make_shard, add_noise
    sh = make_shard(5_000, 250, 500, per_col=16)
    b = add_noise(sh['Ax'], 0.02)
    sizes = np.asarray(sh['block_sizes'])
    return dict(A=sps.csr_matrix(sh['A']), b=b, sizes=sizes, x0=orc.particular_x0(sizes),
                N=orc.block_sizes_to_N(sizes))


def cpu_states(P, A, b, iters, **kw):
    """The iterates at 1, 10 and 50 of solve_in_z_cpu's BB run (a run each:
    GradientDescent logs at record_every = 500 and at the end)."""
    from main import solve_in_z_cpu
    out = {}
    for it in iters:
        _, _, states = solve_in_z_cpu(A, b, P['x0'], P['N'], P['sizes'], 'BB',
                                      options={'max_iter': it, 'opt_tol': 1e-30, 'verbose': 0},
                                      **kw)
        out[it] = np.asarray(states[-1])
    return out


def test_mask_equals_the_row_subset(small, parity):
    from cross_validation import kfold_masks
    P = small
    w = kfold_masks(500, 5)[0]
    train = np.nonzero(w)[0]
    got = cpu_states(P, P['A'], P['b'], (1, 10, 50), row_weights=w)
    ref = cpu_states(P, P['A'][train], P['b'][train], (1, 10, 50))
    for it in (1, 10, 50):
        assert np.any(got[it] != 0.0)
        parity('row_weights_cpu_mask_%d' % it, elem_err(got[it], ref[it]), 1e-12)
    # and the weights matter: the unweighted run is another one
    plain = cpu_states(P, P['A'], P['b'], (50,))
    assert elem_err(plain[50], ref[50]) > 1e-6


def test_weights_equal_scaled_rows(small, parity):
    P = small
    rs = np.random.RandomState(21)
    w = rs.choice([0.25, 1.0, 4.0], size=500)
    root = np.sqrt(w)                      # exactly 0.5, 1, 2
    assert np.array_equal(root * root, w)
    D = sps.diags(root)
    got = cpu_states(P, P['A'], P['b'], (1, 10, 50), row_weights=w)
    ref = cpu_states(P, sps.csr_matrix(D.dot(P['A'])), root * P['b'], (1, 10, 50))
    for it in (1, 10, 50):
        parity('row_weights_cpu_weights_%d' % it, elem_err(got[it], ref[it]), 1e-12)


def test_cpu_weights_are_bb_only(small):
    from main import solve_in_z_cpu
    P = small
    for method in ('LBFGS', 'DORE'):
        with pytest.raises(ValueError):
            solve_in_z_cpu(P['A'], P['b'], P['x0'], P['N'], P['sizes'], method,
                           options={'max_iter': 2, 'opt_tol': 1e-30}, row_weights=np.ones(500))
    with pytest.raises(ValueError):
        solve_in_z_cpu(P['A'], P['b'], P['x0'], P['N'], P['sizes'], 'BB',
                       options={'max_iter': 2, 'opt_tol': 1e-30}, row_weights=np.ones(499))


def test_kfold_cpu(small, parity):
    from cross_validation import kfold, kfold_masks
    P = small
    folds = kfold(P['A'], P['b'], P['x0'], P['N'], P['sizes'], 3, device='cpu',
                  options={'max_iter': 50, 'opt_tol': 1e-30, 'verbose': 0})
    masks = kfold_masks(500, 3)
    assert len(folds) == 3
    for fold, w in zip(folds, masks):
        assert set(fold) == {'iters', 'stop', 'f_train', 'held_out', 'z', 'seconds'}
        assert fold['iters'] == 50 and fold['stop'] == 'max_iter'
        x = P['x0'] + P['N'].dot(fold['z'])
        test, train = np.nonzero(w == 0.0)[0], np.nonzero(w)[0]
        want = 0.5 * np.linalg.norm(P['A'][test].dot(x) - P['b'][test]) ** 2
        parity('kfold_cpu_held_out', abs(fold['held_out'] - want) / want, 1e-10)
        want = 0.5 * np.linalg.norm(P['A'][train].dot(x) - P['b'][train]) ** 2
        parity('kfold_cpu_f_train', abs(fold['f_train'] - want) / want, 1e-10)
        assert fold['held_out'] > 0 and fold['seconds'] >= 0


def test_main_cv_argument():
    import main
    args = main.parser().parse_args(['--cv', '3'])
    assert args.cv == 3
    assert main.parser().parse_args([]).cv is None
    args = main.parser().parse_args(['--cv', '3', '--method', 'LBFGS'])
    with pytest.raises(ValueError, match='cv'):
        main.main(args=args)
    args = main.parser().parse_args(['--cv', '3', '--reproducible'])
    with pytest.raises(ValueError, match='cv'):
        main.main(args=args)
