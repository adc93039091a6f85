"""BBEngine(fixed_sums=True) -- order-free fixed-point row sums on the dealt
tiles (bsls_bb_problem.fx_sums): what can be checked without a device -- the
row bounds, the tile plans for twice the LDS, the command line, and the
combinations the engine refuses before it touches the GPU."""
import numpy as np
import pytest
import scipy.sparse as sps


def test_bounds_scaled_and_general():
    from device import fixed_sum_bounds
    A = sps.csr_matrix(np.array([[1.0, 0.0, -2.5, 0.0],
                                 [0.0, 0.0, 0.0, 0.0],
                                 [0.5, 0.5, 0.5, -0.25]]))
    AT = A.T.tocsr()
    # general: the largest row sum of |values| of A (K1) and of A' (K2)
    a1, a2 = fixed_sum_bounds(A, AT, scaled=False)
    assert a1 == 3.5 and a2 == 3.0
    # scaled incidence: every term is a gathered entry, so the longest row
    a1, a2 = fixed_sum_bounds(A, AT, scaled=True)
    assert a1 == 4.0 and a2 == 2.0
    # an empty matrix still gives a positive bound (check_problem wants one)
    Z = sps.csr_matrix((3, 4))
    assert fixed_sum_bounds(Z, Z.T.tocsr(), scaled=False) == (1.0, 1.0)
    assert fixed_sum_bounds(Z, Z.T.tocsr(), scaled=True) == (1.0, 1.0)


# (rows, cols) of K1's image of A and K2's of A' (halo row) at the benchmark
# configurations C3 (1M routes, 100k links) and C5 (10M routes, 1M links)
@pytest.mark.parametrize('m,n', [(100_000, 1_000_000), (1_000_000, 10_000_000)])
@pytest.mark.parametrize('layout', [1, 2])
def test_tile_plans_leave_room_for_two_words(m, n, layout):
    import _native
    from device import tile_plan, fixed_plan_fits
    for rows, cols, halo in ((m, n, 0), (n, m, 1)):
        plan = tile_plan(rows, cols, halo, colv_lds=True, layout=layout)
        H = plan[0]
        assert H >= 64
        assert 2 * (H + halo + 1) * 8 <= _native.TILE_LDS_BYTES
        assert fixed_plan_fits(plan, halo)
        # dealt entries index a local row in 16 bits
        assert H + halo < 65536
    # the float form's K2 plan at C5 is the tallest the LDS holds: no room for two words
    tall = (_native.TILE_LDS_BYTES // 8 - 2, 1, 0)
    assert not fixed_plan_fits(tall, 1)


def test_parser_reproducible():
    import main
    p = main.parser()
    a = p.parse_args(['--reproducible'])
    assert a.reproducible is True and not a.deterministic
    a = p.parse_args([])
    assert a.reproducible is None
    with pytest.raises(SystemExit):
        p.parse_args(['--reproducible', '--deterministic'])


def test_main_refuses_other_methods_before_any_work():
    import argparse
    import main
    args = argparse.Namespace(noise=0, file='no-such-file.mat', log='WARN', init=False, eq='CP',
                              method='DORE', deterministic=None, reproducible=True)
    with pytest.raises(ValueError, match='BB only'):
        main.main(args=args)
    args = argparse.Namespace(noise=0, file='no-such-file.mat', log='WARN', init=False, eq='CP',
                              method='BB', deterministic=True, reproducible=True)
    with pytest.raises(ValueError, match='exclude'):
        main.main(args=args)


def _tiny():
    A = sps.csr_matrix(np.array([[1.0, 1.0, 0.0, 0.0], [0.0, 1.0, 1.0, 1.0]]))
    return A, np.array([1.0, 2.0]), np.array([2, 2])


@pytest.mark.parametrize('kw', [dict(deterministic=True),
                                dict(tile_layouts=(0, 0)),
                                dict(tile_layouts=(2, 0)),
                                dict(fmt='panels'),
                                dict(link_parts=2)])
def test_engine_refuses_combinations_without_a_device(kw):
    """Each is a ValueError raised before the engine touches the device (none
    is present where this test runs)."""
    from device import BBEngine
    A, b, sizes = _tiny()
    with pytest.raises(ValueError, match='fixed_sums'):
        BBEngine(A, b, sizes, fixed_sums=True, **kw)


def test_environment_default(monkeypatch):
    """BSLS_FIXED_SUMS=1 is the default of fixed_sums=None for the whole-problem
    default engine only; engines built for another purpose do not take it, and a
    conflicting BSLS_TILE_LAYOUT is an error, not a silent float run."""
    from device import BBEngine
    A, b, sizes = _tiny()
    monkeypatch.setenv('BSLS_FIXED_SUMS', '1')
    monkeypatch.setenv('BSLS_TILE_LAYOUT', '0,0')
    with pytest.raises(ValueError, match='fixed_sums'):
        BBEngine(A, b, sizes)


def test_gradient_descent_refuses_other_methods():
    from gradient_descent import GradientDescent

    class Eng:
        fixed_sums = True
    for method in ('DORE', 'LBFGS'):
        gd = GradientDescent(z0=np.zeros(2), method=method, engine=Eng())
        with pytest.raises(ValueError, match='BB only'):
            gd.run()
