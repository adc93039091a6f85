"""Per-link weights on the BB engine (bsls_bb_problem.roww,
BBEngine.set_row_weights) and k-fold cross-validation on one engine
(cross_validation.kfold): K1's weighted row finish form by form against the
same engine with the weights off, BB iterates against the oracle run the way
the reference holds links out (the row subset A[train], b[train]) or on rows
scaled by the weights' exact square roots, the exits, one engine serving mask
after mask, and every refusal.  Needs an MI355X."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

SEED = 237423433
U = 2.0 ** -53


def elem_err(a, b):
    """max over elements of |a - b| / max(1, |b|) (the project's iterate contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ---- 1. the finish, form by form ---------------------------------------------
_SMALL = {}


def small(m):
    if m not in _SMALL:
        from synthetic import make_shard, add_noise
        sh = make_shard(5_000, 250, m, per_col=16)
        _SMALL[m] = (sh, add_noise(sh['Ax'], 0.02))
    return _SMALL[m]


# K1's forms: tiles of H = 192 rows (divides neither m) in 4 column groups
# (bb_k1_sum), 1 (finished in the walk's kernel), 10 (bb_k1_sum's loop past 8
# groups), and the panels (bb_k1's finish from the group partials)
FORMS = {'tiles4': dict(fmt='tiles', tile_plans=((192, 4, 0), None)),
         'tiles1': dict(fmt='tiles', tile_plans=((192, 1, 0), None)),
         'tiles10': dict(fmt='tiles', tile_plans=((192, 10, 0), None)),
         'panels': dict(fmt='panels')}


def form_engine(m, form, layouts, general):
    from device import BBEngine
    sh, b = small(m)
    eng = BBEngine(sh['A'], b, sh['block_sizes'], options={'max_iter': 5, 'opt_tol': 1e-30},
                   general=general, tile_layouts=layouts, **FORMS[form])
    if form == 'panels':
        assert eng.A_til is None and eng.A_pan is not None
    else:
        assert eng.A_til.img['ngroups'] == int(form[5:]) and m % 192
    return eng


def sentinels():
    import _native
    s = 1000.25 + np.arange(_native.S_COUNT, dtype=np.float64)
    s[_native.S_STOP] = 0.0
    return s


def k1_of(eng, xg, s0=None):
    """Stage 7 on x as K1 gathers it, scal prefilled; returns (r, scal)."""
    import torch
    eng.x.copy_(torch.from_numpy(xg))
    eng.scal.copy_(torch.from_numpy(sentinels() if s0 is None else s0))
    eng.r.fill_(-7.0)
    eng.stage(7, 0)
    torch.cuda.synchronize()
    return eng.r.cpu().numpy().copy(), eng.scalars().copy()


def mask_weights(m, H=192):
    """0/1: zeros at rows 0 and m - 1 and a run of zeros across the first
    row-block boundary (and the panels' boundaries are inside it or not: the
    run is 40 rows), ones elsewhere."""
    w = np.ones(m)
    w[0] = w[m - 1] = 0.0
    w[H - 20:H + 20] = 0.0
    return w


def mixed_weights(m):
    w = np.random.RandomState(5).choice([0.0, 0.25, 1.0, 4.0], size=m)
    w[0], w[m - 1], w[1], w[m - 2] = 0.0, 4.0, 0.25, 0.0
    return w


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('layouts', [(2, 2), (0, 0)])
@pytest.mark.parametrize('form', sorted(FORMS))
@pytest.mark.parametrize('m', [500, 501])
def test_finish_forms(cuda, parity, m, form, layouts, general):
    import _native
    S = _native
    eng = form_engine(m, form, layouts, general)
    fixed_order = form == 'panels' or layouts[0] == 0
    tag = 'rw_finish_%d_%s_%d_%s' % (m, form, layouts[0], 'general' if general else 'scaled')
    rs = np.random.RandomState(7)
    x = rs.rand(eng.n)
    xg = x if general else eng.colv.cpu().numpy() * x
    s0 = sentinels()
    r_plain, s_plain = k1_of(eng, xg)
    assert s_plain[S.S_HELD] == s0[S.S_HELD]          # unweighted: slot 15 never written
    assert np.all(r_plain != -7.0) and np.all(np.isfinite(r_plain))
    touched = {S.S_RR, S.S_FX, S.S_HELD}
    for kind, w in (('mask', mask_weights(m)), ('mixed', mixed_weights(m))):
        eng.set_row_weights(w)
        assert eng.P.roww == eng.row_weights.data_ptr()
        r_w, s_w = k1_of(eng, xg)
        want = np.where(w == 0.0, 0.0, w * r_plain)
        if fixed_order:
            assert np.array_equal(bits(r_w), bits(want)), (kind, float(np.max(np.abs(r_w - want))))
        else:
            parity(tag + '_r_' + kind, elem_err(r_w, want), 1e-12)
            assert np.array_equal(bits(r_w[w == 0.0]), bits(np.zeros(int(np.sum(w == 0.0)))))
        rr = math.fsum(w * r_plain * r_plain)
        held = math.fsum((r_plain * r_plain)[w == 0.0])
        assert held > 0.0
        parity(tag + '_rr_' + kind, rel(s_w[S.S_RR], rr), (m + 4) * U)
        parity(tag + '_held_' + kind, rel(s_w[S.S_HELD], held), (m + 4) * U)
        nr = np.sqrt(s_w[S.S_RR])
        assert bits(s_w[S.S_FX]) == bits(0.5 * (nr * nr))
        assert eng.held_out() == 0.5 * s_w[S.S_HELD]
        for k in range(S.S_COUNT):
            if k not in touched:
                assert bits(s_w[k]) == bits(s0[k]), k
    # a NaN in target on a held-out row: r there stays an exact 0.0 and f
    # finite; the hold-out error shows it
    import torch
    w = mask_weights(m)
    eng.set_row_weights(w)
    keep = eng.target.clone()
    eng.target[192] = float('nan')
    r_n, s_n = k1_of(eng, xg)
    eng.target.copy_(keep)
    assert bits(r_n[192]) == bits(0.0) and np.all(np.isfinite(r_n))
    assert np.isfinite(s_n[S.S_RR]) and np.isfinite(s_n[S.S_FX]) and np.isnan(s_n[S.S_HELD])
    # weights off again: the plain finish, slot 15 untouched
    eng.set_row_weights(None)
    assert not eng.P.roww and eng.held_out() == 0.0
    r_off, s_off = k1_of(eng, xg)
    assert bits(s_off[S.S_HELD]) == bits(s0[S.S_HELD])
    if fixed_order:
        assert np.array_equal(bits(r_off), bits(r_plain))
        assert np.array_equal(bits(s_off), bits(s_plain))
    else:
        parity(tag + '_r_off', elem_err(r_off, r_plain), 1e-12)
    torch.cuda.synchronize()


# ---- 2. BB iterates --------------------------------------------------------------
@pytest.fixture(scope='module')
def shard50k(orc):
    """The 50k-route problem, fold 0 of 5 and weights from {0.25, 1, 4}, with
    the oracle's traces: on the train rows, and on rows scaled by the exact
    square roots {0.5, 1, 2}."""
    from synthetic import make_shard, add_noise
    from cross_validation import kfold_masks
    sh = make_shard(50_000, 2_500, 5_000, per_col=16, seed=3)
    b = add_noise(sh['Ax'], 0.02, seed=3)
    A, sizes = sps.csr_matrix(sh['A']), np.asarray(sh['block_sizes'])
    masks = kfold_masks(5_000, 5)
    train = np.nonzero(masks[0])[0]
    wts = np.random.RandomState(21).choice([0.25, 1.0, 4.0], size=5_000)
    root = np.sqrt(wts)
    assert np.array_equal(root * root, wts)
    As = sps.csr_matrix(sps.diags(root).dot(A))
    out = dict(A=A, b=b, sizes=sizes, masks=masks, wts=wts)
    for name, (Ar, br) in (('mask', (A[train], b[train])), ('wts', (As, root * b))):
        ref = orc.bb_trace(Ar, br, sizes, 30, record_every=1)
        out['ref_' + name] = ref
        out['f_' + name] = float(orc.solve_in_z_parts(Ar, br, sizes)['f'](ref[30]))
    return out


def run_bb(P, iters=30, eng=None, weights=None, opt_tol=1e-30, **kw):
    """solve() with every iterate logged; returns (engine, {iter: z})."""
    from device import BBEngine
    if eng is None:
        eng = BBEngine(P['A'], P['b'], P['sizes'], options={'max_iter': iters, 'opt_tol': opt_tol},
                       row_weights=weights, **kw)
    rec = {}

    def log(i, s, dt):
        rec[i] = s
        return 0.0
    eng.solve(log=log, record_every=1, poll=1)
    return eng, rec


ENGINES = {'default': {}, 'deterministic': {'deterministic': True}, 'general': {'general': True}}


@pytest.mark.parametrize('kind', ['mask', 'wts'])
@pytest.mark.parametrize('which', sorted(ENGINES))
def test_iterates_match_oracle(cuda, shard50k, parity, which, kind):
    import _native
    P = shard50k
    w = P['masks'][0] if kind == 'mask' else P['wts']
    eng, rec = run_bb(P, weights=w, **ENGINES[which])
    assert eng.P.roww and eng.iterations == 30
    for i in (1, 10, 30):
        parity('rw_bb_%s_%s_%d' % (which, kind, i), elem_err(rec[i], P['ref_' + kind][i]), 1e-12)
    parity('rw_bb_%s_%s_f' % (which, kind),
           rel(eng.scalars()[_native.S_FX], P['f_' + kind]), 1e-12)


# ---- 3. exits --------------------------------------------------------------------
def test_max_iter_exit(cuda, shard50k):
    import _native
    eng, rec = run_bb(shard50k, weights=shard50k['masks'][0])
    assert eng.iterations == 30 and max(rec) == 30
    assert eng.stop_reason == _native.STOP_MAXITER
    assert _native.STOP_TEXT[eng.stop_reason] == 'max_iter'


# The opt_tol exit.  q_i = ||g_i||^2 / (1 + |f_i|) of the oracle on the masked
# problem (train rows of fold 0 of 5) falls slowly and smoothly: over 300
# iterations the largest one-iteration drop below every earlier q is a factor
# 1.152 (at iteration 2; q_1 = 2.88695603e8, q_300 = 1.4966e8), and seeds 0..39
# of the same problem give 1.117 .. 1.157, all at iteration 2 -- nowhere a
# factor 4, which an exit with q <= opt_tol / 2 after q >= 2 opt_tol needs.
# The one exit those margins allow is iteration 1, which has no earlier q:
# OPT_TOL = 1e9, exit iteration 1, q_1 / OPT_TOL = 0.2887 (<= 0.5: a factor
# 1.73 inside); the margin above is empty.  (Problem seed 3, as the other
# tests here; the engine's run measured the same exit on an MI355X.)
OPT_TOL, OPT_EXIT = 1.0e9, 1


def test_opt_tol_exit(cuda, orc, shard50k):
    import _native
    P = shard50k
    train = np.nonzero(P['masks'][0])[0]
    Ar, br = P['A'][train], P['b'][train]
    opts = {'max_iter': 300, 'verbose': 0, 'opt_tol': OPT_TOL}
    ref = orc.bb_trace(Ar, br, P['sizes'], 300, record_every=1, options=opts)
    assert max(ref) == OPT_EXIT
    Q = orc.solve_in_z_parts(Ar, br, P['sizes'])
    g = Q['nabla_f'](Q['z0'])
    q1 = float(g.dot(g)) / (1.0 + abs(float(Q['f'](ref[OPT_EXIT]))))
    assert q1 <= 0.5 * OPT_TOL, q1
    for kw in ({}, {'deterministic': True}):
        eng, rec = run_bb(P, iters=300, weights=P['masks'][0], opt_tol=OPT_TOL, **kw)
        assert eng.iterations == OPT_EXIT and max(rec) == OPT_EXIT
        assert eng.stop_reason == _native.STOP_GRAD
        assert _native.STOP_TEXT[eng.stop_reason] == 'Exiting... norm(grad) too small'
        assert elem_err(rec[OPT_EXIT], ref[OPT_EXIT]) <= 1e-12


# ---- 4. one engine, many masks ------------------------------------------------------
@pytest.mark.parametrize('det', [True, False])
def test_one_engine_many_masks(cuda, shard50k, parity, det):
    P = shard50k
    m0, m1 = P['masks'][0], P['masks'][1]
    eng, a = run_bb(P, weights=m0, deterministic=det)
    sa = eng.scalars().copy()
    ptrs = image_ptrs(eng)
    eng.set_row_weights(m1)
    _, b1 = run_bb(P, eng=eng)
    sb = eng.scalars().copy()
    eng.set_row_weights(m0)
    _, c = run_bb(P, eng=eng)
    sc = eng.scalars().copy()
    fresh, f1 = run_bb(P, weights=m1, deterministic=det)
    assert image_ptrs(eng) == ptrs
    assert elem_err(a[30], b1[30]) > 1e-6          # another fold, another fit
    if det:
        assert np.array_equal(bits(c[30]), bits(a[30])) and np.array_equal(bits(sc), bits(sa))
        assert np.array_equal(bits(b1[30]), bits(f1[30]))
        assert np.array_equal(bits(sb), bits(fresh.scalars()))
    else:
        parity('rw_masks_third_vs_first', elem_err(c[30], a[30]), 1e-12)
        parity('rw_masks_second_vs_fresh', elem_err(b1[30], f1[30]), 1e-12)
    eng.set_row_weights(None)
    _, off = run_bb(P, eng=eng)
    never, n1 = run_bb(P, deterministic=det)
    assert not never.P.roww
    if det:
        assert np.array_equal(bits(off[30]), bits(n1[30]))
        assert np.array_equal(bits(eng.scalars()), bits(never.scalars()))
    else:
        parity('rw_masks_off_vs_never', elem_err(off[30], n1[30]), 1e-12)


def image_ptrs(eng):
    out = []
    for img in (eng.A_til, eng.AT_til, eng.A_pan, eng.AT_pan):
        if img is not None:
            out += sorted(t.data_ptr() for t in img.t.values())
    return out + [eng.target.data_ptr(), eng.work.data_ptr()]


# ---- 5. cross_validation.kfold on one engine ----------------------------------------
def test_kfold_gpu(cuda, orc, shard50k, parity, monkeypatch):
    import device
    from cross_validation import kfold, kfold_masks
    P = shard50k
    x0 = orc.particular_x0(P['sizes'])
    N = orc.block_sizes_to_N(P['sizes'])
    eng = device.BBEngine(P['A'], P['b'], P['sizes'], x0=x0)
    ptrs = image_ptrs(eng)
    built = []
    init = device.BBEngine.__init__
    monkeypatch.setattr(device.BBEngine, '__init__',
                        lambda self, *a, **k: (built.append(1), init(self, *a, **k))[1])
    folds = kfold(P['A'], P['b'], x0, N, P['sizes'], 3, engine=eng,
                  options={'max_iter': 100, 'opt_tol': 1e-30})
    assert not built                                  # the engine passed in served every fold
    assert image_ptrs(eng) == ptrs and eng.row_weights is None and not eng.P.roww
    assert len(folds) == 3
    for k, (fold, w) in enumerate(zip(folds, kfold_masks(5_000, 3))):
        assert set(fold) == {'iters', 'stop', 'f_train', 'held_out', 'z', 'seconds'}
        assert fold['iters'] == 100 and fold['stop'] == 'max_iter'
        x = x0 + N.dot(fold['z'])
        test, train = np.nonzero(w == 0.0)[0], np.nonzero(w)[0]
        want = 0.5 * np.linalg.norm(P['A'][test].dot(x) - P['b'][test]) ** 2
        parity('rw_kfold_held_out_%d' % k, rel(fold['held_out'], want), 1e-10)
        want = 0.5 * np.linalg.norm(P['A'][train].dot(x) - P['b'][train]) ** 2
        parity('rw_kfold_f_train_%d' % k, rel(fold['f_train'], want), 1e-10)
    # without engine=, exactly one is built for all folds
    folds2 = kfold(P['A'], P['b'], x0, N, P['sizes'], 3,
                   options={'max_iter': 10, 'opt_tol': 1e-30})
    assert len(built) == 1 and len(folds2) == 3


# ---- 6. rejections --------------------------------------------------------------------
def test_engine_rejections(cuda):
    from device import BBEngine
    from distributed import ShardedBB
    from gradient_descent import GradientDescent
    sh, b = small(500)
    w = mask_weights(500)
    args = (sh['A'], b, sh['block_sizes'])
    for bad in (np.ones(499), -w, np.where(w == 0, np.nan, w), np.where(w == 0, np.inf, w)):
        with pytest.raises(ValueError):
            BBEngine(*args, row_weights=bad)
    with pytest.raises(ValueError, match='fixed_sums'):
        BBEngine(*args, row_weights=w, fixed_sums=True)
    fx = BBEngine(*args, fixed_sums=True)
    with pytest.raises(ValueError, match='fixed_sums'):
        fx.set_row_weights(w)
    eng = BBEngine(*args, row_weights=w, options={'max_iter': 5, 'opt_tol': 1e-30})
    for bad in (np.ones(501), -w):
        with pytest.raises(ValueError):
            eng.set_row_weights(bad)
    assert eng.P.roww == eng.row_weights.data_ptr()      # a refused swap changes nothing
    with pytest.raises(ValueError, match='row_weights'):
        eng.set_shard_role(1)
    with pytest.raises(ValueError, match='row_weights'):
        eng.set_shard_role(2)
    eng.set_shard_role(0)
    with pytest.raises(ValueError, match='row_weights'):
        eng.set_r_fixed(2.0 ** 40)
    with pytest.raises(ValueError, match='row_weights'):
        eng.line_search()
    with pytest.raises(ValueError, match='row_weights'):
        ShardedBB(eng, lambda t: None)
    for method in ('DORE', 'LBFGS'):
        gd = GradientDescent(z0=np.zeros(eng.nz), method=method, engine=eng,
                             options={'max_iter': 2, 'opt_tol': 1e-30})
        with pytest.raises(ValueError, match='row_weights'):
            gd.run()
    # and with the weights off all of it is allowed again
    eng.set_row_weights(None)
    eng.line_search()
    eng.set_shard_role(1)
    eng.set_shard_role(0)


def test_library_rejections(cuda):
    """BSLS_E_ARG from the library itself with bsls_bb_problem.roww set: the
    stages and entry points the weights do not cover, and the problem fields
    they do not go with."""
    import torch
    import _native
    from _native import stream_handle
    from device import BBEngine, LineSearch
    from distributed import ModelComm
    L = _native.lib()
    E = _native.BSLS_E_ARG
    sh, b = small(500)
    eng = BBEngine(sh['A'], b, sh['block_sizes'], row_weights=mask_weights(500),
                   options={'max_iter': 5, 'opt_tol': 1e-30})
    eng.set_z0(np.zeros(eng.nz))
    eng.prologue()
    P = eng.P
    st = stream_handle()
    for stage in (2, 8, 9, 10, 11, 12, 13, 14, 15):
        assert L.bsls_bb_stage(P, stage, 1, st) == E, stage
    assert L.bsls_bb_k2_part(P, 1, 0, st) == E
    assert L.bsls_bb_k1_rows(P, 1, 0, 1, st) == E
    assert L.bsls_bb_residual_rows(P, 1, 0, 1, st) == E
    assert L.bsls_dore_iterate(P, _native.DoreState(), 0, 1, st) == E
    ls = LineSearch(eng)
    z = torch.zeros(eng.nz, dtype=torch.float64, device='cuda')
    S = ls._state(z, z, z, ls.fx)
    assert L.bsls_lbfgs_ls_begin(P, S, st) == E
    assert L.bsls_lbfgs_ls_trials(P, S, 1, st) == E
    assert L.bsls_lbfgs_ls_finish(P, S, None, None, st) == E
    comm = ModelComm(1, 0)
    try:
        for role in (0, 1):
            P.shard_role = role
            assert L.bsls_bb_shard_iterate(P, comm.handle, 1, 1, st) == E
            other = torch.cuda.Stream()
            lb = (ctypes.c_int64 * 3)(0, 1, 2)
            assert L.bsls_bb_shard_iterate_parts(P, comm.handle, 1, 1, 2, lb,
                                                 ctypes.c_void_p(other.cuda_stream), st) == E
    finally:
        P.shard_role = 0
        comm.close()
    for field, bad in (('shard_role', 1), ('shard_role', 2), ('k1_atomic', 2), ('fx_sums', 1),
                       ('r_fx', 2.0 ** 40)):
        keep = getattr(P, field)
        setattr(P, field, bad)
        assert L.bsls_bb_iterate(P, 1, 1, st) == E, field
        assert L.bsls_bb_stage(P, 7, 0, st) == E, field
        setattr(P, field, keep)
    # the stages the weights cover, and the engine itself, still run
    for stage in (1, 3, 6, 7):
        assert L.bsls_bb_stage(P, stage, 0, st) == _native.BSLS_OK, stage
    eng.set_z0(np.zeros(eng.nz))
    eng.prologue()
    eng.iterate(1, 2)
    torch.cuda.synchronize()
    assert int(eng.scalars()[_native.S_ITER]) == 2


# ---- 7. main.main(--cv) -----------------------------------------------------------------
def test_main_cv(cuda, tmp_path):
    import bsls_utils
    import main
    np.random.seed(SEED)
    fname = os.path.join(str(tmp_path), 'test_main.mat')
    bsls_utils.generate_data(fname=fname)
    # (deterministic: the normal run repeats bit for bit, so the two can be compared)
    base = dict(noise=0, file=fname, log='WARN', init=False, eq='CP', method='BB',
                deterministic=True)
    iters0, _, states0, out0 = main.main(args=argparse.Namespace(**base))
    iters, _, states, out = main.main(args=argparse.Namespace(cv=3, **base))
    assert 'cv' not in out0 and len(out['cv']) == 3
    assert list(iters) == list(iters0)
    assert all(np.array_equal(a, b2) for a, b2 in zip(states, states0))
    assert set(out) - {'cv'} == set(out0)
    for k in out0:
        a, b2 = out[k], out0[k]
        if isinstance(b2, np.ndarray) or isinstance(b2, float):
            assert np.array_equal(np.asarray(a), np.asarray(b2)), k
        else:
            assert a == b2, k
    # the folds against SciPy, on the problem main solved
    from bsls_matrices import BSLSMatrices
    from cross_validation import kfold_masks
    bm = BSLSMatrices(fname=fname, full=True, L=True, OD=True, CP=True, LP=True, eq='CP',
                      init=False)
    bm.degree_reduced_form()
    AA, bb, N, block_sizes, x_split, nz, scaling, rsort_index, x0 = bm.get_LS()
    AA = sps.csr_matrix(AA)
    for fold, w in zip(out['cv'], kfold_masks(AA.shape[0], 3)):
        x = x0 + N.dot(fold['z'])
        test = np.nonzero(w == 0.0)[0]
        want = 0.5 * np.linalg.norm(AA[test].dot(x) - bb[test]) ** 2
        assert abs(fold['held_out'] - want) <= 1e-10 * max(want, 1e-300), (fold['held_out'], want)
        assert fold['iters'] >= 1 and fold['stop']
    with pytest.raises(ValueError, match='cv'):
        main.main(args=argparse.Namespace(**dict(base, cv=3, method='LBFGS')))
    with pytest.raises(ValueError, match='cv'):
        main.main(args=argparse.Namespace(**dict(base, cv=3, deterministic=None,
                                                  reproducible=True)))
