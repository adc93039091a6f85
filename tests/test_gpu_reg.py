"""The weighted L2 regulariser on the BB engine (bsls_bb_problem.reg_w,
BBEngine.set_regulariser): the bb_reg kernel alone through the C ABI, K2's
extra operand form by form against the same engine with the pointer cleared,
the f that bb_record_f stores, BB iterates against the oracle's loop on the
reference's closures (python/CrossValidation.py:141-144), the exits, one
engine serving lambda after lambda, cross-validation over lambda, and every
refusal.  The problem is test_gpu_row_weights.py's 5 000-route one with d =
0.5 + 1.5 U(0, 1); lambda = 100 (the regulariser about two thirds of f after
400 iterations; 0.1 % after the 30 run here) and 3.7e5 (99 % after 300; 61-69 %
after 30).  Needs an MI355X."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

import test_bb_scalars_model as M
from test_reg_host import LAMBDAS, bits, oracle_trace, reference_closures, small

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
OPTS = {'max_iter': 10 ** 6, 'opt_tol': 1e-30}


def elem_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def sentinels(stop=0.0):
    import _native
    s = 1000.25 + np.arange(_native.S_COUNT, dtype=np.float64)
    s[_native.S_STOP] = stop
    return s


def put(t, a):
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    t[:a.size].copy_(torch.from_numpy(a))


def get(t, count=None):
    return t[:count if count is not None else t.numel()].cpu().numpy().copy()


def mask5(m):
    return (np.arange(m) % 5 != 0).astype(np.float64)


def reg_word(eng):
    import torch
    return float(eng.reg_work[:8].view(torch.float64).item())


# ---- 1. bsls_bb_reg alone ---------------------------------------------------------
# Blocks of 2, 3, 64, 65, 66, then 56 so that a block ends on the last lane of
# workgroup 0 (x entry 255) and the next starts on the first lane of workgroup
# 1; the block of 1000 crosses three workgroup boundaries (its halo entries),
# and n = 1319 = 5 * 256 + 39: six workgroups, the last one partly filled.
SIZES = np.array([2, 3, 64, 65, 66, 56, 1000, 2, 61], dtype=np.int64)
GUARD = 32


def test_bb_reg_kernel(cuda):
    import torch
    import _native
    from _native import stream_handle
    from device import BBEngine, reg_model
    L = _native.lib()
    n, nz = int(SIZES.sum()), int(SIZES.sum() - SIZES.size)
    assert np.cumsum(SIZES)[5] == 256 and n % 256 and -(-n // 256) >= 3
    rs = np.random.RandomState(17)
    A = sps.random(64, n, density=0.05, random_state=rs, format='csr')
    eng = BBEngine(A, rs.rand(64), SIZES, options=OPTS, fmt='panels', general=True)
    eng.set_regulariser(1.0)
    st = stream_handle()
    w = 100.0 * (0.5 + 1.5 * rs.rand(n)) ** 2
    w[rs.rand(n) < 0.1] = 0.0
    w[255] = w[256] = 7.0
    put(eng.reg_w, w)
    zs = [rs.rand(nz) + 0.01, rs.rand(nz) + 0.01]
    put(eng.z[0], zs[0])
    put(eng.z[1], zs[1])
    # reg_g and reg_work of the test's own, with guard entries around them
    f64 = dict(dtype=torch.float64, device='cuda')
    gbuf = torch.full((nz + 2 * GUARD,), 7.5, **f64)
    wbytes = L.bsls_bb_reg_work_size(n)
    assert wbytes % 8 == 0
    wbuf = torch.zeros(wbytes // 8 + GUARD, **f64)
    wbuf[wbytes // 8:] = 7.5
    eng.P.reg_g = gbuf[GUARD:].data_ptr()
    eng.P.reg_work = wbuf.data_ptr()
    S0 = sentinels()
    tk = slice(64 // 8, 64 // 8 + (L.bsls_ticket_bytes() + 7) // 8)
    first = None
    for zbuf in (0, 1):
        want_g, want_t = reg_model(zs[zbuf], SIZES, w)
        for launch in range(3):
            gbuf.fill_(7.5)
            put(eng.scal, S0)
            assert L.bsls_bb_reg(eng.P, zbuf, 0, st) == _native.BSLS_OK
            torch.cuda.synchronize()
            g, wk = get(gbuf), get(wbuf)
            assert np.all(g[:GUARD] == 7.5) and np.all(g[GUARD + nz:] == 7.5)
            assert np.all(wk[wbytes // 8:] == 7.5)
            assert np.array_equal(bits(get(eng.scal)), bits(S0))
            assert np.all(bits(wk[tk]) == 0)             # the tickets: ready for the next launch
            assert np.array_equal(bits(g[GUARD:GUARD + nz]), bits(want_g)), launch
            tot = wk[0]
            if launch == 0:
                first = (g, tot)
            assert np.array_equal(bits(g), bits(first[0])) and bits(tot) == bits(first[1])
        # the sum: against math.fsum, and the model's own order bit for bit
        xhat = _N(SIZES).dot(zs[zbuf]) + _x0(SIZES)
        ref = math.fsum(w * xhat ** 2)
        print('bb_reg zbuf %d: sum %.17g fsum %.17g rel %.3g bound %.3g model %.17g'
              % (zbuf, tot, ref, rel(tot, ref), (n + 3) * U, want_t))
        assert abs(tot - ref) <= (n + 3) * U * ref
        assert bits(tot) == bits(want_t)
    # a stopped run inside an iteration: nothing is written
    gbuf.fill_(7.5)
    wk0 = get(wbuf)
    S = sentinels(stop=2.0)
    put(eng.scal, S)
    assert L.bsls_bb_reg(eng.P, 1, 3, st) == _native.BSLS_OK
    torch.cuda.synchronize()
    assert np.all(get(gbuf) == 7.5)
    assert np.array_equal(bits(get(wbuf)), bits(wk0))
    assert np.array_equal(bits(get(eng.scal)), bits(S))
    # ... and outside an iteration (iter 0) the stop flag is not looked at
    assert L.bsls_bb_reg(eng.P, 1, 0, st) == _native.BSLS_OK
    torch.cuda.synchronize()
    assert not np.any(get(gbuf)[GUARD:GUARD + nz] == 7.5)
    # arguments
    put(eng.scal, S0)
    for zbuf in (-1, 2):
        assert L.bsls_bb_reg(eng.P, zbuf, 0, st) == _native.BSLS_E_ARG
    keep = eng.P.reg_w
    eng.P.reg_w = None
    assert L.bsls_bb_reg(eng.P, 0, 0, st) == _native.BSLS_E_ARG
    eng.P.reg_w = keep
    for field in ('reg_g', 'reg_work'):
        keep = getattr(eng.P, field)
        setattr(eng.P, field, None)
        assert L.bsls_bb_reg(eng.P, 0, 0, st) == _native.BSLS_E_ARG
        setattr(eng.P, field, keep)
    torch.cuda.synchronize()


def _N(sizes):
    from oracle import oracle
    return oracle.block_sizes_to_N(sizes)


def _x0(sizes):
    from oracle import oracle
    return oracle.particular_x0(sizes)


# ---- 2. K2 with the regulariser ------------------------------------------------------
# K2's forms: tiles of H = 192 rows in one column group and in three (the
# partials' hand-off), and the panels
K2FORMS = {'tiles1': dict(fmt='tiles', tile_plans=(None, (192, 1, 0))),
           'tiles3': dict(fmt='tiles', tile_plans=(None, (192, 3, 0))),
           'panels': dict(fmt='panels')}


@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('layouts', [(2, 2), (0, 0)])
@pytest.mark.parametrize('form', sorted(K2FORMS))
def test_k2_forms(cuda, parity, form, layouts, general):
    import torch
    import _native
    from _native import stream_handle
    from device import BBEngine, reg_model
    S = _native
    A, b, sizes, d = small(501)
    eng = BBEngine(A, b, sizes, options=OPTS, general=general, tile_layouts=layouts,
                   reg_lambda=LAMBDAS[0], reg_weights=d, **K2FORMS[form])
    if form == 'panels':
        assert eng.AT_til is None and eng.AT_pan is not None
    else:
        assert eng.AT_til.img['ngroups'] == int(form[5:]) and eng.n % 192
    assert eng.scaled == (not general) and eng.P.reg_w == eng.reg_w.data_ptr()
    fixed_order = form == 'panels' or layouts[1] == 0
    tag = 'reg_k2_%s_%d_%s' % (form, layouts[1], 'general' if general else 'scaled')
    L = _native.lib()
    nz, m = eng.nz, eng.m
    off = L.bsls_bb_dz_offset(eng.m, eng.n, eng.nz)
    dzt = eng.work[off:off + 8 * nz].view(torch.float64)
    rs = np.random.RandomState(41)
    z = rs.rand(nz)
    put(eng.z[0], z)
    assert L.bsls_bb_reg(eng.P, 0, 0, stream_handle()) == S.BSLS_OK
    reg_g = get(eng.reg_g, nz)
    want_g, _ = reg_model(z, sizes, LAMBDAS[0] * d * d)
    assert np.array_equal(bits(reg_g), bits(want_g))
    # |r| in 2^-10 [0.25, 4): the rows of A'|r| stay below 42 (16 entries of at
    # most 998 a row), so the dealt walks' order noise -- at most 15 u sum|terms|
    # a row, two rows an entry, two runs compared -- is provably below 3e-13,
    # inside the 1e-12 the dealt forms are held to, whatever order the atomics
    # take
    r = 2.0 ** -10 * M.signed(rs, m)
    g_prev, dz = 100.0 * M.signed(rs, nz), M.signed(rs, nz)
    for it in (0, 1):
        zn = it & 1

        def k2(plain):
            eng.load_r(r)
            put(eng.g[0], g_prev)
            eng.g[zn].fill_(3.0) if it else None
            put(dzt, dz)
            s0 = sentinels()
            put(eng.scal, s0)
            if plain:
                with eng._plain():
                    eng.stage(S.STAGE_K2, it)
            else:
                eng.stage(S.STAGE_K2, it)
            torch.cuda.synchronize()
            return get(eng.g[zn], nz), get(eng.scal), s0
        g_plain, s_plain, s0 = k2(True)
        g_reg, s_reg, _ = k2(False)
        assert eng.P.reg_w == eng.reg_w.data_ptr()
        assert np.array_equal(bits(get(eng.reg_g, nz)), bits(reg_g))      # K2 only reads it
        want = g_plain + reg_g
        assert float(np.max(np.abs(reg_g))) > 1.0 and np.all(g_plain != 3.0)
        err = elem_err(g_reg, want)
        print('%s it %d: max|g_reg - fl(g_plain + reg_g)| / max(1, |.|) = %.3g' % (tag, it, err))
        if fixed_order:
            assert np.array_equal(bits(g_reg), bits(want)), (it, err)
        else:
            parity('%s_g_%d' % (tag, it), err, 1e-12)
        if it == 0:
            assert np.array_equal(bits(s_reg), bits(s0))      # no scalar outside an iteration
            continue
        assert np.array_equal(bits(get(eng.g[0], nz)), bits(g_prev))
        dg = g_reg - g_prev
        refs = {S.S_SUMDG: M.exact_sum(dg), S.S_DZDG: M.exact_sum(dz, dg),
                S.S_DGDG: M.exact_sum(dg, dg), S.S_GG: M.exact_sum(g_reg, g_reg)}
        for slot, es in refs.items():
            print('%s slot %d: got %.17g ref %.17g err %.3g bound %.3g'
                  % (tag, slot, s_reg[slot], es.ref, float(M.error(s_reg[slot], es)),
                     float(M.bound(es))))
            assert es.k == nz and M.within(s_reg[slot], es), (slot, s_reg[slot], es.ref)
        for k in range(S.S_COUNT):
            if k not in refs:
                assert bits(s_reg[k]) == bits(s0[k]), k
        # and the regulariser is in the sums: they are not the plain run's
        assert s_reg[S.S_GG] != s_plain[S.S_GG]


# ---- 3. f -----------------------------------------------------------------------------
def fx_check(s, word, tag, parity):
    """scal[FX] against 0.5 RR + 0.5 sum formed exactly from the device's words."""
    import _native
    want = Fraction(s[_native.S_RR]) / 2 + Fraction(word) / 2
    err = abs(Fraction(s[_native.S_FX]) - want) / want
    parity(tag, float(err), 2 * U)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('lam', LAMBDAS)
def test_f_words(cuda, parity, lam, masked):
    import torch
    import _native
    S = _native
    from device import BBEngine
    A, b, sizes, d = small(500)
    w = mask5(500) if masked else None
    eng = BBEngine(A, b, sizes, options={'max_iter': 30, 'opt_tol': 1e-30}, deterministic=True,
                   reg_lambda=lam, reg_weights=d, row_weights=w)
    tag = 'reg_f_%g_%s' % (lam, 'mask' if masked else 'all')
    # inside an iteration: the K1 finish of iteration 30
    z = eng.solve().clone()
    torch.cuda.synchronize()
    s = eng.scalars().copy()
    assert s[S.S_ITER] == 30 and reg_word(eng) > 0.0
    fx_check(s, reg_word(eng), tag + '_iter', parity)
    share = 0.5 * reg_word(eng) / s[S.S_FX]
    print('%s: f %.6e, the regulariser %.1f %% of it' % (tag, s[S.S_FX], 100 * share))
    # outside one (stage 7 after Z2X and bsls_bb_reg): every slot but FX as
    # without the regulariser
    s0 = sentinels()
    put(eng.scal, s0)
    f_reg = eng.f(z)
    s_reg = eng.scalars().copy()
    word = reg_word(eng)
    assert f_reg == s_reg[S.S_FX]
    fx_check(s_reg, word, tag + '_stage7', parity)
    eng.set_regulariser(0)
    put(eng.scal, s0)
    f_plain = eng.f(z)
    s_plain = eng.scalars().copy()
    nr = np.sqrt(s_plain[S.S_RR])
    assert bits(f_plain) == bits(0.5 * (nr * nr))
    touched = {S.S_RR, S.S_FX} | ({S.S_HELD} if masked else set())
    for k in range(S.S_COUNT):
        if k != S.S_FX:
            assert bits(s_reg[k]) == bits(s_plain[k]), k
        if k not in touched:
            assert bits(s_reg[k]) == bits(s0[k]), k
    if masked:
        assert s_reg[S.S_HELD] > 0.0 and eng.held_out() == 0.5 * s_reg[S.S_HELD]
    assert f_reg > f_plain


# ---- 4. BB iterates ---------------------------------------------------------------------
@pytest.fixture(scope='module')
def traces(orc):
    """The oracle's 30 iterates on the reference-form closures, per (lambda,
    masked): the mask the way the reference holds links out, on the row
    subset."""
    A, b, sizes, d = small(501)
    keep = np.nonzero(mask5(501))[0]
    out = {}
    for lam in LAMBDAS:
        for masked in (False, True):
            Ar, br = (A[keep], b[keep]) if masked else (A, b)
            P, f, nabla_f = reference_closures(orc, Ar, br, sizes, lam, d)
            ref = oracle_trace(orc, P, f, nabla_f, 30)
            out[lam, masked] = (ref, float(f(ref[30])))
    return out


def run_bb(iters=30, eng=None, lam=None, masked=False, opt_tol=1e-30, **kw):
    """solve() with every iterate logged; returns (engine, {iter: z})."""
    from device import BBEngine
    if eng is None:
        A, b, sizes, d = small(501)
        eng = BBEngine(A, b, sizes, options={'max_iter': iters, 'opt_tol': opt_tol},
                       row_weights=mask5(501) if masked else None, reg_lambda=lam,
                       reg_weights=d, **kw)
    rec = {}

    def log(i, s, dt):
        rec[i] = s
        return 0.0
    eng.solve(log=log, record_every=1, poll=1)
    return eng, rec


ENGINES = {'default': {}, 'deterministic': {'deterministic': True}, 'general': {'general': True}}


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('lam', LAMBDAS)
@pytest.mark.parametrize('which', sorted(ENGINES))
def test_iterates_match_oracle(cuda, traces, parity, which, lam, masked):
    import _native
    ref, f_ref = traces[lam, masked]
    eng, rec = run_bb(lam=lam, masked=masked, **ENGINES[which])
    assert eng.P.reg_w and eng.iterations == 30 and bool(eng.P.roww) == masked
    tag = 'reg_bb_%s_%g_%s' % (which, lam, 'mask' if masked else 'all')
    for i in (1, 10, 30):
        parity('%s_%d' % (tag, i), elem_err(rec[i], ref[i]), 1e-12)
    parity(tag + '_f', rel(eng.scalars()[_native.S_FX], f_ref), 1e-12)
    if which == 'deterministic':
        s1 = eng.scalars().copy()
        _, again = run_bb(eng=eng)
        for i in (1, 10, 30):
            assert np.array_equal(bits(again[i]), bits(rec[i])), i
        assert np.array_equal(bits(eng.scalars()), bits(s1))


# ---- 5. exits ----------------------------------------------------------------------------
def test_max_iter_exit(cuda):
    import _native
    eng, rec = run_bb(lam=LAMBDAS[0], masked=True)
    assert eng.iterations == 30 and max(rec) == 30
    assert eng.stop_reason == _native.STOP_MAXITER
    assert _native.STOP_TEXT[eng.stop_reason] == 'max_iter'


# The opt_tol exit, pinned as test_gpu_row_weights.py pins it.  q_i = ||g_i||^2 /
# (1 + |f_i|) of the oracle on this problem (m = 501, fold 1-in-5 held out,
# lambda = 100) falls slowly: q_1 = 2.87278946e8, q_2 = 2.5142e8, q_10 =
# 2.0002e8, q_60 = 1.5908e8, and the largest one-iteration drop below every
# earlier q over 60 iterations is a factor 1.143 (1.19 unmasked, 1.28 / 1.25 at
# lambda = 3.7e5) -- nowhere a factor 4, which an exit with q <= opt_tol / 2
# after q >= 2 opt_tol needs.  What can be pinned is the exit at iteration 1,
# which has no earlier q: OPT_TOL = 1e9, q_1 / OPT_TOL = 0.2873 (<= 0.5).  f
# in q is the regularised objective, so the exit also pins scal[FX].
OPT_TOL, OPT_EXIT = 1.0e9, 1


def test_opt_tol_exit(cuda, orc):
    import _native
    A, b, sizes, d = small(501)
    keep = np.nonzero(mask5(501))[0]
    lam = LAMBDAS[0]
    P, f, nabla_f = reference_closures(orc, A[keep], b[keep], sizes, lam, d)
    rec = {}

    def log(i, s, dt):
        rec[i] = np.array(s)
        return 0.0
    orc.bb_solve(P['z0'], f, nabla_f, orc.stopping, record_every=1, proj=P['proj'], log=log,
                 options={'max_iter': 300, 'verbose': 0, 'opt_tol': OPT_TOL})
    assert max(rec) == OPT_EXIT
    g = nabla_f(P['z0'])
    q1 = float(g.dot(g)) / (1.0 + abs(float(f(rec[OPT_EXIT]))))
    assert q1 <= 0.5 * OPT_TOL, q1
    # without the regulariser in f the threshold is another: the plain f is a
    # third of it at lambda = 100 after 400 iterations, here at iteration 1
    for kw in ({}, {'deterministic': True}):
        eng, got = run_bb(iters=300, lam=lam, masked=True, opt_tol=OPT_TOL, **kw)
        assert eng.iterations == OPT_EXIT and max(got) == OPT_EXIT
        assert eng.stop_reason == _native.STOP_GRAD
        assert _native.STOP_TEXT[eng.stop_reason] == 'Exiting... norm(grad) too small'
        assert elem_err(got[OPT_EXIT], rec[OPT_EXIT]) <= 1e-12


# ---- 6. one engine, many lambda -------------------------------------------------------------
def image_ptrs(eng):
    out = []
    for img in (eng.A_til, eng.AT_til, eng.A_pan, eng.AT_pan):
        if img is not None:
            out += sorted(t.data_ptr() for t in img.t.values())
    return out + [eng.target.data_ptr(), eng.work.data_ptr()]


def test_one_engine_many_lambda(cuda):
    import torch
    from device import BBEngine
    l1, l2 = LAMBDAS
    A, b, sizes, d = small(501)
    eng, a = run_bb(lam=l1, deterministic=True)
    sa = eng.scalars().copy()
    ptrs = image_ptrs(eng)
    eng.set_regulariser(l2)                      # (d kept)
    assert np.array_equal(get(eng.reg_w), l2 * d * d)
    _, b2 = run_bb(eng=eng)
    sb = eng.scalars().copy()
    eng.set_regulariser(l1)
    _, c = run_bb(eng=eng)
    sc = eng.scalars().copy()
    fresh, f2 = run_bb(lam=l2, deterministic=True)
    assert image_ptrs(eng) == ptrs
    assert elem_err(a[30], b2[30]) > 1e-6          # another lambda, another fit
    assert np.array_equal(bits(c[30]), bits(a[30])) and np.array_equal(bits(sc), bits(sa))
    assert np.array_equal(bits(b2[30]), bits(f2[30]))
    assert np.array_equal(bits(sb), bits(fresh.scalars()))
    # the plain operators on a regularised engine are a plain engine's
    never = BBEngine(A, b, sizes, options={'max_iter': 30, 'opt_tol': 1e-30}, deterministic=True)
    rs = np.random.RandomState(2)
    z = torch.from_numpy(rs.rand(eng.nz)).cuda()
    r = torch.from_numpy(M.signed(rs, eng.m)).cuda()
    x = torch.from_numpy(rs.rand(eng.n)).cuda()
    for name, arg in (('apply_A', z), ('apply_AT', r), ('apply_A_x', x)):
        got, want = getattr(eng, name)(arg), getattr(never, name)(arg)
        assert np.array_equal(bits(get(got)), bits(get(want))), name
        assert eng.P.reg_w == eng.reg_w.data_ptr()
    v = rs.rand(eng.nz)
    assert np.array_equal(bits(eng.lsv_matvec(v)), bits(never.lsv_matvec(v)))
    # nabla_f and residual follow the regularised objective
    g_reg, g_plain = get(eng.nabla_f(z)), get(never.nabla_f(z))
    assert np.array_equal(bits(g_reg), bits(g_plain + get(eng.reg_g, eng.nz)))
    assert np.array_equal(bits(get(eng.residual(z))), bits(get(never.residual(z))))
    # lambda 0: a never-regularised engine's run, bit for bit
    eng.set_regulariser(0)
    assert not eng.P.reg_w and eng.reg_lambda == 0.0
    _, off = run_bb(eng=eng)
    _, n1 = run_bb(eng=never)
    assert np.array_equal(bits(off[30]), bits(n1[30]))
    assert np.array_equal(bits(eng.scalars()), bits(never.scalars()))
    eng.set_regulariser(None)
    assert not eng.P.reg_w


# ---- 7. cross-validation over lambda -------------------------------------------------------
def test_kfold_reg_gpu_vs_cpu(cuda, orc, parity, monkeypatch):
    import device
    from cross_validation import kfold, kfold_path, label_masks
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    x0, N = P['x0'], P['N']
    opts = {'max_iter': 20, 'opt_tol': 1e-30}
    lam = LAMBDAS[0]
    gpu = kfold(A, b, x0, N, sizes, 2, options=opts, reg_lambda=lam, reg_weights=d)
    cpu = kfold(A, b, x0, N, sizes, 2, options=opts, reg_lambda=lam, reg_weights=d,
                device='cpu')
    assert len(gpu) == len(cpu) == 2
    for k, (fg, fc) in enumerate(zip(gpu, cpu)):
        assert set(fg) == set(fc) == {'iters', 'stop', 'f_train', 'held_out', 'z', 'seconds'}
        assert fg['iters'] == fc['iters'] == 20 and fg['stop'] == fc['stop'] == 'max_iter'
        parity('reg_kfold_f_%d' % k, rel(fg['f_train'], fc['f_train']), 1e-10)
        parity('reg_kfold_held_%d' % k, rel(fg['held_out'], fc['held_out']), 1e-10)
        parity('reg_kfold_z_%d' % k, elem_err(fg['z'], fc['z']), 1e-10)
    # label-grouped folds through masks=
    masks = label_masks(np.arange(500) // 250)
    lab = kfold(A, b, x0, N, sizes, None, options=opts, reg_lambda=lam, reg_weights=d,
                masks=masks)
    for k in range(2):
        assert np.array_equal(masks[k] == 0.0, (np.arange(500) // 250) == k)
        parity('reg_kfold_label_%d' % k, elem_err(lab[k]['z'], gpu[k]['z']), 1e-10)
    # the path: per-lambda kfold calls, on one engine
    built = []
    init = device.BBEngine.__init__
    monkeypatch.setattr(device.BBEngine, '__init__',
                        lambda self, *a, **k: (built.append(1), init(self, *a, **k))[1])
    lams = [0.0, LAMBDAS[0], LAMBDAS[1]]
    path = kfold_path(A, b, x0, N, sizes, 2, lams, reg_weights=d, options=opts,
                      deterministic=True)
    assert len(built) == 1
    assert path['lambdas'] == lams and len(path['folds']) == 3
    eng = device.BBEngine(A, b, sizes, x0=x0, deterministic=True)
    for j, lam_j in enumerate(lams):
        one = kfold(A, b, x0, N, sizes, 2, options=opts, engine=eng, reg_lambda=lam_j,
                    reg_weights=d)
        assert not eng.P.reg_w and not eng.P.roww      # the engine passed in is put back
        for fa, fb in zip(path['folds'][j], one):
            assert np.array_equal(bits(fa['z']), bits(fb['z']))
            assert fa['held_out'] == fb['held_out'] and fa['f_train'] == fb['f_train']
        assert path['held_out'][j] == float(np.mean([f['held_out'] for f in one]))
    # an engine passed in with a regulariser of its own gets lambda and d back
    d0 = np.full(5000, 2.0)
    eng.set_regulariser(3.0, d0)
    kfold(A, b, x0, N, sizes, 2, options=opts, engine=eng, reg_lambda=lam, reg_weights=d)
    assert eng.reg_lambda == 3.0 and np.array_equal(get(eng.reg_d), d0)
    assert np.array_equal(get(eng.reg_w), 3.0 * d0 * d0) and eng.P.reg_w == eng.reg_w.data_ptr()
    eng.set_regulariser(0)
    assert path['best_index'] == int(np.argmin(path['held_out']))
    assert path['best'] == lams[path['best_index']]


def test_continuation_engine(cuda, orc, parity):
    import BB
    import continuation_solver
    import main
    import solvers
    from c_extensions import _cpu
    from device import BBEngine
    A, b, sizes, d = small(500)
    P = orc.solve_in_z_parts(A, b, sizes)
    opts = {'max_iter': 10, 'opt_tol': 1e-30}
    lam, steps = LAMBDAS[0], 2
    eng = BBEngine(A, b, sizes, options=opts, reg_weights=d)
    z = continuation_solver.solve_engine(eng, P['z0'], lam, steps=steps)
    assert eng.reg_lambda == lam and eng.iterations == 10
    # the host form: the reference's ramp over closures f(z, lamb), lamb = i / steps
    cum = np.concatenate(([0], np.cumsum(sizes - 1)))

    def proj(x):
        _cpu.isotonic(1, x, cum[:-1], x.shape[0], None, 1)
        return np.maximum(np.minimum(x, 1.), 0.)
    zh = P['z0']
    for i in range(steps + 1):
        f, nabla_f = main.host_closures(A, P['N'], P['target'], P['x0'], None,
                                        lam * i / float(steps), d)
        zh = BB.solve(zh, f, nabla_f, solvers.stopping, proj=proj, log=lambda i, s, dt: 0.0,
                      options=opts)
    parity('reg_continuation', elem_err(get(z), zh), 1e-10)


# ---- 8. refusals ---------------------------------------------------------------------------
def test_engine_refusals(cuda):
    import torch
    import DORE
    from cross_validation import kfold
    from device import BatchBB, BBEngine
    from distributed import ShardedBB
    from gradient_descent import GradientDescent
    A, b, sizes, d = small(500)
    args = (A, b, sizes)
    for bad in (np.ones(4999), -d, np.where(d > 1.9, np.nan, d), np.where(d > 1.9, np.inf, d)):
        with pytest.raises(ValueError):
            BBEngine(*args, reg_lambda=1.0, reg_weights=bad)
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            BBEngine(*args, reg_lambda=bad)
    with pytest.raises(ValueError, match='fixed_sums'):
        BBEngine(*args, reg_lambda=1.0, fixed_sums=True)
    fx = BBEngine(*args, fixed_sums=True)
    with pytest.raises(ValueError, match='fixed_sums'):
        fx.set_regulariser(1.0)
    # another x0 than the particular one: the device's N z + x0 would not be it
    x1 = np.zeros(5000)
    x1[np.cumsum(sizes) - 2] = 1.0
    with pytest.raises(ValueError, match='x0'):
        BBEngine(*args, x0=x1, reg_lambda=1.0)
    with pytest.raises(ValueError, match='x0'):
        BBEngine(*args, x0=x1).set_regulariser(1.0)
    eng = BBEngine(*args, reg_lambda=LAMBDAS[0], reg_weights=d,
                   options={'max_iter': 5, 'opt_tol': 1e-30})
    for bad in (-1.0, float('nan')):
        with pytest.raises(ValueError):
            eng.set_regulariser(bad)
    with pytest.raises(ValueError):
        eng.set_regulariser(1.0, np.ones(4999))
    assert eng.P.reg_w == eng.reg_w.data_ptr() and eng.reg_lambda == LAMBDAS[0]
    with pytest.raises(ValueError, match='regulariser'):
        eng.set_shard_role(1)
    with pytest.raises(ValueError, match='regulariser'):
        eng.set_shard_role(2)
    eng.set_shard_role(0)
    with pytest.raises(ValueError, match='regulariser'):
        eng.set_r_fixed(2.0 ** 40)
    with pytest.raises(ValueError, match='regulariser'):
        eng.line_search()
    with pytest.raises(ValueError, match='regulariser'):
        ShardedBB(eng, lambda t: None)
    with pytest.raises(ValueError, match='regulariser'):
        DORE.solve_engine(eng, np.zeros(eng.nz), 1.0, eng.target, log=lambda i, s, dt: 0.0)
    for method in ('DORE', 'LBFGS'):
        gd = GradientDescent(z0=np.zeros(eng.nz), method=method, engine=eng,
                             options={'max_iter': 2, 'opt_tol': 1e-30})
        with pytest.raises(ValueError, match='regulariser'):
            gd.run()
    from oracle import oracle
    x0, N = oracle.particular_x0(sizes), oracle.block_sizes_to_N(sizes)
    with pytest.raises(ValueError, match='batch'):
        kfold(A, b, x0, N, sizes, 2, batch=2, reg_lambda=1.0)
    with pytest.raises(ValueError, match='regulariser'):
        BatchBB(A, [b, b], sizes, reg_lambda=1.0)
    with pytest.raises(ValueError, match='regulariser'):
        BatchBB(A, [b, b], sizes, reg_weights=d)
    # and with lambda 0 all of it is allowed again
    eng.set_regulariser(0)
    eng.line_search()
    eng.set_shard_role(1)
    eng.set_shard_role(0)
    torch.cuda.synchronize()


def test_library_refusals(cuda):
    """BSLS_E_ARG from the library itself with bsls_bb_problem.reg_w set: the
    stages and entry points the regulariser does not cover, and the problem
    fields it does not go with."""
    import torch
    import _native
    from _native import stream_handle
    from device import BBEngine, LineSearch
    from distributed import ModelComm
    L = _native.lib()
    E = _native.BSLS_E_ARG
    A, b, sizes, d = small(500)
    eng = BBEngine(A, b, sizes, reg_lambda=LAMBDAS[0], reg_weights=d, row_weights=mask5(500),
                   options={'max_iter': 5, 'opt_tol': 1e-30})
    eng.set_z0(np.zeros(eng.nz))
    eng.prologue()
    P = eng.P
    st = stream_handle()
    eng.set_row_weights(None)                 # (the refusals below are the regulariser's own)
    for stage in (2, 8, 9, 10, 11, 12, 13, 14, 15):
        assert L.bsls_bb_stage(P, stage, 1, st) == E, stage
    assert L.bsls_bb_k2_part(P, 1, 0, st) == E
    assert L.bsls_bb_k1_rows(P, 1, 0, 1, st) == E
    assert L.bsls_bb_residual_rows(P, 1, 0, 1, st) == E
    assert L.bsls_dore_iterate(P, _native.DoreState(), 0, 1, st) == E
    keep = (P.reg_w, eng.reg_lambda)
    eng.reg_lambda = 0.0                      # (LineSearch's own check is the Python one)
    ls = LineSearch(eng)
    eng.reg_lambda = keep[1]
    z = torch.zeros(eng.nz, dtype=torch.float64, device='cuda')
    Sx = ls._state(z, z, z, ls.fx)
    assert L.bsls_lbfgs_ls_begin(P, Sx, st) == E
    assert L.bsls_lbfgs_ls_trials(P, Sx, 1, st) == E
    assert L.bsls_lbfgs_ls_finish(P, Sx, None, None, st) == E
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
                       ('r_fx', 2.0 ** 40), ('reg_g', None), ('reg_work', None)):
        keep = getattr(P, field)
        setattr(P, field, bad)
        assert L.bsls_bb_iterate(P, 1, 1, st) == E, field
        assert L.bsls_bb_stage(P, 7, 0, st) == E, field
        assert L.bsls_bb_prologue(P, st) == E, field
        assert L.bsls_bb_reg(P, 0, 0, st) == E, field
        setattr(P, field, keep)
    # the stages the regulariser covers, and the engine itself, still run
    for stage in (1, 3, 6, 7):
        assert L.bsls_bb_stage(P, stage, 0, st) == _native.BSLS_OK, stage
    eng.set_z0(np.zeros(eng.nz))
    eng.prologue()
    eng.iterate(1, 2)
    torch.cuda.synchronize()
    assert int(eng.scalars()[_native.S_ITER]) == 2
