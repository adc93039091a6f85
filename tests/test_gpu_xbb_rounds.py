"""One round of the fused x-space BB / L-BFGS engine (csrc/xbb.hip,
device.XBBEngine), slot by slot.  Needs an MI355X.

State is planted, not evolved: x, g, x_new, g_new, all 16 scal[] slots (the
meaningful ones chosen, the rest distinct sentinels), hist[], lb[], s, y and r
are written, eng.rounds(1) runs, and everything is read back.  The host model
(tests/test_xbb_rounds_model.py, validated there against the oracle's loops) is
fed the device's own SQ, GD, DXDG, DGDG, STEPINF (and, on an L-BFGS round, the
device's three coefficients) and must then give, bit for bit: every scal slot
-- MODE, ITER, F, FOLD, T, TT, REVERT, STOP, ROUNDS, BACKTRACKS and every
sentinel the branch does not write -- x, g, x_new (the oracle's projection
under BSLS_PROJ=exact), s, y, hist[] and the rho ring.  Bit for bit holds
because the library is built without fused multiply-adds, the elementwise
kernels round as NumPy does, and every reduction is a fixed-order (ticketed
last-workgroup) one.

The sums themselves: SQ, GD, DXDG, DGDG against the exact rational sum over
the device's own vectors within (k + 4) u sum|terms| (derived,
test_bb_scalars_model); STEPINF bit for bit; on the dyadic grid-stride case
all of them bit for bit.  r and g_new against SciPy on the device's x_new and
r within the bounds the operator tests already hold: the CSR kernels within
(nnz + 4) u (sum|a x| + |add|) per row (test_gpu_xspace_kernels.test_csr_spmv),
the panel / fixed-point residual within 1e-12 relative with g_new bit-identical
to SciPy's (test_gpu_lsq.test_lsq_operator).  The L-BFGS direction against the
long-double LBFGS_helper within 1e-11 ||d||_inf
(test_gpu_plugins.test_lbfgs_device_history_direction).  With BSLS_PARITY_LOG
set the measured errors are appended to that file
(profiles/xbb_rounds_parity.jsonl).
"""
import math

import numpy as np
import pytest
import scipy.sparse as sps

import test_bb_scalars_model as M
import test_xbb_rounds_model as X
from test_xbb_rounds_model import (BACKTRACK, BACKTRACKS, DGDG, DXDG, F, FOLD, GD, INIT, ITER,
                                   MAXITER, MODE, OPT, PROG, REVERT, ROUNDS, SQ, STEP, STEPINF,
                                   STOP, STOPPED, T, TT, same_bits)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
XMAX = 4.0                      # every planted |x| stays within the bound given to start()


def nan_bits(a, b):
    """Bit for bit, a NaN matching any NaN (0/0 has no one bit pattern)."""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(
        np.asarray(b, dtype=np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return same_bits(a[ok], b[ok])


_PROBLEMS = {}


def problem(name):
    if name not in _PROBLEMS:
        if name in ('Podd', 'Peven'):
            _PROBLEMS[name] = X.problem_P(name == 'Podd')
        elif name == 'stride':
            c = X.dyadic_bb_case(X.STRIDE_N)
            sizes = X.grid_problem(X.STRIDE_N)[2]
            _PROBLEMS[name] = (c['A'], c['b'], sizes)
            _PROBLEMS['stride-case'] = c
        else:
            _PROBLEMS[name] = X.grid_problem(int(name[1:]))
    return _PROBLEMS[name]


class Rig:
    """An engine over one problem, operator kind and projection, with the
    planting / reading helpers."""

    def __init__(self, prob, kind='csr', ball=False, C=0, fast=False):
        import _native
        from algorithm_utils import SparseLSQ, get_solver_parts
        from device import XBBEngine
        assert (_native.XS_MODE, _native.XS_STEPINF, _native.XS_BACKTRACKS, _native.XS_COUNT) == (
            MODE, STEPINF, BACKTRACKS, X.COUNT)
        assert (_native.XM_INIT, _native.XM_STOPPED, _native.XSTOP_PROG) == (INIT, STOPPED, PROG)
        self.A, self.b, self.sizes = problem(prob)
        self.A = sps.csr_matrix(self.A)
        self.AT = sps.csr_matrix(self.A.T)
        self.starts = X.starts_of(self.sizes)
        self.m, self.n = self.A.shape
        self.kind, self.proj_kind, self.C, self.fast = kind, 'ball' if ball else 'simplex', C, fast
        self.name = '%s/%s/%s/C%d%s' % (prob, kind, self.proj_kind, C, '/fast' if fast else '')
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(SparseLSQ, 'PANEL_MIN_NNZ', (1 << 62) if kind == 'csr' else 0)
            if kind == 'panels':
                mp.setenv('BSLS_LSQ_K1', 'panels')
            else:
                mp.delenv('BSLS_LSQ_K1', raising=False)
            mp.delenv('BSLS_LSQ_K2', raising=False)
            mp.setenv('BSLS_PROJ', 'fast' if fast else 'exact')
            _, proj, _, obj = get_solver_parts((self.A, self.b), self.starts, 1.0, is_sparse=True,
                                               lasso=ball)
            self.eng = XBBEngine(obj, proj, lbfgs=C)
        if kind == 'csr':
            assert obj.lsq is None
        else:
            assert obj.lsq is not None and obj.lsq.k1 == kind and obj.lsq.k2 == 'panels'
            assert bool(obj.lsq.op.fixed) == (kind == 'tiles_fixed')
        assert (self.eng.P.ball & 2 != 0) == fast
        self.x_start = np.full(self.n, 0.5)
        self.x_start[0] = XMAX

    def params(self, **kw):
        p = dict(max_iter=10 ** 6, opt_tol=1e-6, prog_tol=1e-12, f_min=None, hist_cap=16, C=self.C)
        p.update(kw)
        return p

    def put(self, t, a):
        import torch
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == t.numel()
        t.copy_(torch.from_numpy(a))

    def state(self, vec, **slots):
        """A full state from planted x, g, xn, gn: scal with a distinct
        sentinel in every slot not named, sentinel s, y, r; lb sentinels with
        the rho ring of vec['rho'] where given."""
        s = 1000.25 + np.arange(X.COUNT, dtype=np.float64)
        s[[MODE, ITER, F, T, TT, REVERT, ROUNDS, BACKTRACKS]] = [STEP, 7.0, 1e300, 1.0, 1.0, 0.0,
                                                                 41.0, 5.0]
        for k, v in slots.items():
            s[getattr(X, k)] = v
        C = self.C
        lb = 3000.25 + np.arange(2 * C + 8, dtype=np.float64) if C else np.zeros(0)
        if C and 'rho' in vec:
            lb[:C] = vec['rho']
        st = dict(x=vec['x'], g=vec['g'], xn=vec['xn'], gn=vec['gn'], scal=s, lb=lb,
                  r=np.full(self.m, 5.5), hist=None,
                  sv=np.full(self.n, 7.0) if C else None, yv=np.full(self.n, -7.0) if C else None)
        for k in ('x', 'xn'):
            assert np.nanmax(np.abs(st[k])) <= XMAX
        return st

    def start(self, x0, P):
        self.eng.start(x0, f_min=P['f_min'], opt_tol=P['opt_tol'], max_iter=P['max_iter'],
                       prog_tol=P['prog_tol'], hist_cap=P['hist_cap'])

    def plant(self, st):
        """Write a state (after a start()); hist gets its sentinels here."""
        e = self.eng
        st['hist'] = 2000.5 + np.arange(e.hist.numel(), dtype=np.float64)
        for t, k in ((e.x, 'x'), (e.g, 'g'), (e.xn, 'xn'), (e.gn, 'gn'), (e.r, 'r'),
                     (e.scal, 'scal'), (e.hist, 'hist')):
            self.put(t, st[k])
        if self.C:
            self.put(e.lb, st['lb'])
            self.put(e.s, st['sv'])
            self.put(e.y, st['yv'])

    def read(self):
        e = self.eng
        g = lambda t: t.cpu().numpy().copy()
        return dict(x=g(e.x), g=g(e.g), xn=g(e.xn), gn=g(e.gn), r=g(e.r), scal=g(e.scal),
                    hist=g(e.hist), lb=g(e.lb) if self.C else np.zeros(0),
                    sv=g(e.s) if self.C else None, yv=g(e.y) if self.C else None)

    def run(self, st, P, count=1):
        self.start(self.x_start, P)
        self.plant(st)
        self.eng.rounds(count)
        return self.read()


_RIGS = {}


def rig(cuda, *key, **kw):
    k = key + tuple(sorted(kw.items()))
    if k not in _RIGS:
        _RIGS[k] = Rig(*key, **kw)
    return _RIGS[k]


@pytest.fixture(scope='module', autouse=True)
def _drop_rigs():
    yield
    _RIGS.clear()
    _PROBLEMS.clear()


# ---- the checks every round gets -------------------------------------------------------

def sum_ref(a, b):
    return M.exact_sum(a, b) if a.size <= 20000 else X.fast_exact_sum(a, b)


def csr_rows(A, x):
    """Per row: the long-double sum of a_ij x_j and sum|a_ij x_j| (1 + 2u)."""
    ip = A.indptr
    p = A.data.astype(LD) * x[A.indices].astype(LD)
    nz = np.diff(ip) > 0
    R, S = np.zeros(A.shape[0], dtype=LD), np.zeros(A.shape[0])
    if p.size:
        R[nz] = np.add.reduceat(p, ip[:-1][nz])
        S[nz] = np.add.reduceat(np.abs(p).astype(np.float64), ip[:-1][nz]) * (1.0 + 2.0 * U)
    return R, S


def check_operator(R, after, parity, tag):
    """r = A x_new - b and g_new = A' r on the device's own x_new and r."""
    xn, r, gn = after['xn'], after['r'], after['gn']
    if R.kind == 'csr':
        ref, S = csr_rows(R.A, xn)
        bnd = (np.diff(R.A.indptr) + 4) * U * (S + np.abs(R.b))
        err = np.abs(r.astype(LD) - (ref - R.b.astype(LD))).astype(np.float64)
        parity('%s/r_row_ratio' % tag, float(np.max(err / np.maximum(bnd, 1e-300))), 1.0)
        ref, S = csr_rows(R.AT, r)
        bnd = (np.diff(R.AT.indptr) + 4) * U * S
        err = np.abs(gn.astype(LD) - ref).astype(np.float64)
        ok = bnd > 0
        assert np.all(gn[~ok] == 0.0)
        if ok.any():
            parity('%s/gn_row_ratio' % tag, float(np.max(err[ok] / bnd[ok])), 1.0)
    else:
        ref = R.A.dot(xn) - R.b
        tol = 1e-12 * np.abs(ref) + 1e-12 * np.abs(ref).max()     # assert_allclose(rtol, atol)
        parity('%s/r_ratio' % tag, float(np.max(np.abs(r - ref) / np.maximum(tol, 1e-300))), 1.0)
        assert same_bits(gn, R.AT.dot(r)), tag


def check_sums(R, before, after, parity, tag, planted=()):
    """planted: the sums whose terms were planted term by term -- every term
    within 2^-10 of the largest (M.terms_ok), so that a dropped or doubled
    element moves the sum by 1e9 times its bound."""
    s = after['scal']
    es = sum_ref(after['r'], after['r'])
    parity('%s/SQ_ratio' % tag, float(M.error(s[SQ], es) / max(M.bound(es), M.U ** 20)), 1.0)
    assert M.within(s[SQ], es), (tag, s[SQ], es.ref)
    if int(before['scal'][MODE]) in (INIT, STOPPED):
        return
    dx, dg = after['xn'] - after['x'], after['gn'] - after['g']
    want_inf = float(np.max(np.abs(dx)))
    assert same_bits(s[STEPINF], want_inf), (tag, s[STEPINF], want_inf)
    sums = [('GD', GD, after['g'], dx)]
    if s[ITER] == before['scal'][ITER] + 1.0:
        sums += [('DXDG', DXDG, dx, dg), ('DGDG', DGDG, dg, dg)]
    for name, slot, a, b in sums:
        es = sum_ref(a, b)
        if name in planted:
            assert M.terms_ok(a * b), (tag, name)
        if es.sumabs == 0:
            assert s[slot] == 0.0, (tag, name)
            continue
        parity('%s/%s_ratio' % (tag, name), float(M.error(s[slot], es) / M.bound(es)), 1.0)
        assert M.within(s[slot], es), (tag, name, s[slot], es.ref)


def check_round(R, before, after, P, parity, tag, bounds=True, planted=()):
    """The model, fed the device's sums, against everything read back."""
    C = R.C
    s0 = before['scal']
    lb_round = C > 0 and int(s0[MODE]) == STEP and s0[ITER] > 5.0
    s1 = after['scal']
    dev = dict(SQ=s1[SQ], GD=s1[GD], DXDG=s1[DXDG], DGDG=s1[DGDG], STEPINF=s1[STEPINF],
               r=after['r'], gn=after['gn'])
    if lb_round:
        dev['coef'] = after['lb'][2 * C:2 * C + 3]
        dev['lb'] = after['lb']
    want = X.round_model(before, R.A, R.AT, R.b, R.starts, R.proj_kind, P, dev=dev)
    for q in range(X.COUNT):
        assert nan_bits(s1[q], want['scal'][q]), (tag, 'scal', q, s1[q], want['scal'][q], s0[q])
    for k in ('x', 'g', 'hist') + (('sv', 'yv') if C else ()):
        assert nan_bits(after[k], want[k]), (tag, k)
    if R.fast:
        ref = want['xn']
        err = float(np.max(np.abs(after['xn'] - ref) / np.maximum(1.0, np.abs(ref))))
        parity('%s/xn_fast' % tag, err, 1e-12)
    else:
        assert nan_bits(after['xn'], want['xn']), (tag, 'xn', float(np.nanmax(np.abs(
            after['xn'] - want['xn']))))
    if C:
        assert nan_bits(after['lb'][:C], want['lb'][:C]), (tag, 'rho ring')
        if lb_round:
            k = int(s0[ITER]) - 1
            used = {C + (k - j) % C for j in range(1, min(k, C) + 1)}
            keep = [q for q in range(C, 2 * C + 8) if q not in used and not 2 * C <= q < 2 * C + 4]
        else:
            keep = list(range(C, 2 * C + 8))
        assert same_bits(after['lb'][keep], before['lb'][keep]), (tag, 'lb untouched')
    if bounds:
        check_operator(R, after, parity, tag)
        check_sums(R, before, after, parity, tag, planted)
    return want


# ---- a, b, c: STEP, BACKTRACK and REVERT rounds ----------------------------------------------

BB_RIGS = [('Podd', 'csr', False), ('Podd', 'panels', False), ('Podd', 'tiles_fixed', False),
           ('Peven', 'csr', True), ('Peven', 'panels', True), ('Peven', 'tiles_fixed', False)]
GRID_RIGS = [('n%d' % n, 'csr', False) for n in X.GRID_NS]
IDS = lambda v: '-'.join(str(q) for q in v) if isinstance(v, tuple) else None


@pytest.mark.parametrize('key', BB_RIGS + GRID_RIGS, ids=IDS)
def test_step_round(cuda, parity, key):
    R = rig(cuda, key[0], key[1], ball=key[2])
    vec = X.planted_vectors(R.n, seed=11)
    for it, t in ((1.0, 1.0), (7.0, 0.0123)):
        st = R.state(vec, MODE=STEP, ITER=it, T=t, TT=0.64)
        P = R.params(hist_cap=16 if it == 1.0 else 3)        # ITER 7 -> k = 7 >= hist_cap
        after = R.run(st, P)
        tag = 'step/%s/it%d' % (R.name, it)
        want = check_round(R, st, after, P, parity, tag)
        assert same_bits(after['x'], vec['xn']) and same_bits(after['g'], vec['gn'])
        xo = vec['xn'] + (-t) * vec['gn']
        X.project(xo, R.starts, R.proj_kind)
        assert same_bits(after['xn'], xo), tag
        s = after['scal']
        assert (s[MODE], s[ITER], s[FOLD], s[TT], s[REVERT], s[STOP]) == (STEP, it + 1, 1e300,
                                                                          1.0, 0.0, 0.0)
        assert s[ROUNDS] == 42.0 and s[BACKTRACKS] == 5.0 and s[F] == .5 * s[SQ]
        assert same_bits(s[T], s[DXDG] / s[DGDG]) and s[15] == st['scal'][15]
        if it == 1.0:
            assert same_bits(after['hist'][1], s[F])
            assert same_bits(np.delete(after['hist'], 1), np.delete(st['hist'], 1))
        else:
            assert same_bits(after['hist'], st['hist'])      # k >= hist_cap: untouched


def test_step_round_fast_projection(cuda, parity):
    """BSLS_PROJ=fast: x_new within the sort-free projection's 1e-12
    max(1, |ref|) of the oracle's; everything else as under exact."""
    R = rig(cuda, 'Podd', 'csr', fast=True)
    vec = X.planted_vectors(R.n, seed=11)
    st = R.state(vec, MODE=STEP, ITER=7.0, T=0.0123)
    after = R.run(st, R.params())
    check_round(R, st, after, R.params(), parity, 'step/%s' % R.name)
    ends = np.append(R.starts[1:], R.n)
    sums = np.array([after['xn'][a:b].sum() for a, b in zip(R.starts, ends)])
    assert np.max(np.abs(sums - 1.0)) <= 1e-12 and after['xn'].min() >= 0.0


def infeasible(x, starts, ends, kind):
    """x is clearly outside the feasible set, so a projection would have moved
    it: a block off the simplex (a negative entry, or a sum 1e-3 away from 1),
    or outside the l1 ball (|block|_1 > 1 + 1e-3)."""
    for a, b in zip(starts, ends):
        blk = x[a:b]
        if kind == 'ball':
            if np.abs(blk).sum() > 1.0 + 1e-3:
                return True
        elif blk.min() < 0.0 or abs(blk.sum() - 1.0) > 1e-3:
            return True
    return False


@pytest.mark.parametrize('key', BB_RIGS + GRID_RIGS, ids=IDS)
def test_backtrack_round(cuda, parity, key):
    R = rig(cuda, key[0], key[1], ball=key[2])
    base = X.planted_vectors(R.n, seed=12)
    ends = np.append(R.starts[1:], R.n)
    rs = np.random.RandomState(12)
    for tt, planted in ((0.8, ('GD',)), (0.8 * 0.8, ('DXDG', 'DGDG'))):
        vec = dict(base)
        if 'DGDG' in planted:
            # g = (host g_new at the combined point) - d, |d| in [0.25, 4]: the
            # device's dg is d to rounding, so dx.dg and dg.dg are planted
            # term by term (as test_bb_scalars_model does for g_prev)
            xa = (1.0 - tt) * base['x'] + tt * base['xn']
            vec['g'] = R.AT.dot(R.A.dot(xa) - R.b) - M.signed(rs, R.n)
        st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=tt, REVERT=0.0, T=0.37)
        P = R.params()
        after = R.run(st, P)
        tag = 'backtrack/%s/tt%.2f' % (R.name, tt)
        check_round(R, st, after, P, parity, tag, planted=planted)
        xo = (1.0 - tt) * vec['x'] + tt * vec['xn']
        assert same_bits(after['xn'], xo), tag
        assert same_bits(after['x'], vec['x']) and same_bits(after['g'], vec['g'])
        # no projection ran: the planted x_new is off the simplex / outside
        # the ball, and so is the combination
        assert infeasible(xo, R.starts, ends, R.proj_kind), tag
        s = after['scal']
        assert (s[MODE], s[ITER], s[TT], s[STOP]) == (STEP, 8.0, 1.0, 0.0)       # F = 1e300
        # a rejected one: F far below
        st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=tt, REVERT=0.0, F=-1e300)
        after = R.run(st, P)
        check_round(R, st, after, P, parity, tag + '/reject', bounds=False)
        s = after['scal']
        assert (s[MODE], s[ITER], s[REVERT], s[BACKTRACKS]) == (BACKTRACK, 7.0, 0.0, 6.0)
        assert same_bits(s[TT], tt * .8) and s[F] == -1e300
        assert same_bits(s[[FOLD, DXDG, DGDG, STOP]], st['scal'][[FOLD, DXDG, DGDG, STOP]])


@pytest.mark.parametrize('key', BB_RIGS + GRID_RIGS[:4], ids=IDS)
def test_revert_round(cuda, parity, key):
    R = rig(cuda, key[0], key[1], ball=key[2])
    vec = X.planted_vectors(R.n, seed=13)
    st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=0.8 ** 9, REVERT=1.0)
    P = R.params()
    after = R.run(st, P)
    check_round(R, st, after, P, parity, 'revert/%s' % R.name)
    assert same_bits(after['xn'], vec['x']) and same_bits(after['x'], vec['x'])
    s = after['scal']
    assert s[GD] == 0.0 and s[STEPINF] == 0.0 and s[DXDG] == 0.0 and s[REVERT] == 0.0


# ---- the Armijo boundary -------------------------------------------------------------------

@pytest.mark.parametrize('key', BB_RIGS[:4], ids=IDS)
def test_armijo_boundary(cuda, parity, key):
    """f_new > f + 1e-4 g.(x_new - x) is strict: F one ulp below the doubles
    that put the line exactly on f_new rejects, those doubles and the one
    above accept."""
    R = rig(cuda, key[0], key[1], ball=key[2])
    vec = X.planted_vectors(R.n, seed=14)
    P = R.params()
    tt = 0.8
    st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=tt, REVERT=0.0)
    learn = R.run(st, P)['scal']
    f_new, gd = .5 * learn[SQ], learn[GD]
    below, lo, hi, above = X.armijo_boundary(f_new, gd)
    assert lo + 1e-4 * gd == f_new and below + 1e-4 * gd < f_new
    for name, Fv, accept in (('below', below, False), ('lo', lo, True), ('hi', hi, True),
                             ('above', above, True)):
        st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=tt, REVERT=0.0, F=Fv)
        after = R.run(st, P)
        tag = 'armijo/%s/%s' % (R.name, name)
        check_round(R, st, after, P, parity, tag, bounds=False)
        s = after['scal']
        assert same_bits(s[SQ], learn[SQ]) and same_bits(s[GD], gd), tag     # deterministic
        if accept:
            assert (s[MODE], s[ITER], s[TT], s[BACKTRACKS]) == (STEP, 8.0, 1.0, 5.0), tag
            assert same_bits(s[F], f_new) and same_bits(s[FOLD], Fv), tag
        else:
            assert (s[MODE], s[ITER], s[BACKTRACKS], s[REVERT]) == (BACKTRACK, 7.0, 6.0, 0.0), tag
            assert same_bits(s[TT], tt * .8) and same_bits(s[F], Fv), tag


@pytest.mark.parametrize('key', BB_RIGS[:3], ids=IDS)
def test_revert_flag_at_the_step_threshold(cuda, parity, key):
    """REVERT = (||x_new - x||_inf < 1e-12) on a rejected round, the step just
    below and just above."""
    R = rig(cuda, key[0], key[1], ball=key[2])
    base = X.planted_vectors(R.n, seed=15)
    rs = np.random.RandomState(15)
    P = R.params()
    for delta, want in ((1.2e-12, 1.0), (1.3e-12, 0.0)):       # times tt = 0.8
        vec = dict(base)
        d = rs.uniform(0.2, 0.9, size=R.n) * delta
        d[R.n // 2] = delta
        vec['xn'] = base['x'] + d
        st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=0.8, REVERT=0.0, F=-1e300)
        after = R.run(st, P)
        tag = 'threshold/%s/%g' % (R.name, delta)
        check_round(R, st, after, P, parity, tag, bounds=False)
        s = after['scal']
        assert 0.5e-12 < s[STEPINF] < 2e-12 and (s[STEPINF] < 1e-12) == bool(want), s[STEPINF]
        assert (s[MODE], s[REVERT], s[BACKTRACKS]) == (BACKTRACK, want, 6.0), tag
        assert same_bits(s[TT], 0.8 * .8)


# ---- the stop table --------------------------------------------------------------------------

def _frozen(R, first):
    """After a stop, three more rounds change nothing (the SpMVs rewrite r
    and g_new to the same values); with L-BFGS, s, y and the whole of lb too."""
    R.eng.rounds(3)
    again = R.read()
    assert again['lb'].size == (2 * R.C + 8 if R.C else 0)
    for k in ('scal', 'x', 'g', 'xn', 'gn', 'r', 'hist', 'lb') + (('sv', 'yv') if R.C else ()):
        assert nan_bits(again[k], first[k]), k


@pytest.mark.parametrize('key', [BB_RIGS[0], BB_RIGS[2], BB_RIGS[3]], ids=IDS)
def test_stop_table(cuda, parity, key):
    R = rig(cuda, key[0], key[1], ball=key[2])
    vec = X.planted_vectors(R.n, seed=16)
    base = dict(MODE=BACKTRACK, ITER=8.0, TT=0.8, REVERT=0.0)
    learn = R.run(R.state(vec, **base), R.params())['scal']
    f_new, gd = .5 * learn[SQ], learn[GD]
    Fv = f_new + 1.0 + 1e-4 * abs(gd)                          # accepts; |F - f_new| > 1
    gap = Fv - f_new
    yes = dict(max_iter=9, f_min=f_new, prog_tol=2.0 * gap)
    no = dict(max_iter=10 ** 6, f_min=f_new - 1.0, prog_tol=1e-12)
    table = [((), 0), (('max_iter',), MAXITER), (('f_min',), OPT), (('prog_tol',), PROG),
             (('max_iter', 'f_min'), OPT), (('max_iter', 'prog_tol'), PROG),
             (('f_min', 'prog_tol'), PROG), (('max_iter', 'f_min', 'prog_tol'), PROG)]
    for on, reason in table:
        P = R.params(**{k: (yes if k in on else no)[k] for k in yes})
        st = R.state(vec, F=Fv, **base)
        after = R.run(st, P)
        tag = 'stop/%s/%s' % (R.name, '+'.join(on) or 'none')
        check_round(R, st, after, P, parity, tag, bounds=False)
        s = after['scal']
        assert (s[STOP], s[MODE], s[ITER]) == (reason, STOPPED if reason else STEP, 9.0), tag
        assert same_bits(s[F], f_new) and same_bits(s[FOLD], Fv) and s[ROUNDS] == 42.0
        if reason:
            _frozen(R, after)
    # no f_min at all, and max_iter = 0: nothing matches
    for P in (R.params(max_iter=9, f_min=None, prog_tol=1e-12, opt_tol=1e30),
              R.params(max_iter=0)):
        st = R.state(vec, F=Fv, **base)
        after = R.run(st, P)
        check_round(R, st, after, P, parity, 'stop/%s/no-f_min,max_iter=%d' % (
            R.name, P['max_iter']), bounds=False)
        want = MAXITER if P['max_iter'] == 9 else 0
        assert after['scal'][STOP] == want and after['scal'][ITER] == st['scal'][ITER] + 1.0
    # the INIT round
    x0 = {k: vec['x'] for k in ('x', 'g', 'xn', 'gn')}
    x0['g'] = vec['g']
    for P, reason in ((R.params(max_iter=1), MAXITER), (R.params(f_min=1e300), OPT),
                      (R.params(max_iter=0), 0), (R.params(max_iter=1, f_min=1e300), OPT),
                      (R.params(max_iter=1, prog_tol=np.inf), MAXITER)):
        st = R.state(x0, MODE=INIT, ITER=55.0, F=77.0, T=9.0, TT=0.5)
        after = R.run(st, P)
        tag = 'stop/%s/init/max_iter=%g,f_min=%s,prog_tol=%g' % (R.name, P['max_iter'],
                                                                  P['f_min'], P['prog_tol'])
        check_round(R, st, after, P, parity, tag)
        s = after['scal']
        assert (s[STOP], s[MODE], s[ITER], s[FOLD], s[T], s[TT]) == (
            reason, STOPPED if reason else STEP, 1.0, np.inf, 1.0, 1.0), tag
        assert same_bits(after['hist'][0], s[F]) and s[F] == .5 * s[SQ]
        assert same_bits(after['hist'][1:], st['hist'][1:]) and same_bits(after['xn'], vec['x'])
        assert same_bits(after['g'], vec['g'])                 # INIT leaves g alone
        if reason:
            _frozen(R, after)


# ---- the revert gets f and g back ---------------------------------------------------------------

@pytest.mark.parametrize('big', [False, True], ids=['x0<=1', 'x0>1'])
@pytest.mark.parametrize('key', BB_RIGS, ids=IDS)
def test_revert_reproduces_f_and_g(cuda, key, big):
    """What the revert exit rests on: a REVERT = 1 round recomputes obj(x) and
    gets f and g back bit for bit, so f_new > f + 0 is false, the round
    accepts with a zero step and the PROG test ends the run.  Through
    eng.start / eng.rounds, so that the fixed-point residual runs with the
    x_bound shortcut start() arms."""
    R = rig(cuda, key[0], key[1], ball=key[2])
    rs = np.random.RandomState(17)
    x0 = np.repeat(1.0 / R.sizes, R.sizes)
    if big:
        x0 = x0 + rs.uniform(0.0, 3.0, size=R.n)
        assert x0.max() > 1.0
    P = R.params()
    R.start(x0, P)
    if R.kind == 'tiles_fixed':
        assert R.eng._xb >= max(1.0, x0.max())
    R.eng.rounds(1)
    init = R.read()
    s = init['scal']
    assert (s[MODE], s[ITER]) == (STEP, 1.0) and same_bits(init['xn'], x0)
    f0, g0 = s[F], init['gn']
    # the state after some rejected steps from x0: g = g_new(x0), another x_new
    st = R.state(dict(x=x0, g=g0, xn=rs.uniform(0.0, 1.0, size=R.n), gn=np.full(R.n, 3.0)),
                 MODE=BACKTRACK, REVERT=1.0, F=f0, ITER=4.0, TT=0.8 ** 30)
    R.plant(st)
    R.eng.rounds(1)
    after = R.read()
    s = after['scal']
    assert same_bits(.5 * s[SQ], f0) and same_bits(after['gn'], g0) and same_bits(after['xn'], x0)
    assert same_bits(after['r'], init['r'])
    assert s[GD] == 0.0 and s[DXDG] == 0.0 and s[DGDG] == 0.0 and math.isnan(s[T])
    assert (s[MODE], s[STOP], s[ITER], s[BACKTRACKS]) == (STOPPED, PROG, 5.0, 5.0)
    assert same_bits(s[F], f0) and same_bits(s[FOLD], f0)


# ---- L-BFGS -----------------------------------------------------------------------------------------

def lbfgs_checks(R, vec, it, parity, tag):
    C = R.C
    st = R.state(vec, MODE=STEP, ITER=float(it), T=0.0123)
    P = R.params()
    after = R.run(st, P)
    check_round(R, st, after, P, parity, tag)
    assert same_bits(after['x'], vec['xn']) and same_bits(after['g'], vec['gn'])
    lb = after['lb']
    if it <= 5:
        assert same_bits(lb[C:], st['lb'][C:])                  # coefficients untouched
        xo = vec['xn'] + (-0.0123) * vec['gn']                   # the BB point
        X.project(xo, R.starts, R.proj_kind)
        assert same_bits(after['xn'], xo), tag
        assert same_bits(after['sv'], st['sv']) and same_bits(after['yv'], st['yv'])
        return after
    sv, yv = vec['xn'] - vec['x'], vec['gn'] - vec['g']
    assert same_bits(after['sv'], sv) and same_bits(after['yv'], yv), tag
    a, b, c, t = lb[2 * C:2 * C + 4]
    d_dev = -((a * vec['gn'] + b * sv) + c * yv)
    rhos = X.ring_rhos(st['lb'], it, C)
    d_ref = X.lbfgs_direction(vec['gn'], sv, yv, rhos, dtype=LD)
    scale = float(np.max(np.abs(d_ref)))
    # the condition on the inputs: the reference recursion itself is stable here
    d_dbl = X.lbfgs_direction(vec['gn'], sv, yv, rhos)
    assert float(np.max(np.abs(d_dbl - d_ref))) <= 1e-12 * scale
    if C > 1:
        # ... and a wrong ring slot shows: two slots exchanged move d by > 1e-8
        p, q = X.swap_pairs(C, it)
        lb2 = st['lb'].copy()
        lb2[p], lb2[q] = st['lb'][q], st['lb'][p]
        d_swap = X.lbfgs_direction(vec['gn'], sv, yv, X.ring_rhos(lb2, it, C), dtype=LD)
        assert float(np.max(np.abs(d_swap - d_ref))) > 1e-8 * scale, tag
    parity('%s/direction' % tag, float(np.max(np.abs(d_dev - d_ref))) / scale, 1e-11)
    assert abs(t - sv.dot(yv) / yv.dot(yv)) <= 1e-12 * abs(t)
    xo = vec['xn'] + d_dev
    X.project(xo, R.starts, R.proj_kind)
    assert same_bits(after['xn'], xo), tag
    return after


LBFGS_CASES = [(C, it) for C in X.LBFGS_CS for it in X.lbfgs_iters(C)]


@pytest.mark.parametrize('C,it', LBFGS_CASES)
def test_lbfgs_round(cuda, parity, C, it):
    R = rig(cuda, 'Podd', 'csr', C=C)
    vec = X.lbfgs_case(R.n, C, it, seed=7 * C + it)
    after = lbfgs_checks(R, vec, it, parity, 'lbfgs/%s/it%d' % (R.name, it))
    s = after['scal']
    assert s[ITER] == it + 1.0 and same_bits(after['lb'][(it - 1) % C], 1.0 / s[DXDG])


@pytest.mark.parametrize('key', [('Peven', 'tiles_fixed', False), ('Peven', 'panels', True)]
                         + GRID_RIGS, ids=IDS)
def test_lbfgs_round_other_operators_and_grids(cuda, parity, key):
    R = rig(cuda, key[0], key[1], ball=key[2], C=3)
    for it in (5, 7):
        vec = X.lbfgs_case(R.n, 3, it, seed=40 + it)
        lbfgs_checks(R, vec, it, parity, 'lbfgs/%s/it%d' % (R.name, it))


LB_STOP_RIGS = [('Podd', 'csr', False, 3), ('Peven', 'tiles_fixed', False, 3),
                ('Podd', 'csr', False, 1)]


@pytest.mark.parametrize('key', LB_STOP_RIGS, ids=IDS)
def test_lbfgs_stop_then_frozen(cuda, parity, key):
    """An accepting L-BFGS STEP round that stops (max_iter = ITER + 1), on the
    recursion (ITER 7) and on the BB branch (ITER 4); three more rounds then
    leave scal, x, g, x_new, g_new, r, s, y, hist and the whole of lb as they
    are -- xlb_step, xlb_dir and the finish return at once."""
    R = rig(cuda, key[0], key[1], ball=key[2], C=key[3])
    for it in (7, 4):
        vec = X.lbfgs_case(R.n, R.C, it, seed=60 + it)
        st = R.state(vec, MODE=STEP, ITER=float(it), T=0.0123)
        P = R.params(max_iter=it + 1)
        after = R.run(st, P)
        check_round(R, st, after, P, parity, 'lbfgs-stop/%s/it%d' % (R.name, it))
        s = after['scal']
        assert (s[MODE], s[STOP], s[ITER], s[TT]) == (STOPPED, MAXITER, it + 1.0, 1.0)
        if it > 5:
            assert same_bits(after['sv'], vec['xn'] - vec['x'])
        _frozen(R, after)


@pytest.mark.parametrize('key', [('Podd', 'csr', False, 0), ('Podd', 'tiles_fixed', False, 0)]
                         + LB_STOP_RIGS, ids=IDS)
def test_planted_stopped_state_is_inert(cuda, parity, key):
    """MODE = STOPPED planted with a TT and REVERT that a BACKTRACK round would
    act on, and an ITER on either side of 5: a round changes no slot but SQ
    and no vector but r and g_new, which the SpMVs set to A x_new - b, its
    ||r||^2 and A' r."""
    R = rig(cuda, key[0], key[1], ball=key[2], C=key[3])
    vec = X.lbfgs_case(R.n, R.C, 7, seed=70) if R.C else X.planted_vectors(R.n, seed=70)
    P = R.params()
    for it, tt, revert in ((7.0, 0.5, 0.0), (7.0, 0.5, 1.0), (3.0, 0.64, 0.0)):
        st = R.state(vec, MODE=STOPPED, ITER=it, TT=tt, REVERT=revert, T=0.37, STOP=PROG)
        after = R.run(st, P)
        tag = 'stopped/%s/it%d,tt%g,revert%d' % (R.name, it, tt, revert)
        check_round(R, st, after, P, parity, tag)
        keep = [q for q in range(X.COUNT) if q != SQ]            # (SQ: the residual's own)
        assert same_bits(after['scal'][keep], st['scal'][keep])
        assert same_bits(after['xn'], vec['xn'])
        _frozen(R, after)


# ---- NaN ------------------------------------------------------------------------------------------------

def test_nan_in_a_backtrack_round(cuda, parity):
    """One NaN in x_new on a BACKTRACK round (no projection sees it): STEPINF
    and SQ are NaN, and the round accepts -- `while f_new > upper` is false
    for a NaN f_new."""
    R = rig(cuda, 'Podd', 'csr')
    vec = dict(X.planted_vectors(R.n, seed=18))
    vec['xn'] = vec['xn'].copy()
    vec['xn'][R.n // 3] = np.nan
    for Fv in (1e300, -1e300, 0.0):
        st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=0.8, REVERT=0.0, F=Fv)
        P = R.params(f_min=0.0)
        after = R.run(st, P)
        check_round(R, st, after, P, parity, 'nan/%s' % R.name, bounds=False)
        s = after['scal']
        assert math.isnan(s[STEPINF]) and math.isnan(s[SQ]) and math.isnan(s[F])
        assert math.isnan(s[GD]) and math.isnan(s[DXDG])
        assert (s[MODE], s[REVERT], s[STOP], s[ITER], s[BACKTRACKS]) == (STEP, 0.0, 0.0, 8.0, 5.0)
        assert np.isnan(after['xn']).sum() == 1 and math.isnan(after['hist'][7])


# ---- the grid-stride problem ------------------------------------------------------------------------------

def test_grid_stride_bb(cuda, parity):
    """n = 2 (1048576 + 2048 + 300) + 1: xbb_step and xbb_finish stride, the
    finish grid's second pass is partly filled with clamped loads, the tail is
    odd.  A BACKTRACK round with tt = 1/2 on a dyadic grid: all five sums bit
    for bit (exact in any order: asserted in integers by dyadic_bb_case); then
    a STEP round on generic vectors, the sums within their bounds."""
    R = rig(cuda, 'stride', 'csr')
    c = _PROBLEMS['stride-case']
    assert R.n == X.STRIDE_N and X.finish_grid(R.n) == X.step_grid(R.n) == 1024
    vec = dict(x=c['x'], g=c['g'], xn=c['xn'], gn=np.full(R.n, 3.0))
    st = R.state(vec, MODE=BACKTRACK, ITER=7.0, TT=0.5, REVERT=0.0)
    P = R.params()
    after = R.run(st, P)
    check_round(R, st, after, P, parity, 'stride/bb/dyadic', bounds=False)
    assert same_bits(after['xn'], c['xa']) and same_bits(after['r'], c['r'])
    assert same_bits(after['gn'], c['gn'])
    s = after['scal']
    for name, v in c['want'].items():
        assert same_bits(s[getattr(X, name)], v), (name, s[getattr(X, name)], v)
    assert same_bits(s[T], c['want']['DXDG'] / c['want']['DGDG'])
    vec = X.planted_vectors(R.n, seed=19)
    st = R.state(vec, MODE=STEP, ITER=7.0, T=0.0123)
    after = R.run(st, P)
    check_round(R, st, after, P, parity, 'stride/bb/step')
    assert same_bits(after['x'], vec['xn']) and same_bits(after['g'], vec['gn'])


def test_grid_stride_lbfgs(cuda, parity):
    """xlb_step and xlb_dir striding (C = 3, iteration 7) on a dyadic grid:
    g.s, g.y, s.y, y.y are exact in any order, so the coefficients and alpha
    must be the host's scalar recursion bit for bit; the finish sums (after
    the projection, no longer dyadic) within their bounds."""
    C, it = 3, 7
    R = rig(cuda, 'stride', 'csr', C=C)
    vec = X.dyadic_lbfgs_case(R.n, C, it)
    after = lbfgs_checks(R, vec, it, parity, 'stride/lbfgs')
    lb0 = np.zeros(2 * C + 8)
    lb0[:C] = vec['rho']
    coef, alpha = X.lbfgs_coefficients(*vec['sums'], lb0, it, C)
    assert same_bits(after['lb'][2 * C:2 * C + 4], np.array(coef))
    # (the finish has since written rho of iteration 8 into the ring, not alpha)
    assert same_bits(after['lb'][C:2 * C], np.array([alpha[q] for q in range(C)]))
