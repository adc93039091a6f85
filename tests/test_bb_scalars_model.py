"""The reference model of tests/test_gpu_bb_scalars.py, and its own checks on
the CPU: the exact sums the engine's scal[] slots are compared with, the
planted inputs, the slices of ||r||^2, the WARN boundaries of BB.py:27 and the
table that drives the stop rule (solvers.py:40-63, `oracle.stopping`).

Exact sums.  Every double is a rational, so the products and their sum are
formed in fractions.Fraction without any rounding and rounded once to the
reference double.  A device sum of k terms, in whatever order and with or
without fused multiply-adds, satisfies

    |got - ref| <= (k + 4) u sum|terms|,   u = 2^-53

(one rounding per product, k - 1 per addition chain, one for the reference;
the form tests/test_gpu_xspace_kernels.py uses) -- derived, not measured.

Term sizes.  A dropped or doubled term t moves the sum by |t|; the check sees
it when |t| exceeds twice the bound.  For the planted sums (sum dg, dz.dg,
dg.dg, the r^2 slices) every term is at least 2^-10 of the largest, hence at
least sum|terms| / (1024 k): with k <= 3k that is 1e9 times the bound.  g.g
cannot be planted term by term -- g = N'A'r is the image of the 321 planted
rows of r, with exact zeros where a route's rows of A' are empty -- so for it
the condition asserted is the one the argument needs: every term is 0 or at
least four times the bound (`detectable`).

For the same reason g_prev is planted as (host N'A'r) - d with d of random sign
and |d| in [0.25, 4], not as a vector of that size itself: dg = g - g_prev is
then d to rounding and its terms meet the 2^-10 condition, which they could
not with |g| up to some hundreds against |g_prev| <= 4.
"""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import numpy.linalg as la
import pytest

U = Fraction(1, 2 ** 53)
STOP_NOCHANGE, STOP_MAXITER, STOP_GRAD, STOP_DG = 1, 2, 3, 4

ExactSum = namedtuple('ExactSum', 'ref exact sumabs k')


def exact_sum(a, b=None):
    """sum_j a_j (b = None) or sum_j a_j b_j, exactly: the reference double
    (rounded once), the rational itself, sum |terms| and the term count."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if b is None:
        terms = [Fraction(v) for v in a.tolist()]
    else:
        b = np.asarray(b, dtype=np.float64).reshape(-1)
        assert a.shape == b.shape
        terms = [Fraction(v) * Fraction(w) for v, w in zip(a.tolist(), b.tolist())]
    tot = sum(terms, Fraction(0))
    sumabs = sum((abs(t) for t in terms), Fraction(0))
    return ExactSum(float(tot), tot, sumabs, len(terms))     # int / int: correctly rounded


def bound(es):
    """(k + 4) u sum|terms|, a Fraction."""
    return (es.k + 4) * U * es.sumabs


def error(got, es):
    return abs(Fraction(float(got)) - Fraction(es.ref))


def within(got, es):
    return math.isfinite(float(got)) and error(got, es) <= bound(es)


def terms_ok(terms):
    """Every term at least 2^-10 of the largest (none zero)."""
    t = np.abs(np.asarray(terms, dtype=np.float64))
    return bool(t.size and t.min() > 0.0 and t.min() >= t.max() * 2.0 ** -10)


def detectable(terms):
    """Every term 0 or at least four times the bound of its sum; returns
    (ok, number of zero terms)."""
    t = np.abs(np.asarray(terms, dtype=np.float64))
    es = exact_sum(t)
    nz = t[t > 0.0]
    ok = bool(nz.size and Fraction(float(nz.min())) >= 4 * bound(es))
    return ok, int(t.size - nz.size)


# ---- planted inputs -----------------------------------------------------------

def signed(rs, n, lo=0.25, hi=4.0):
    """n values of random sign, |value| uniform in [lo, hi)."""
    return rs.choice([-1.0, 1.0], size=n) * rs.uniform(lo, hi, size=n)


def z_rows(sizes):
    """The x row of every z coordinate (a block's last route has none)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    keep = np.ones(int(sizes.sum()), dtype=bool)
    keep[np.cumsum(sizes) - 1] = False
    return np.flatnonzero(keep)


def host_gradient(A, sizes, r):
    """N'A'r with SciPy: g_j = w_i - w_{i+1}, w = A'r, i = z_rows[j]."""
    w = A.T.tocsr().dot(np.asarray(r, dtype=np.float64))
    i = z_rows(sizes)
    return w[i] - w[i + 1]


def planted(A, sizes, seed):
    """r, dz, the dg the sums should see (d) and g_prev = host g - d, for both
    parities the same; x for the K1 stages (|entries| in [0.25, 1])."""
    rs = np.random.RandomState(seed)
    m, n = A.shape
    nz = n - len(sizes)
    r = signed(rs, m)
    gh = host_gradient(A, sizes, r)
    d = signed(rs, nz)
    return dict(r=r, gh=gh, d=d, g_prev=gh - d, dz=signed(rs, nz),
                x=rs.uniform(0.25, 1.0, size=n), z=rs.uniform(0.0, 1.0, size=nz),
                g_step=signed(rs, nz))


# ---- the slices of ||r||^2 (stage 10, bsls_bb_k2_part) ---------------------------

SLICE_K = 200     # the one-row slice (k, k + 1)
SHORT = (100, 102)  # shorter than any engine's number of K2 workgroups (>= 3)


def slices(m):
    return [(0, 0), (0, m), (1, m - 1), (107, 214), (SLICE_K, SLICE_K + 1), (m - 5, m), SHORT]


def slice_rows(m, lo, hi):
    """The rows a slice sums: hi > lo cuts, anything else is the whole of r
    (bb.hip: cut = rr_hi > rr_lo)."""
    return (lo, hi) if hi > lo else (0, m)


def slice_r(r, lo, hi):
    """r with the two rows just outside the slice at +-64 (their squares,
    4096, are what a one-row overreach adds)."""
    out = np.array(r, dtype=np.float64)
    a, b = slice_rows(out.shape[0], lo, hi)
    if a > 0:
        out[a - 1] = 64.0
    if b < out.shape[0]:
        out[b] = -64.0
    return out


# ---- BB.py:27 -------------------------------------------------------------------

def warns(t):
    return abs(t) <= 1e-10 or abs(t) > 1e10


def warn_table():
    """(t, whether the WARN count grows): both boundaries from both sides,
    both signs, and a large finite step."""
    rows = []
    for s in (1.0, -1.0):
        rows += [(s * 1e-10, True), (s * math.nextafter(1e-10, 1.0), False), (s * 1e10, False),
                 (s * math.nextafter(1e10, math.inf), True), (s * 1e300, True)]
    return rows


# ---- the stop rule ---------------------------------------------------------------

StopRow = namedtuple('StopRow', 'name it max_iter opt_tol rr gg dgdg early_exit')


def fx_of(rr):
    nr = math.sqrt(rr)
    return 0.5 * (nr * nr)              # 0.5 * la.norm(r)**2, main.py:53


def threshold(opt_tol, rr):
    return opt_tol * (1 + abs(fx_of(rr)))


def stop_table():
    big, M = 1e6, 100
    t6 = threshold(0.5, 6.0)
    rows = [
        StopRow('before-max-iter', M - 1, M, 1e-30, 6.0, big, 1.0, 1),
        StopRow('at-max-iter', M, M, 1e-30, 6.0, big, 1.0, 1),
        # sqrt(2)**2 = 2.0000000000000004 > 2: no stop (gg <= 2 would stop)
        StopRow('gg-2-thr-2', 5, M, 2.0, 0.0, 2.0, 1.0, 1),
        StopRow('gg-below-thr', 5, M, 0.5, 6.0, math.nextafter(t6, 0.0), 1.0, 1),
        StopRow('gg-at-thr', 5, M, 0.5, 6.0, t6, 1.0, 1),
        StopRow('gg-above-thr', 5, M, 0.5, 6.0, math.nextafter(t6, math.inf), 1.0, 1),
        StopRow('dgdg-zero', 5, M, 1e-30, 6.0, big, 0.0, 1),
        StopRow('dgdg-denormal', 5, M, 1e-30, 6.0, big, 5e-324, 1),
        StopRow('max-iter-over-grad-dg', M, M, 0.5, 6.0, 1e-3, 0.0, 1),
        StopRow('grad-over-dg', 5, M, 0.5, 6.0, 1e-3, 0.0, 1),
        StopRow('no-early-exit', 5, M, 0.5, 6.0, 1e-3, 0.0, 0),
        StopRow('no-early-exit-max-iter', M, M, 0.5, 6.0, 1e-3, 0.0, 0),
    ]
    assert threshold(2.0, 0.0) == 2.0
    return rows


def vec_with_sq(v):
    """A vector whose la.norm is sqrt(v) -- for v = 2 the one whose squares
    sum to it exactly, (1, 1); else the one entry sqrt(v) (sqrt(fl(s * s)) = s)."""
    x = np.array([1.0, 1.0]) if v == 2.0 else np.array([math.sqrt(v)])
    assert la.norm(x) == math.sqrt(v), v
    return x


def r_with_sq(m, rr):
    """r of m rows whose squares sum to the small integer rr exactly, in any order."""
    r = np.zeros(m)
    k, left = 0, int(rr)
    assert left == rr and left >= 0
    while left:
        s = math.isqrt(left)
        r[k] = float(s)
        left -= s * s
        k += 1
    return r


def oracle_reason(row, stopping):
    """The engine's stop code for a row, decided by `oracle.stopping` on
    vectors with the row's norms: which of its clauses returns, in its order."""
    fx = fx_of(row.rr)
    opts = {'max_iter': row.max_iter, 'opt_tol': row.opt_tol}
    # its first clause alone: a gradient no tolerance of the table passes, no
    # delta_g -- all that the loop with the early exits off keeps
    assert row.opt_tol * (1 + abs(fx)) < 1e300
    if stopping(np.array([1e150]), fx, row.it, 1.0, options=opts):
        return STOP_MAXITER
    if not row.early_exit:
        return 0
    g, dg = vec_with_sq(row.gg), vec_with_sq(row.dgdg)
    if not stopping(g, fx, row.it, 1.0, delta_g=dg, options=opts):
        return 0
    return STOP_GRAD if stopping(g, fx, row.it, 1.0, options=opts) else STOP_DG


def device_rule(row, gg_itself=False):
    """bb_stop_reason (csrc/bb.hip) restated; gg_itself: the mutant that tests
    gg where the reference tests sqrt(gg)**2."""
    if row.it >= row.max_iter:
        return STOP_MAXITER
    if row.early_exit:
        gn = math.sqrt(row.gg)
        if (row.gg if gg_itself else gn * gn) <= row.opt_tol * (1 + abs(fx_of(row.rr))):
            return STOP_GRAD
        if math.sqrt(row.dgdg) == 0:
            return STOP_DG
    return 0


# ---- the model's own checks --------------------------------------------------------

def test_exact_sum_against_fsum():
    """On exactly representable inputs (integers times powers of two, products
    below 2^53 apart) the exact sum is math.fsum's, and both equal the integer
    arithmetic."""
    rs = np.random.RandomState(7)
    a = rs.randint(-2 ** 20, 2 ** 20, size=3001).astype(np.float64) * 2.0 ** -7
    b = rs.randint(-2 ** 20, 2 ** 20, size=3001).astype(np.float64) * 2.0 ** 3
    es = exact_sum(a)
    assert es.ref == math.fsum(a.tolist()) == float(int((a * 2.0 ** 7).astype(np.int64).sum())) / 128
    assert es.k == 3001 and es.sumabs == Fraction(math.fsum(np.abs(a).tolist()))
    ep = exact_sum(a, b)
    prod = (a * 2.0 ** 7).astype(np.int64).astype(object) * (b * 2.0 ** -3).astype(np.int64)
    assert ep.exact == Fraction(int(prod.sum()), 16)
    assert ep.ref == math.fsum((a * b).tolist())           # (each product exact in a double)
    # inexact products: fsum of the rounded products is a different number
    c = rs.rand(500) + 0.5
    ec = exact_sum(c, c)
    assert ec.exact == sum((Fraction(v) ** 2 for v in c.tolist()), Fraction(0))
    assert within(float(np.dot(c, c)), ec) and not within(float(np.dot(c, c)) * (1 + 1e-12), ec)


def test_exact_sum_against_mpmath():
    mpmath = pytest.importorskip('mpmath')
    rs = np.random.RandomState(11)
    a, b = signed(rs, 2700), signed(rs, 2700)
    with mpmath.workprec(4000):
        tot = mpmath.fsum(mpmath.mpf(v) * mpmath.mpf(w) for v, w in zip(a.tolist(), b.tolist()))
        assert mpmath.mpf(exact_sum(a, b).exact.numerator) / exact_sum(a, b).exact.denominator == tot
        with mpmath.workprec(53):
            ref = float(+tot)
    assert exact_sum(a, b).ref == ref


def test_bound_sees_a_dropped_or_doubled_term():
    """What the term-size condition is for: with every term within 2^-10 of
    the largest, leaving one out or adding one twice is outside the bound --
    for the smallest term too."""
    rs = np.random.RandomState(3)
    a, b = signed(rs, 2700), signed(rs, 2700)
    assert terms_ok(a * b) and terms_ok(a * a) and terms_ok(a)
    for es, t in ((exact_sum(a, b), a * b), (exact_sum(a, a), a * a), (exact_sum(a), a)):
        j = int(np.argmin(np.abs(t)))
        assert within(es.ref, es)
        assert not within(es.ref - t[j], es) and not within(es.ref + t[j], es)
        assert Fraction(float(abs(t[j]))) > 10 ** 6 * bound(es)
    assert not terms_ok(np.array([1.0, 2.0 ** -11])) and not terms_ok(np.array([1.0, 0.0]))
    ok, zeros = detectable(np.array([0.0, 1.0, 1e-9, 3.0]))
    assert ok and zeros == 1
    assert not detectable(np.array([1.0, 1e-15]))[0]


@pytest.fixture(scope='module', params=[321, 320], ids=['m321', 'm320'])
def case(request):
    from test_gpu_handoffs import make_problem
    m = request.param
    A, b, sizes = make_problem(m, seed=31 + m)
    return A, b, sizes, planted(A, sizes, seed=1000 + m)


def test_planted_inputs_meet_the_term_size_conditions(case):
    A, b, sizes, pl = case
    m, n = A.shape
    nz = n - len(sizes)
    assert pl['g_prev'].shape == pl['dz'].shape == (nz,) and pl['r'].shape == (m,)
    for v in (pl['r'], pl['d'], pl['dz'], pl['g_step']):
        assert np.all((np.abs(v) >= 0.25) & (np.abs(v) < 4.0))
    dg = pl['gh'] - pl['g_prev']                 # what the device forms, to g's rounding
    assert np.max(np.abs(dg - pl['d'])) <= 1e-9
    assert terms_ok(dg) and terms_ok(pl['dz'] * dg) and terms_ok(dg * dg)
    ok, zeros = detectable(pl['gh'] * pl['gh'])
    assert ok and 0 < zeros < nz // 4            # (the routes whose rows of A' are empty)
    # K1's r = A x + target at the planted x (stage 7)
    x0 = np.zeros(n)
    x0[np.cumsum(sizes) - 1] = 1.0
    r7 = A.dot(pl['x']) + (A.dot(x0) - b)
    assert terms_ok(r7 * r7)
    # stage 2's r + target
    r2 = pl['r'] + (A.dot(x0) - b)
    assert detectable(r2 * r2) == (True, 0)


def test_slices_and_their_neighbours(case):
    A, b, sizes, pl = case
    m = A.shape[0]
    seen = set()
    for lo, hi in slices(m):
        a, c = slice_rows(m, lo, hi)
        assert 0 <= a < c <= m
        r = slice_r(pl['r'], lo, hi)
        assert terms_ok(r[a:c] * r[a:c])
        assert np.array_equal(r[a:c], pl['r'][a:c])
        es = exact_sum(r[a:c], r[a:c])
        for j in ([a - 1] if a > 0 else []) + ([c] if c < m else []):
            assert abs(r[j]) == 64.0
            assert not within(es.ref + r[j] * r[j], es)          # a one-row overreach
        for j in (a, c - 1):                                      # a one-row shortfall
            assert not within(es.ref - r[j] * r[j], es)
        seen.add((a > 0, c < m, c - a))
    assert slice_rows(m, 0, 0) == (0, m) and SHORT[1] - SHORT[0] < 3
    assert {s[:2] for s in seen} == {(False, False), (True, True), (True, False)}
    # (107, 214) straddles row 128, a bound of K1's 64-row blocks and so of the
    # link parts (the GPU test checks it against the engine's group_col)
    assert 107 < 128 < 214


def test_warn_boundaries():
    """The two comparisons of BB.py:27, `abs(t) <= 1e-10 or abs(t) > 1e10`."""
    tab = warn_table()
    assert len(tab) == 10 and all(math.isfinite(t) for t, _ in tab)
    for t, grows in tab:
        assert warns(t) == grows, t
    assert [g for _, g in tab[:5]] == [True, False, False, True, True]
    # `<` for `<=` changes exactly the rows at +-1e-10
    assert [t for t, g in tab if (abs(t) < 1e-10 or abs(t) > 1e10) != g] == [1e-10, -1e-10]


def test_stop_table_against_the_oracle(orc):
    rows = stop_table()
    want = {r.name: oracle_reason(r, orc.stopping) for r in rows}
    for r in rows:
        assert device_rule(r) == want[r.name], r
        assert np.sum(r_with_sq(321, r.rr) ** 2) == r.rr
    # what the rows were written for (the three at the threshold: as the
    # oracle decides; below it stops, and somewhere from there on it does not)
    at = [want.pop(k) for k in ('gg-below-thr', 'gg-at-thr', 'gg-above-thr')]
    assert at[0] == STOP_GRAD and set(at) == {STOP_GRAD, 0} and at == sorted(at, reverse=True)
    assert want == {'before-max-iter': 0, 'at-max-iter': STOP_MAXITER, 'gg-2-thr-2': 0,
                    'dgdg-zero': STOP_DG, 'dgdg-denormal': 0,
                    'max-iter-over-grad-dg': STOP_MAXITER, 'grad-over-dg': STOP_GRAD,
                    'no-early-exit': 0, 'no-early-exit-max-iter': STOP_MAXITER}
    want = {r.name: oracle_reason(r, orc.stopping) for r in rows}
    # the row the mutant `gg <= threshold` gets wrong
    wrong = [r.name for r in rows if device_rule(r, gg_itself=True) != want[r.name]]
    assert 'gg-2-thr-2' in wrong
