"""The host model of one round of the fused x-space BB / L-BFGS engine
(csrc/xbb.hip, device.XBBEngine), and its own checks on the CPU.  The GPU
side is tests/test_gpu_xbb_rounds.py.

round_model restates the state machine of bsls_xbb_rounds in NumPy doubles,
with the elementwise roundings of the reference (python/BATCH.py:55-214,
python/algorithm_utils.py:88-94,113-137,158-172) and of xbb.hip, which is built
without fused multiply-adds:

    x + (-t)*g     (1-tt)*x + tt*x_new     x_new = x on a revert
    f_new = .5*sq  upper = f + 1e-4*gd     t = dxdg/dgdg     tt *= .8
    revert = stepinf < 1e-12               reject iff f_new > upper

The five sums of a round (||r||^2, g.(x_new - x), dx.dg, dg.dg, ||dx||_inf),
r and g_new come from SciPy / NumPy, or from the caller (`dev`): the GPU test
feeds the device's own sums, so that every decision slot has to match bit for
bit although the device adds in another order.

What validates the model: iterated from INIT with SciPy products, the oracle's
projection and NumPy dots it reproduces oracle.batch_solve_bb and
oracle.batch_solve_lbfgs (the reference's loops restated, oracle/oracle.py)
bit for bit -- x, f, iterations, the stop string, every progress value and the
number of backtracks -- on runs that backtrack and end by the line search's
revert, with rings that are not full, full and wrapped.

Also here: the L-BFGS direction over queues that all hold the one (s, y)
(LBFGS_helper, BATCH.py:196-214) in double and long double with the planted
rings of the GPU test and their conditioning; the doubles F around the Armijo
boundary fl(F + 1e-4 gd) == f_new; the problems of the GPU test; a fast exact
dot (two-product + math.fsum) for the 2M-entry case.  exact_sum, bound, within
and terms_ok are test_bb_scalars_model's.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sps

import test_bb_scalars_model as M
from test_bb_scalars_model import bound, exact_sum, terms_ok, within

(MODE, ITER, F, FOLD, T, TT, REVERT, GD, DXDG, DGDG, STEPINF, SQ, STOP, ROUNDS,
 BACKTRACKS) = range(15)
COUNT = 16
INIT, STEP, BACKTRACK, STOPPED = range(4)
MAXITER, OPT, PROG = 1, 2, 3
DECISIONS = (MODE, ITER, F, FOLD, T, TT, REVERT, STOP, ROUNDS, BACKTRACKS)
LD = np.longdouble

# the launch geometry of csrc/xbb.hip
XT, XGRID, XU = 256, 1024, 4


def step_grid(n):
    return min(max(-(-n // XT), 1), XGRID)


def finish_grid(n):
    return min(max(-(-(n >> 1) // (XT * XU)), 1), XGRID)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the stop rule (algorithm_utils.stopping, :158-172) -----------------------

def stop_reason(i, max_iter, f, f_old, opt_tol, prog_tol, f_min=None):
    """Every test runs; the last true one names the reason."""
    reason = 0
    if i == max_iter:
        reason = MAXITER
    if f_min is not None and f - f_min < opt_tol:
        reason = OPT
    if abs(f_old - f) < prog_tol:
        reason = PROG
    return reason


def stop_string(reason, f, f_old, f_min):
    """The reference's `stop` for a reason code (as device.XBBEngine.solve)."""
    if reason == MAXITER:
        return 'max_iter'
    if reason == OPT:
        return 'f-f_min = {} < opt_tol'.format(f - f_min)
    assert reason == PROG
    return '|f_old-f| = {} < prog_tol'.format(abs(f_old - f))


# ---- L-BFGS --------------------------------------------------------------------

def ring_rhos(lb, it, C):
    """The rho queue at iteration `it`, oldest first: rho of iteration i' sits
    in slot (i' - 2) % C, the queue holds the last min(it - 1, C) of them."""
    k = int(it) - 1
    m = min(k, C)
    return [lb[(k - m + j) % C] for j in range(m)]


def lbfgs_direction(g, s, y, rhos, dtype=np.float64):
    """LBFGS_helper (BATCH.py:196-214) over queues that all hold the one
    (s, y) and the rho list `rhos` (oldest first), in `dtype`."""
    g, s, y = (np.asarray(v, dtype=dtype) for v in (g, s, y))
    rhos = [dtype(r) for r in rhos]
    m = len(rhos)
    alpha = np.zeros(max(m, 1), dtype=dtype)
    d = g.copy()
    for j in range(1, m + 1):
        alpha[-j] = rhos[-j] * s.T.dot(d)
        d -= alpha[-j] * y
    t = s.T.dot(y) / y.T.dot(y)
    d *= t
    for j in range(m):
        beta = rhos[j] * y.T.dot(d)
        d += s * (alpha[-m + j] - beta)
    d *= dtype(-1.0)
    return d


def lbfgs_coefficients(gs, gy, sy, yy, lb, it, C):
    """xlb_step_kernel's scalar recursion restated operation by operation (no
    fused multiply-adds): (a, b, c, t) of d = -(a g + b s + c y), and alpha by
    ring slot.  Bit-identical to the device given the same four sums."""
    gs, gy, sy, yy = (np.float64(v) for v in (gs, gy, sy, yy))
    k = int(it) - 1
    m = min(k, C)
    alpha = {}
    a, b, c = np.float64(1.0), np.float64(0.0), np.float64(0.0)
    for j in range(1, m + 1):
        q = (k - j) % C
        al = np.float64(lb[q]) * (a * gs + c * sy)
        alpha[q] = al
        c = c - al
    t = sy / yy
    a = a * t
    c = c * t
    for j in range(m):
        q = (k - m + j) % C
        beta = np.float64(lb[q]) * ((a * gy + b * sy) + c * yy)
        b = b + (alpha[q] - beta)
    return (a, b, c, t), alpha


def direction_from_coefficients(coef, g, s, y):
    """xlb_dir_kernel: d = -((a g + b s) + c y)."""
    a, b, c = (np.float64(v) for v in coef[:3])
    return -((a * g + b * s) + c * y)


# ---- one round --------------------------------------------------------------------

def project(x, starts, kind):
    from oracle import oracle
    (oracle.proj_multi_ball_c if kind == 'ball' else oracle.proj_multi_simplex_c)(x, starts)


def new_state(x0, params):
    """bsls_xbb_init after XBBEngine.start: the state before the INIT round."""
    x0 = np.array(x0, dtype=np.float64)
    n, C = x0.size, int(params.get('C', 0))
    scal = np.zeros(COUNT)
    scal[MODE], scal[TT], scal[T] = INIT, 1.0, 1.0
    z = lambda: np.zeros(n)
    return dict(x=x0, g=z(), xn=z(), gn=z(), r=None, scal=scal,
                hist=np.zeros(int(params['hist_cap'])), lb=np.zeros(2 * C + 8 if C else 0),
                sv=z() if C else None, yv=z() if C else None)


def round_model(state, A, AT, b, starts, kind, params, dev=None):
    """One round of bsls_xbb_rounds on a copy of `state`.

    state: x, g, xn, gn, r, scal (16), hist, lb, sv, yv (NumPy doubles).
    kind: 'simplex' or 'ball'.  params: max_iter, opt_tol, prog_tol, f_min
    (None: no such test), hist_cap, C (0: BB).  dev: what the device itself
    computed in this round, taken in place of the host's -- 'SQ', 'GD',
    'DXDG', 'DGDG', 'STEPINF', 'r', 'gn', and for an L-BFGS round 'coef'
    (a, b, c) and 'lb' (its alpha and coefficient slots are copied; the rho
    ring stays the model's)."""
    dev = dev or {}
    st = {k: (None if v is None else np.array(v, dtype=np.float64)) for k, v in state.items()}
    s = st['scal']
    mode = int(s[MODE])
    x, g, xn, gn = st['x'], st['g'], st['xn'], st['gn']
    if mode == STOPPED:
        # every launch returns at once but the two SpMVs, which recompute r,
        # ||r||^2 and g_new at the final x_new (the same values after a stop)
        if 'r' in dev:
            st['r'] = np.array(dev['r'], dtype=np.float64)
            gn[:] = dev['gn']
        else:
            st['r'] = A.dot(xn) - b
            gn[:] = AT.dot(st['r'])
        s[SQ] = dev['SQ'] if 'SQ' in dev else st['r'].T.dot(st['r'])
        return st
    C = int(params.get('C', 0))
    if mode == INIT:
        xn[:] = x
    elif mode == STEP:
        if C > 0 and s[ITER] > 5.0:
            st['sv'][:] = xn - x                      # np.add(x_new, -x, delta_x)
            st['yv'][:] = gn - g
            x[:] = xn
            g[:] = gn
            if 'coef' in dev:
                d = direction_from_coefficients(dev['coef'], g, st['sv'], st['yv'])
            else:
                d = lbfgs_direction(g, st['sv'], st['yv'], ring_rhos(st['lb'], s[ITER], C))
            if 'lb' in dev:
                st['lb'][C:] = np.asarray(dev['lb'])[C:]
            xn[:] = x + d
        else:
            x[:] = xn
            g[:] = gn
            xn[:] = x + (-s[T]) * g
        project(xn, starts, kind)
    else:
        if s[REVERT] != 0.0:
            xn[:] = x
        else:
            tt = s[TT]
            xn[:] = (1.0 - tt) * x + tt * xn
    if 'r' in dev:
        st['r'] = np.array(dev['r'], dtype=np.float64)
        gn[:] = dev['gn']
    else:
        st['r'] = A.dot(xn) - b
        gn[:] = AT.dot(st['r'])
    s[SQ] = dev['SQ'] if 'SQ' in dev else st['r'].T.dot(st['r'])
    f_new = .5 * s[SQ]
    s[ROUNDS] += 1.0
    P = params
    if mode == INIT:
        s[F], s[FOLD], s[ITER], s[T], s[TT] = f_new, np.inf, 1.0, 1.0, 1.0
        if P['hist_cap'] > 0:
            st['hist'][0] = f_new
        r = stop_reason(1.0, P['max_iter'], f_new, np.inf, P['opt_tol'], P['prog_tol'],
                        P.get('f_min'))
        s[STOP] = r
        s[MODE] = STOPPED if r else STEP
        return st
    dx = xn - x
    s[GD] = dev['GD'] if 'GD' in dev else g.dot(dx)
    s[STEPINF] = dev['STEPINF'] if 'STEPINF' in dev else (np.max(np.abs(dx)) if dx.size else 0.0)
    upper = s[F] + 1e-4 * s[GD]
    if f_new > upper:
        s[BACKTRACKS] += 1.0
        s[TT] = s[TT] * .8
        s[REVERT] = 1.0 if s[STEPINF] < 1e-12 else 0.0
        s[MODE] = BACKTRACK
        return st
    dg = gn - g
    it = s[ITER] + 1.0
    f = s[F]
    s[FOLD], s[F] = f, f_new
    s[DXDG] = dev['DXDG'] if 'DXDG' in dev else dx.T.dot(dg)
    s[DGDG] = dev['DGDG'] if 'DGDG' in dev else dg.T.dot(dg)
    with np.errstate(all='ignore'):
        s[T] = np.float64(s[DXDG]) / np.float64(s[DGDG])
        if C > 0:
            st['lb'][(int(it) - 2) % C] = np.float64(1.0) / np.float64(s[DXDG])
    s[TT], s[REVERT], s[ITER] = 1.0, 0.0, it
    k = int(it) - 1
    if k < P['hist_cap']:
        st['hist'][k] = f_new
    r = stop_reason(it, P['max_iter'], f_new, f, P['opt_tol'], P['prog_tol'], P.get('f_min'))
    s[STOP] = r
    s[MODE] = STOPPED if r else STEP
    return st


def solve_model(A, b, starts, x0, kind, params, limit=20000):
    """The model iterated from INIT to its stop; also the modes it went through."""
    A = sps.csr_matrix(A)
    AT = sps.csr_matrix(A.T)
    st = new_state(x0, params)
    modes = []
    while int(st['scal'][MODE]) != STOPPED:
        modes.append((int(st['scal'][MODE]), st['scal'][REVERT]))
        st = round_model(st, A, AT, b, starts, kind, params)
        assert len(modes) < limit
    return st, modes


# ---- the Armijo boundary -------------------------------------------------------------

def armijo_boundary(f_new, gd):
    """The doubles F with fl(F + fl(1e-4 gd)) == f_new: (below, lo, hi, above),
    [lo, hi] the plateau, below / above its neighbours.  The round rejects iff
    f_new > F + 1e-4 gd: at `below` (f_new is above the line) and nowhere
    from `lo` on.  ValueError where no double lands on f_new."""
    f_new, c = np.float64(f_new), np.float64(1e-4) * np.float64(gd)
    Fv = f_new - c
    for _ in range(128):
        u = Fv + c
        if u == f_new:
            break
        Fv = np.nextafter(Fv, np.inf if u < f_new else -np.inf)
    else:
        raise ValueError('no F with F + 1e-4 gd == f_new')
    lo = hi = Fv
    while np.nextafter(lo, -np.inf) + c == f_new:
        lo = np.nextafter(lo, -np.inf)
    while np.nextafter(hi, np.inf) + c == f_new:
        hi = np.nextafter(hi, np.inf)
    return np.nextafter(lo, -np.inf), lo, hi, np.nextafter(hi, np.inf)


# ---- exact dots in seconds -------------------------------------------------------------

def _split(a):
    c = 134217729.0 * a                      # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def fast_exact_sum(a, b=None):
    """exact_sum for long vectors: every product as an exact pair of doubles
    (Dekker's two-product, no fused multiply-add needed), summed by math.fsum
    -- the correctly rounded sum, as exact_sum's.  Returns an M.ExactSum whose
    `exact` is the rounded reference and whose `sumabs` is an upper bound of
    sum|terms| (so bound() is no tighter than exact_sum's).  Magnitudes must
    stay clear of over- and underflow (|terms| in [1e-100, 1e100])."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    if b is None:
        ref = math.fsum(a.tolist())
        sumabs = math.fsum(np.abs(a).tolist()) * (1.0 + 2.0 ** -50)
        return M.ExactSum(ref, Fraction(ref), Fraction(sumabs), a.size)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    assert a.shape == b.shape
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    ref = math.fsum(p.tolist() + e.tolist())
    sumabs = math.fsum(np.abs(p).tolist()) * (1.0 + 2.0 ** -50)
    return M.ExactSum(ref, Fraction(ref), Fraction(sumabs), a.size)


# ---- problems -------------------------------------------------------------------------

P_SPECIAL = [1, 2, 64, 65, 150]
GRID_NS = (1, 2, 3, 2049, 2050, 16384, 16386, 16387)
STRIDE_N = 2 * (1048576 + 2 * 1024 + 300) + 1


def starts_of(sizes):
    return np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)


def problem_P(odd, m=321, noise=0.02):
    """A scaled incidence with small integer flows (as
    test_gpu_handoffs.make_problem): m links, ~2.7k routes, blocks of 1, 2, 64,
    65, 150 and 2..40; n odd or even as asked.  Returns A, b, sizes."""
    rs = np.random.RandomState(4100 + int(odd))
    sizes = np.concatenate([rs.randint(2, 41, size=115), P_SPECIAL])
    rs.shuffle(sizes)
    if (int(sizes.sum()) % 2 == 1) != bool(odd):
        sizes = np.concatenate([sizes, [1]])
    n = int(sizes.sum())
    pat = sps.random(m, n, density=0.03, random_state=rs, format='csr')
    pat.data[:] = 1.0
    colv = rs.randint(1, 6, size=n).astype(np.float64)
    A = sps.csr_matrix(pat.multiply(colv[None, :]))
    A.sort_indices()
    xv = np.zeros(n)
    xv[starts_of(sizes) + rs.randint(0, sizes)] = 1.0
    b = A.dot(xv) * (1.0 + noise * rs.randn(m))
    return A, b, sizes


def trivial_matrix(n, m=64):
    """m = 64 rows, one or two small integer entries per column."""
    j = np.arange(n, dtype=np.int64)
    r1 = j % m
    two = (j % 2 == 0) & (m > 1)
    r2 = (r1 + 1 + (j // 2) % (m - 1)) % m          # != r1
    rows = np.concatenate([r1, r2[two]])
    cols = np.concatenate([j, j[two]])
    vals = np.concatenate([1.0 + (j % 3), 1.0 + (j[two] % 2)])
    A = sps.csr_matrix((vals, (rows, cols)), shape=(m, n))
    A.sort_indices()
    return A


def grid_sizes(n):
    """Blocks of 1 .. 97 entries that fill n."""
    sizes, k = [], 0
    while sum(sizes) < n:
        sizes.append(min(1 + (37 * k) % 97, n - sum(sizes)))
        k += 1
    return np.array(sizes, dtype=np.int64)


def grid_problem(n):
    rs = np.random.RandomState(n % 100003)
    A = trivial_matrix(n)
    if n < 10 ** 5:
        sizes = grid_sizes(n)
    else:                                            # blocks of 100, the rest in one
        k = n // 100
        sizes = np.concatenate([np.full(k, 100), [n - 100 * k] if n % 100 else []]).astype(np.int64)
    b = np.round(rs.uniform(-4.0, 4.0, size=A.shape[0]) * 8.0) / 8.0
    return A, b, sizes


def dyadic(rs, n, lo, hi, den):
    """n multiples of 1/den in [lo, hi], none zero."""
    v = rs.randint(int(lo * den), int(hi * den) + 1, size=n).astype(np.float64)
    v[v == 0.0] = 1.0
    return v / den


def int_dot(a, b, den_a, den_b):
    """sum a_j b_j for a, b multiples of 1/den_a, 1/den_b, in integers:
    (the integer, its denominator).  Asserts sum |a_j b_j| < 2^53 in units of
    the common denominator: every partial sum, in whatever order and grouping,
    is then an integer below 2^53 in those units, hence an exact double."""
    ia = np.round(np.asarray(a) * den_a).astype(np.int64)
    ib = np.round(np.asarray(b) * den_b).astype(np.int64)
    assert np.array_equal(ia / den_a, a) and np.array_equal(ib / den_b, b)
    assert np.max(np.abs(ia), initial=0) < 2 ** 26 and np.max(np.abs(ib), initial=0) < 2 ** 26
    terms = ia * ib                                  # |terms| < 2^52 each
    assert math.fsum(np.abs(terms).astype(np.float64).tolist()) < 2.0 ** 53
    tot = int(np.sum(terms, dtype=np.int64))
    return tot, den_a * den_b


def dyadic_bb_case(n, seed=77):
    """The BACKTRACK round (tt = 1/2) of the grid-stride problem on a dyadic
    grid: trivial_matrix(n), x, g, x_new, and b = A x_new' - r with a planted
    r, where x_new' = x/2 + x_new/2.  Every product and every partial sum of
    ||r||^2, g.dx, dx.dg, dg.dg is an integer multiple of 2^-6 below 2^53, so
    each sum is exact in any order.  Returns the vectors and the exact values
    (formed in integers)."""
    rs = np.random.RandomState(seed)
    A = trivial_matrix(n)
    AT = sps.csr_matrix(A.T)
    x = dyadic(rs, n, 0.125, 1.0, 8)
    dxp = dyadic(rs, n, -2.0, 2.0, 4)
    xn = x + dxp
    g = dyadic(rs, n, -4.0, 4.0, 8)
    r = dyadic(rs, A.shape[0], -4.0, 4.0, 8)
    xa = 0.5 * x + 0.5 * xn
    dx = xa - x
    assert np.array_equal(dx, dxp / 2) and np.array_equal(xa * 16, np.round(xa * 16))
    b = A.dot(xa) - r
    assert np.array_equal(A.dot(xa) - b, r)
    # the two products, in any order: per row sum|a x| + |b| (sixteenths) and
    # sum|a' r| (eighths) stay below 2^53
    assert np.max(abs(A).dot(np.abs(xa)) + np.abs(b)) * 16 < 2.0 ** 53
    assert np.max(abs(AT).dot(np.abs(r))) * 8 < 2.0 ** 53
    gn = AT.dot(r)
    dg = gn - g
    want = {}
    for name, (u, v) in dict(SQ=(r, r), GD=(g, dx), DXDG=(dx, dg), DGDG=(dg, dg)).items():
        tot, den = int_dot(u, v, 8, 8)
        assert abs(tot) < 2 ** 53
        want[name] = tot / den
        assert Fraction(want[name]) == Fraction(tot, den)
    want['STEPINF'] = float(np.max(np.abs(dx)))
    return dict(A=A, b=b, x=x, g=g, xn=xn, xa=xa, r=r, gn=gn, want=want)


def dyadic_lbfgs_case(n, C, it, seed=78):
    """An L-BFGS STEP round on a dyadic grid: x, g, x_new, g_new multiples of
    1/8, so s, y and g.s, g.y, s.y, y.y are exact in any order; the four sums
    (in integers) and the rho ring."""
    rs = np.random.RandomState(seed)
    x = dyadic(rs, n, 0.125, 1.0, 8)
    s = dyadic(rs, n, -1.0, 1.0, 8)
    y = 2.0 * s + dyadic(rs, n, -0.25, 0.25, 8)
    g = dyadic(rs, n, -4.0, 4.0, 8)
    xn, gn = x + s, g + y
    assert np.array_equal(xn - x, s) and np.array_equal(gn - g, y)
    sums = []
    for u, v in ((gn, s), (gn, y), (s, y), (y, y)):
        tot, den = int_dot(u, v, 8, 8)
        assert abs(tot) < 2 ** 53
        sums.append(tot / den)
    assert sums[2] > 0
    rho = planted_ring(C, it) / sums[2]
    return dict(x=x, g=g, xn=xn, gn=gn, sv=s, yv=y, sums=sums, rho=rho)


def planted_vectors(n, seed):
    """x in [0.25, 1], g, and a planted (x_new, g_new) with every term of
    g.dx, dx.dg, dg.dg within 2^-10 of the largest (M.terms_ok) and
    dx.dg > 0."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.25, 1.0, size=n)
    g = M.signed(rs, n)
    dx = M.signed(rs, n, 0.25, 1.0)
    dg = dx * rs.uniform(1.0, 4.0, size=n)
    return dict(x=x, g=g, xn=x + dx, gn=g + dg)


def planted_ring(C, it):
    """A rho ring with a distinct, well-scaled factor in every slot: rho_q =
    c_q / (s.y) with c_q in [0.02, 0.06], so that (1 - c)^C stays above 0.04
    and every slot still weighs in the direction.  Returns the factors."""
    rs = np.random.RandomState(100 * C + int(it))
    return 0.02 + 0.04 * (rs.permutation(C) + 0.5) / C


def lbfgs_case(n, C, it, seed):
    """Planted x, g, xn, gn with y.s > 0 and the rho ring of an L-BFGS STEP
    round at iteration `it`."""
    rs = np.random.RandomState(seed)
    x = rs.uniform(0.0, 1.0, size=n)
    g = M.signed(rs, n)
    s = M.signed(rs, n, 0.01, 0.1)
    y = s * rs.uniform(1.0, 3.0, size=n) * (1.0 + 0.05 * rs.randn(n))     # y_j s_j > 0
    xn, gn = x + s, g + y
    sv, yv = xn - x, gn - g
    assert sv.dot(yv) > 0
    rho = planted_ring(C, it) / sv.dot(yv)
    return dict(x=x, g=g, xn=xn, gn=gn, sv=sv, yv=yv, rho=rho)


LBFGS_CS = (1, 3, 50)


def lbfgs_iters(C):
    """The planted ITER of a STEP round: the last BB iteration, the first two
    of the recursion, and a ring not full, just full and wrapped (for small C
    those fall on the BB branch: ITER 2, 3 at C = 1, ITER 4 at C = 3)."""
    return sorted({5, 6, 7, C + 1, C + 2, C + 7})


def swap_pairs(C, it):
    """Two ring slots in use at iteration `it` whose exchange the direction
    must show: the newest and the oldest queued."""
    k = int(it) - 1
    m = min(k, C)
    return (k - 1) % C, (k - m) % C


# ---- the model's own checks ----------------------------------------------------------------

def small_problem(seed, lasso=False):
    rs = np.random.RandomState(seed)
    sizes = np.array([1, 2, 5, 9, 3, 17, 4, 8, 2, 6, 11, 7], dtype=np.int64)
    n, m = int(sizes.sum()), 24
    pat = sps.random(m, n, density=0.25, random_state=rs, format='csr')
    pat.data[:] = 1.0
    colv = rs.randint(1, 6, size=n).astype(np.float64)
    A = sps.csr_matrix(pat.multiply(colv[None, :]))
    xv = np.zeros(n)
    xv[starts_of(sizes) + rs.randint(0, sizes)] = 1.0
    b = A.dot(xv) * (1.0 + 0.05 * rs.randn(m))
    x0 = np.repeat(1.0 / sizes, sizes)
    if lasso:
        x0 = x0 * rs.choice([-1.0, 1.0], size=n)
    return A, b, sizes, x0


class CountingLA:
    """numpy.linalg with its norm calls counted: line_search (oracle.py) calls
    la.norm once per backtrack, and reverts where it is below 1e-12."""

    def __init__(self, la):
        self._la, self.norms, self.reverts = la, 0, 0

    def norm(self, *a, **k):
        v = self._la.norm(*a, **k)
        self.norms += 1
        self.reverts += int(v < 1e-12)
        return v

    def __getattr__(self, name):
        return getattr(self._la, name)


# solver, corrections, lasso, seed of small_problem, prog_tol.  BB reaches
# |f_old - f| < 1e-12 long before a step is rejected for good; with
# prog_tol = 1e-300 only an exact repeat of f stops it, and on these seeds that
# is the revert's.  C = 50: the ring never fills (24 iterations).
REPLAYS = [('bb', 0, False, 18, 1e-300), ('bb', 0, True, 4, 1e-300),
           ('lbfgs', 3, False, 3, 1e-12), ('lbfgs', 1, False, 3, 1e-12),
           ('lbfgs', 10, False, 3, 1e-12), ('lbfgs', 50, False, 3, 1e-12),
           ('lbfgs', 3, True, 0, 1e-12)]


@pytest.mark.parametrize('solver,C,lasso,seed,prog_tol', REPLAYS)
def test_model_replays_the_oracle(orc, monkeypatch, solver, C, lasso, seed, prog_tol):
    A, b, sizes, x0 = small_problem(seed, lasso)
    starts = starts_of(sizes)
    kind = 'ball' if lasso else 'simplex'
    la = CountingLA(orc.la)
    monkeypatch.setattr(orc, 'la', la)
    obj, proj, ls = orc.sparse_parts(A, b, starts, lasso=lasso)
    with np.errstate(all='ignore'):
        if solver == 'bb':
            ref = orc.batch_solve_bb(obj, proj, ls, x0.copy(), max_iter=2000, prog_tol=prog_tol)
        else:
            ref = orc.batch_solve_lbfgs(obj, proj, ls, x0.copy(), max_iter=2000, prog_tol=prog_tol,
                                        corrections=C)
    params = dict(max_iter=2000, opt_tol=1e-6, prog_tol=prog_tol, f_min=None, hist_cap=2001, C=C)
    st, modes = solve_model(A, b, starts, x0, kind, params)
    s = st['scal']
    it = int(s[ITER])
    print('%s C=%d %s: %d iterations, %d backtracks, %d reverts, stop %r'
          % (solver, C, kind, it, la.norms, la.reverts, ref['stop']))
    # the run has what the replay is for
    assert la.norms >= 2 and la.reverts == 1 and ref['stop'].endswith('< prog_tol')
    assert (BACKTRACK, 0.0) in modes and modes[-1] == (BACKTRACK, 1.0)
    if solver == 'lbfgs':
        assert it > 7 and (it > C + 2) == (C <= 10)      # the recursion ran; the ring wrapped
    assert it == ref['iterations']
    assert same_bits(st['xn'], ref['x']) and same_bits(s[F], ref['f'])
    assert stop_string(int(s[STOP]), s[F], s[FOLD], None) == ref['stop']
    assert same_bits(st['hist'][:it], ref['progress'])
    assert int(s[BACKTRACKS]) == la.norms
    assert int(s[ROUNDS]) == len(modes) == it + la.norms
    # the revert round got f and g back and accepted with a zero step
    assert s[F] == s[FOLD] and s[GD] == 0.0 and s[DXDG] == 0.0 and math.isnan(s[T])
    assert same_bits(st['gn'], st['g']) and same_bits(st['xn'], st['x'])


def test_model_max_iter_and_init_stops(orc):
    """max_iter runs (no revert on the way), the INIT stops, max_iter = 0."""
    A, b, sizes, x0 = small_problem(3)
    starts = starts_of(sizes)
    obj, proj, ls = orc.sparse_parts(A, b, starts)
    for k in (1, 2, 7):
        ref = orc.batch_solve_bb(obj, proj, ls, x0.copy(), max_iter=k)
        params = dict(max_iter=k, opt_tol=1e-6, prog_tol=1e-12, f_min=None, hist_cap=k + 1)
        st, modes = solve_model(A, b, starts, x0, 'simplex', params)
        s = st['scal']
        assert ref['stop'] == 'max_iter' and int(s[STOP]) == MAXITER and int(s[ITER]) == k
        assert same_bits(st['xn'], ref['x']) and same_bits(st['hist'][:k], ref['progress'])
        if k == 1:
            assert modes == [(INIT, 0.0)] and s[FOLD] == np.inf and st['hist'][0] == s[F]
    f0 = obj(x0, np.zeros(x0.size))
    ref = orc.batch_solve_bb(obj, proj, ls, x0.copy(), f_min=f0 + 1.0, max_iter=1)
    params = dict(max_iter=1, opt_tol=1e-6, prog_tol=1e-12, f_min=f0 + 1.0, hist_cap=2)
    st, modes = solve_model(A, b, starts, x0, 'simplex', params)
    assert 'opt_tol' in ref['stop'] and int(st['scal'][STOP]) == OPT and len(modes) == 1
    assert stop_string(OPT, st['scal'][F], np.inf, f0 + 1.0) == ref['stop']
    # max_iter = 0 never matches: the run goes on to the revert
    params = dict(max_iter=0, opt_tol=1e-6, prog_tol=1e-12, f_min=None, hist_cap=4)
    st, modes = solve_model(A, b, starts, x0, 'simplex', params)
    assert int(st['scal'][STOP]) == PROG and st['scal'][ITER] > 4


STOP_ROWS = [
    # name, it after the accept, max_iter, f_new, f, f_min, opt_tol, prog_tol, reason
    ('none', 5, 9, 10.0, 11.0, 1.0, 1e-6, 1e-12, 0),
    ('maxiter', 9, 9, 10.0, 11.0, 1.0, 1e-6, 1e-12, MAXITER),
    ('opt', 5, 9, 10.0, 11.0, 10.0, 1e-6, 1e-12, OPT),
    ('prog', 5, 9, 10.0, 10.0, 1.0, 1e-6, 1e-12, PROG),
    ('maxiter+opt', 9, 9, 10.0, 11.0, 10.0, 1e-6, 1e-12, OPT),
    ('maxiter+prog', 9, 9, 10.0, 10.0, 1.0, 1e-6, 1e-12, PROG),
    ('opt+prog', 5, 9, 10.0, 10.0, 10.0, 1e-6, 1e-12, PROG),
    ('all', 9, 9, 10.0, 10.0, 10.0, 1e-6, 1e-12, PROG),
    ('no-fmin', 5, 9, 10.0, 11.0, None, 1e-6, 1e-12, 0),
    ('opt-strict', 5, 9, 10.0, 11.0, 9.0, 1.0, 1e-12, 0),       # f - f_min == opt_tol: no stop
    ('prog-strict', 5, 9, 10.0, 11.0, 1.0, 1e-6, 1.0, 0),        # |f_old - f| == prog_tol
    ('maxiter-0', 5, 0, 10.0, 11.0, 1.0, 1e-6, 1e-12, 0),
    ('nan-f', 5, 9, float('nan'), 11.0, 1.0, 1e-6, 1e-12, 0),
]


def test_stop_table_against_the_oracle(orc):
    codes = {'continue': 0, 'max_iter': MAXITER}
    for name, it, mi, fn, f, fmin, ot, pt, want in STOP_ROWS:
        flag, stop = orc.batch_stopping(it, mi, fn, f, ot, pt, fmin)
        code = codes.get(stop, OPT if 'opt_tol' in stop else PROG)
        assert stop_reason(float(it), mi, fn, f, ot, pt, fmin) == code == want, name
        assert flag == bool(want)
        if want:
            assert stop_string(want, fn, f, fmin) == stop
    # first-match-wins (the reasons tested in the opposite order) gets the combined rows wrong
    first = {r[0] for r in STOP_ROWS
             if (MAXITER if r[1] == r[2] else OPT if r[5] is not None and r[3] - r[5] < r[6]
                 else PROG if abs(r[4] - r[3]) < r[7] else 0) != r[8]}
    assert first == {'maxiter+opt', 'maxiter+prog', 'opt+prog', 'all'}


def test_armijo_boundary_helper():
    rs = np.random.RandomState(5)
    for _ in range(200):
        f_new = np.float64(rs.uniform(1.0, 1000.0))
        gd = np.float64(-rs.uniform(1e-3, 50.0))
        below, lo, hi, above = armijo_boundary(f_new, gd)
        c = np.float64(1e-4) * gd
        assert below < lo <= hi < above
        assert lo + c == f_new and hi + c == f_new
        assert below + c < f_new < above + c
        assert np.nextafter(below, np.inf) == lo and np.nextafter(hi, np.inf) == above
        # reject iff f_new > upper: only below the plateau
        assert [bool(f_new > Fv + c) for Fv in (below, lo, hi, above)] == [True, False, False, False]
        # `>=` for `>` differs exactly on the plateau
        assert [bool(f_new >= Fv + c) for Fv in (below, lo, hi, above)] == [True, True, True, False]
    # gd = 0 (the revert round): the plateau is f_new itself
    assert armijo_boundary(3.5, 0.0) == (np.nextafter(3.5, -np.inf), 3.5, 3.5,
                                         np.nextafter(3.5, np.inf))
    with pytest.raises(ValueError):
        armijo_boundary(1.0, -1e4 * (1.0 + 2.0 ** -52) * 2.0 ** 60)


def test_fast_exact_sum_is_exact_sum():
    rs = np.random.RandomState(9)
    for n in (1, 2, 777, 3001):
        a, b = M.signed(rs, n) * 10.0 ** rs.randint(-3, 4, size=n), M.signed(rs, n)
        es, fs = exact_sum(a, b), fast_exact_sum(a, b)
        assert same_bits(es.ref, fs.ref) and fs.k == es.k
        assert es.sumabs <= fs.sumabs <= es.sumabs * (1 + Fraction(1, 2 ** 40))
        e1, f1 = exact_sum(a), fast_exact_sum(a)
        assert same_bits(e1.ref, f1.ref)
        assert e1.sumabs <= f1.sumabs <= e1.sumabs * (1 + Fraction(1, 2 ** 40))
    # a sum that cancels to its last bits
    a = np.array([1e16, 1.0, -1e16, 1e-3])
    b = np.array([1.0 + 2.0 ** -30, 1.0, 1.0 + 2.0 ** -30, 3.0])
    assert same_bits(exact_sum(a, b).ref, fast_exact_sum(a, b).ref)


def test_lbfgs_direction_model(orc):
    """The vector recursion, the coefficient recursion and the reference's
    deque form agree; the planted cases are well conditioned (double against
    long double within 1e-12 ||d||_inf) and show a wrong ring slot (two slots
    exchanged: more than 1e-8 ||d||_inf)."""
    from collections import deque
    n = 2701
    worst = 0.0
    for C in LBFGS_CS:
        for it in lbfgs_iters(C):
            if it <= 5:
                continue
            pl = lbfgs_case(n, C, it, seed=7 * C + it)
            lb = np.zeros(2 * C + 8)
            lb[:C] = pl['rho']
            assert len(set(lb[:C].tolist())) == C and np.all(lb[:C] > 0)
            rhos = ring_rhos(lb, it, C)
            assert len(rhos) == min(it - 1, C)
            g, s, y = pl['gn'], pl['sv'], pl['yv']       # after the step g is g_new
            d = lbfgs_direction(g, s, y, rhos)
            # the reference's own helper form, on deques (oracle.py:609-619)
            q_dg, q_dx, q_rho = deque([y] * len(rhos)), deque([s] * len(rhos)), deque(rhos)
            dd, alpha, m = g.copy(), np.zeros(C), len(rhos)
            for j in range(1, m + 1):
                alpha[-j] = q_rho[-j] * q_dx[-j].T.dot(dd)
                dd -= alpha[-j] * q_dg[-j]
            dd *= q_dx[-1].T.dot(q_dg[-1]) / q_dg[-1].T.dot(q_dg[-1])
            for j in range(m):
                beta = q_rho[j] * q_dg[j].T.dot(dd)
                dd += q_dx[j] * (alpha[-m + j] - beta)
            dd *= -1.0
            assert same_bits(d, dd)
            dl = lbfgs_direction(g, s, y, rhos, dtype=LD)
            scale = float(np.max(np.abs(dl)))
            dev = float(np.max(np.abs(d.astype(LD) - dl))) / scale
            worst = max(worst, dev)
            assert dev <= 1e-12, (C, it, dev)
            coef, _ = lbfgs_coefficients(g.dot(s), g.dot(y), s.dot(y), y.dot(y), lb, it, C)
            dc = direction_from_coefficients(coef, g, s, y)
            assert float(np.max(np.abs(dc.astype(LD) - dl))) / scale <= 1e-12, (C, it)
            if C > 1:
                p, q = swap_pairs(C, it)
                assert p != q
                lb2 = lb.copy()
                lb2[p], lb2[q] = lb[q], lb[p]
                d2 = lbfgs_direction(g, s, y, ring_rhos(lb2, it, C), dtype=LD)
                assert float(np.max(np.abs(d2 - dl))) / scale > 1e-8, (C, it)
            # the ring read one slot off (every slot planted: unwritten ones too)
            k = it - 1
            off = [lb[(k - m + j + 1) % C] for j in range(m)]
            if C > 1:
                d3 = lbfgs_direction(g, s, y, off, dtype=LD)
                assert float(np.max(np.abs(d3 - dl))) / scale > 1e-8, (C, it)
    print('double against long double, worst: %.3g of ||d||_inf' % worst)


def test_problems_reach_the_edges():
    for odd in (True, False):
        A, b, sizes = problem_P(odd)
        n = int(sizes.sum())
        assert A.shape == (321, n) and (n % 2 == 1) == odd and 2500 < n < 3000
        assert set(P_SPECIAL) <= set(sizes.tolist())
        assert np.all(np.isin(A.data, [1.0, 2.0, 3.0, 4.0, 5.0]))
        assert step_grid(n) > 9 and finish_grid(n) in (2, 3)
    want = {1: 1, 2: 1, 3: 1, 2049: 1, 2050: 2, 16384: 8, 16386: 9, 16387: 9}
    assert {n: finish_grid(n) for n in GRID_NS} == want
    assert {step_grid(n) for n in GRID_NS} >= {1, 9, 64, 65}
    for n in GRID_NS:
        A, b, sizes = grid_problem(n)
        assert A.shape == (64, n) and int(sizes.sum()) == n and sizes.min() >= 1
        per_col = np.diff(A.tocsc().indptr)
        assert per_col.min() >= 1 and per_col.max() <= 2
        assert np.all(A.data == np.round(A.data)) and A.data.min() >= 1
    # the grid-stride problem: both grids capped, the finish grid's second pass
    # partly filled (with clamped loads), an odd tail
    n = STRIDE_N
    n2 = n >> 1
    assert n % 2 == 1 and n > 2 * 1024 * 1024 and step_grid(n) == finish_grid(n) == XGRID
    stride = XGRID * XT * XU
    left = n2 - stride
    assert 0 < left < stride and left == 2 * 1024 + 300
    assert left % XT != 0                           # a step where p >= n2 for some u only


def test_dyadic_cases_are_exact():
    """The dyadic cases at a small n: NumPy's dots (another order than any
    kernel's) give the integer values bit for bit."""
    n = 16387
    c = dyadic_bb_case(n)
    dx, dg = c['xa'] - c['x'], c['gn'] - c['g']
    got = dict(SQ=c['r'].dot(c['r']), GD=c['g'].dot(dx), DXDG=dx.dot(dg), DGDG=dg.dot(dg),
               STEPINF=np.max(np.abs(dx)))
    for k, v in c['want'].items():
        assert same_bits(got[k], v), k
        assert same_bits(math.fsum((np.flip(dx) * np.flip(dg)).tolist()), c['want']['DXDG'])
    L = dyadic_lbfgs_case(n, 3, 7)
    s, y, g = L['sv'], L['yv'], L['gn']
    assert [g.dot(s), g.dot(y), s.dot(y), y.dot(y)] == L['sums']
    lb = np.zeros(14)
    lb[:3] = L['rho']
    coef, alpha = lbfgs_coefficients(*L['sums'], lb, 7, 3)
    d = direction_from_coefficients(coef, g, s, y)
    dl = lbfgs_direction(g, s, y, ring_rhos(lb, 7, 3), dtype=LD)
    assert float(np.max(np.abs(d - dl)) / np.max(np.abs(dl))) <= 1e-12
    assert sorted(alpha) == [0, 1, 2]


def test_planted_vectors_meet_the_term_size_conditions():
    for n in (2701, 3):
        pl = planted_vectors(n, seed=n)
        dx, dg = pl['xn'] - pl['x'], pl['gn'] - pl['g']
        assert terms_ok(pl['g'] * dx) and terms_ok(dx * dg) and terms_ok(dg * dg)
        assert dx.dot(dg) > 0
        es = exact_sum(pl['g'], dx)
        j = int(np.argmin(np.abs(pl['g'] * dx)))
        assert within(es.ref, es) and not within(es.ref - pl['g'][j] * dx[j], es)
        assert Fraction(float(abs(pl['g'][j] * dx[j]))) > 10 ** 6 * bound(es)
