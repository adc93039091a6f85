"""A column shard's partial residual on one GPU (csrc/bb.hip): bsls_bb_stage 1
and 14, bsls_bb_residual_rows and bsls_bb_k1_rows with shard_role 1 (r = A x +
target) and 2 (r = A x), at iteration 0 (no stop test) and inside an iteration
-- the K1 launches without the ||r||^2 reduction, which the single-GPU suites
reach only with shard_role 0.

The problem is test_gpu_handoffs.make_problem's (m = 321: the last row block
of the tiles is one row; m = 320: bb_k1_sum's 16-B pairs; ~2.7k routes).
Engines: the panels (one row block of 16 x 64 rows at these m, so the row
ranges below are cut to it); the thread-stream tiles and the dealt tiles in
four column groups with the default k1_atomic = 0 (on roles 1 / 2 every group
adds into r by atomics, and stages 15 / 14 fold r's initialisation into K3);
the dealt tiles with k1_atomic = 1 (partials + bb_k1_sum); the dealt tiles in
one group (the finish inside bb_k1t).

x and a sentinel r = -7 are planted, one call runs, and r is compared row by
row with M x_dev (+ target on role 1) from SciPy, x_dev the x on the device
(it carries colv, so M is A's 0/1 pattern for a scaled incidence), within
2 (n + 4) 2^-53 (|M| |x_dev| + |target|): each of the two sums of <= n + 1
terms rounds within (n + 4) u of its sum of magnitudes
(test_gpu_bb_scalars.test_k1_finish's bound for the same sum).  Rows outside
a row range keep the sentinel, and scal[] what was planted, bit for bit.
Needs an MI355X.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import test_bb_scalars_model as M
from test_gpu_handoffs import K1_PLAN, K2_PLAN, make_problem

pytestmark = pytest.mark.gpu

KINDS = {'panels': dict(fmt='panels'),
         'det': dict(deterministic=True, fmt='tiles', tile_plans=(K1_PLAN, K2_PLAN)),
         'dealt-sum': dict(tile_plans=(K1_PLAN, K2_PLAN)),
         'dealt-atomic': dict(tile_plans=(K1_PLAN, K2_PLAN)),
         'dealt-g1': dict(tile_plans=((64, 1, 0), K2_PLAN))}
MS = [321, 320]
OPTS = {'max_iter': 10 ** 6, 'opt_tol': 1e-30}
SENTINEL = -7.0
S_STOP, S_COUNT = 0, 16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Rig:
    def __init__(self, kind, m):
        import _native
        from device import BBEngine
        assert (_native.S_STOP, _native.S_COUNT) == (S_STOP, S_COUNT)
        self.kind, self.m = kind, m
        self.A, self.b, self.sizes = make_problem(m, seed=31 + m)
        self.pl = M.planted(self.A, self.sizes, seed=1000 + m)
        self.eng = eng = BBEngine(self.A, self.b, self.sizes, options=OPTS, **KINDS[kind])
        self.n, self.nz = eng.n, eng.nz
        assert eng.scaled and eng.P.k1_atomic == 0 and eng.P.r_fx == 0.0
        if kind == 'panels':
            assert eng.fmt_A == 'panels'
            groups = eng.A_pan.img['ngroups']
        else:
            assert eng.fmt_A == 'tiles'
            groups = eng.A_til.img['ngroups']
            assert groups == (1 if kind == 'dealt-g1' else K1_PLAN[1])
            assert eng.A_til.img['layout'] == (0 if kind == 'det' else 2)
        if kind == 'dealt-sum':
            eng.P.k1_atomic = 1
        # bb.hip k1_init_folded: tiles in several groups whose sums go by atomics
        self.folded = kind != 'panels' and groups > 1 and eng.P.k1_atomic == 0
        assert self.folded == (kind in ('det', 'dealt-atomic'))
        self.nrb, self.H = eng.row_blocks()
        assert self.nrb == (1 if kind == 'panels' else -(-m // 64))
        # the matrix x_dev is multiplied by: x_dev = colv * x already
        pat = sps.csr_matrix(self.A, copy=True)
        pat.data[:] = 1.0
        self.Mx = pat
        self.absM = abs(pat)
        self.target = eng.target.cpu().numpy().copy()
        x = self.pl['x']
        self.xg = eng.colv.cpu().numpy() * x

    def put(self, t, a):
        import torch
        a = np.ascontiguousarray(a, dtype=np.float64)
        t[:a.size].copy_(torch.from_numpy(a))

    def get(self, t, count=None):
        return t[:count if count is not None else t.numel()].cpu().numpy().copy()

    def sentinels(self, stop=0.0):
        s = 1000.25 + np.arange(S_COUNT, dtype=np.float64)
        s[S_STOP] = stop
        return s

    def ranges(self):
        """(0, 2) and (2, nrb), cut to the row blocks the engine has"""
        out = [(0, min(2, self.nrb))]
        if self.nrb > 2:
            out.append((2, self.nrb))
        return out

    def rows(self, rb0, rb1):
        return rb0 * self.H, min(rb1 * self.H, self.m)

    def plant(self, stop=0.0):
        self.put(self.eng.x, self.xg)
        self.eng.r.fill_(SENTINEL)
        s0 = self.sentinels(stop)
        self.put(self.eng.scal, s0)
        return s0

    def want(self, role):
        """(expected r, per-row bound) from the x now on the device"""
        xd = self.get(self.eng.x)
        tg = self.target if role == 1 else np.zeros(self.m)
        want = self.Mx.dot(xd) + tg
        tol = 2 * (self.n + 4) * 2.0 ** -53 * (self.absM.dot(np.abs(xd)) + np.abs(tg))
        return want, tol

    def check_rows(self, role, lo, hi, outside, what):
        """rows [lo, hi) of r against the expectation, the others against
        `outside` (an array) bit for bit"""
        r = self.get(self.eng.r)
        want, tol = self.want(role)
        err = np.abs(r[lo:hi] - want[lo:hi])
        print('%s m%d %s rows [%d, %d): max err %.3g, max err / bound %.3g'
              % (self.kind, self.m, what, lo, hi, float(err.max()), float(np.max(err / tol[lo:hi]))))
        assert np.all(err <= tol[lo:hi]), (self.kind, what, float(err.max()))
        assert same_bits(r[:lo], outside[:lo]) and same_bits(r[hi:], outside[hi:]), (self.kind, what)


@pytest.fixture(scope='module')
def rigs(cuda):
    cache = {}

    def get(kind, m):
        if (kind, m) not in cache:
            cache[kind, m] = Rig(kind, m)
        return cache[kind, m]
    yield get
    cache.clear()


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', list(KINDS))
def test_partial_residual(rigs, kind, m):
    """Stage 1, residual_rows over (0, 2) and (2, nrb), k1_rows (inside an
    iteration; on the engines that fold r's initialisation only after stage
    15, below): r = M x_dev (+ target on role 1) on the rows of the range, the
    sentinel outside, scal untouched."""
    rig = rigs(kind, m)
    eng = rig.eng
    keep = np.full(rig.m, SENTINEL)
    for role in (1, 2):
        eng.set_shard_role(role)
        try:
            for it in (0, 3):
                s0 = rig.plant()
                eng.stage(1, it)
                rig.check_rows(role, 0, rig.m, keep, 'role %d stage 1 it %d' % (role, it))
                assert same_bits(rig.get(eng.scal), s0)
                calls = [('residual_rows', eng.residual_rows)]
                if it > 0 and not rig.folded:
                    calls.append(('k1_rows', eng.k1_rows))
                for name, call in calls:
                    for rb0, rb1 in rig.ranges():
                        s0 = rig.plant()
                        call(it, rb0, rb1)
                        lo, hi = rig.rows(rb0, rb1)
                        rig.check_rows(role, lo, hi, keep,
                                       'role %d %s it %d' % (role, name, it))
                        assert same_bits(rig.get(eng.scal), s0)
        finally:
            eng.P.shard_role = 0


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', ['det', 'dealt-atomic'])
def test_folded_init(rigs, kind, m):
    """Stage 15 (K3 of iteration 3 on a planted z and g, with r's
    initialisation folded in), then stage 14 or k1_rows of the same iteration:
    after stage 15 r is target (role 1) or +0.0 (role 2) bit for bit; the K1
    adds M x_dev to it, x_dev the x stage 15 left on the device."""
    rig = rigs(kind, m)
    eng, pl = rig.eng, rig.pl
    assert rig.folded
    it = 3
    filler = np.full(rig.n, 0.5)
    for role in (1, 2):
        init = rig.target if role == 1 else np.zeros(rig.m)

        def stage15():
            rig.put(eng.z[(it - 1) & 1], pl['z'])
            eng.z[it & 1].fill_(0.5)
            rig.put(eng.g[it & 1], pl['g_step'])
            rig.put(eng.x, filler)
            eng.r.fill_(SENTINEL)
            rig.put(eng.scal, rig.sentinels())
            eng.stage(15, it)
            assert rig.get(eng.scal)[S_STOP] == 0.0
            assert not same_bits(rig.get(eng.x), filler)          # K3 wrote x
            assert same_bits(rig.get(eng.r), init)

        eng.set_shard_role(role)
        try:
            stage15()
            eng.stage(14, it)
            rig.check_rows(role, 0, rig.m, init, 'role %d stage 15 + 14' % role)
            stage15()
            done = 0
            for rb0, rb1 in rig.ranges():
                eng.k1_rows(it, rb0, rb1)
                lo, hi = rig.rows(rb0, rb1)
                assert lo == done
                done = hi
                # the rows of the ranges so far; the rest still as stage 15 left them
                rig.check_rows(role, 0, hi, init, 'role %d stage 15 + k1_rows' % role)
            assert done == rig.m
        finally:
            eng.P.shard_role = 0


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', list(KINDS))
def test_stopped_run(rigs, kind, m):
    """A planted STOP inside an iteration (it = 3): on role 2 the rows of the
    range become +0.0 bit for bit (the all-reduce then leaves role 1's final
    residual) and the rest stays; on role 1 all of r stays.  At it = 0 a
    planted STOP is ignored."""
    rig = rigs(kind, m)
    eng = rig.eng
    keep = np.full(rig.m, SENTINEL)
    stop = float(M.STOP_MAXITER)
    calls = [('stage 1', lambda it, rb0, rb1: eng.stage(1, it), [(0, rig.nrb)]),
             ('residual_rows', eng.residual_rows, rig.ranges())]
    if not rig.folded:
        calls.append(('k1_rows', eng.k1_rows, rig.ranges()))
    for role in (1, 2):
        eng.set_shard_role(role)
        try:
            for name, call, ranges in calls:
                for rb0, rb1 in ranges:
                    s0 = rig.plant(stop)
                    call(3, rb0, rb1)
                    lo, hi = rig.rows(rb0, rb1)
                    want = keep.copy()
                    if role == 2:
                        want[lo:hi] = 0.0
                    assert same_bits(rig.get(eng.r), want), (kind, role, name, rb0, rb1)
                    assert same_bits(rig.get(eng.scal), s0)
            for name, call, ranges in calls[:2]:
                for rb0, rb1 in ranges:
                    s0 = rig.plant(stop)
                    call(0, rb0, rb1)
                    lo, hi = rig.rows(rb0, rb1)
                    rig.check_rows(role, lo, hi, keep, 'role %d %s it 0, STOP planted' % (role, name))
                    assert same_bits(rig.get(eng.scal), s0)
        finally:
            eng.P.shard_role = 0
