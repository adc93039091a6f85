"""The sixteen doubles of the BB engine's scal[] (csrc/bb.hip), slot by slot:
the four BB sums of K2's epilogue, RR and FX of the K1 finish, the slices of
||r||^2 that stages 8 and 10 sum, t and the WARN count of bb_step_t, the stop
reason of bb_stop_reason, and PSUMDG..PGG with their restoration on a stop.

State is planted, not evolved, so every scalar has one known cause: g_prev, dz
and r are written, the other scal slots hold sentinels, one stage runs, and
each slot is compared with its reference -- the sums with the exact rational
sum rounded once, within (k + 4) u sum|terms| (tests/test_bb_scalars_model.py,
where the model, the term-size conditions and the tables are checked on the
CPU); FX, T, ITER, ZBUF, STOP, WARN, the copied P* slots and every untouched
sentinel bit for bit.  dg_j is the double g_new_j - g_prev_j of the g_new the
device stored (g itself: test_gpu_bb.py, test_gpu_fixed_sums.py).

The problem is test_gpu_handoffs.make_problem's (m = 321 and 320, ~2.7k routes,
blocks of 2 .. 150, an odd n_z, empty and one-step tiles).  Engine kinds: the
panels (the builder takes the problem's dense 64 x 600 patch as it is), the
thread-stream tiles, the dealt tiles (scaled and with stored values), the dealt
K2 in two column groups (wpart / rrp hand-off, last_of_sum by row block), the
fixed-point sums (single-GCD stages 3, 4, 7, 9 only) and a link-part engine of
three parts (bsls_bb_k2_part), one rank, no process group.  The sharded stages
run with shard_role 1 on the whole problem: a one-rank shard.  Needs an MI355X.
"""
import math

import numpy as np
import pytest

import test_bb_scalars_model as M
from test_gpu_handoffs import K1_PLAN, K2_PLAN, make_problem

pytestmark = pytest.mark.gpu

KINDS = {'panels': dict(fmt='panels'),
         'det': dict(deterministic=True, fmt='tiles', tile_plans=(K1_PLAN, K2_PLAN)),
         'dealt': dict(tile_plans=(K1_PLAN, K2_PLAN)),
         'dealt-general': dict(general=True, tile_plans=(K1_PLAN, K2_PLAN)),
         'dealt-k2g2': dict(tile_plans=(K1_PLAN, (512, 2, 0))),
         'fixed': dict(fixed_sums=True, tile_plans=(K1_PLAN, K2_PLAN)),
         'parts': dict(fmt='tiles', link_parts=3, tile_plans=(K1_PLAN, (512, 3, 0)))}
ALL = list(KINDS)
SHARDED = [k for k in ALL if k != 'fixed']
SLICED = ['panels', 'dealt', 'dealt-k2g2', 'parts']
MS = [321, 320]
OPTS = {'max_iter': 10 ** 6, 'opt_tol': 1e-30}

S_STOP, S_ITER, S_ZBUF, S_T, S_FX, S_SUMDG, S_DZDG, S_DGDG, S_GG, S_RR, S_WARN = range(11)
S_PSUMDG, S_PDGDG, S_PGG, S_COUNT = 11, 13, 14, 16
SUMS = [S_SUMDG, S_DZDG, S_DGDG, S_GG]
PSUMS = [S_PSUMDG + q for q in range(4)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def unchanged(s0, s1, written):
    """Every slot outside `written` holds what was planted, bit for bit."""
    keep = [q for q in range(S_COUNT) if q not in written]
    assert same_bits(s0[keep], s1[keep]), (keep, s0, s1)


class Rig:
    """An engine, its problem and the planting / reading helpers."""

    def __init__(self, kind, m):
        import torch
        import _native
        from device import BBEngine
        assert (_native.S_SUMDG, _native.S_RR, _native.S_WARN, _native.S_PSUMDG,
                _native.S_COUNT) == (S_SUMDG, S_RR, S_WARN, S_PSUMDG, S_COUNT)
        self.kind, self.m = kind, m
        self.A, self.b, self.sizes = make_problem(m, seed=31 + m)
        self.pl = M.planted(self.A, self.sizes, seed=1000 + m)
        kw = dict(KINDS[kind])
        if kind == 'parts':
            x0 = np.zeros(self.A.shape[1])
            x0[np.cumsum(self.sizes) - 1] = 1.0
            kw['target'] = torch.from_numpy(self.A.dot(x0) - self.b).cuda()
        self.eng = eng = BBEngine(self.A, None if kind == 'parts' else self.b, self.sizes,
                                  options=OPTS, **kw)
        self.nz, self.n = eng.nz, eng.n
        off = _native.load().bsls_bb_dz_offset(eng.m, eng.n, eng.nz)
        self.dz = eng.work[off:off + 8 * eng.nz].view(torch.float64)
        self.target = eng.target.cpu().numpy().copy()
        self.absAT = abs(self.A.T.tocsr())
        if kind == 'panels':
            assert eng.fmt_A == eng.fmt_AT == 'panels'      # the dense patch was not refused
            self.k2_wgs = -(-eng.AT_pan.img['npanels'] // _native.PANEL_WAVES)
        else:
            assert eng.fmt_A == eng.fmt_AT == 'tiles'
            ti = eng.AT_til.img
            want_g = {'dealt-k2g2': 2, 'parts': 3}.get(kind, 1)
            assert ti['ngroups'] == want_g and eng.A_til.img['ngroups'] == K1_PLAN[1]
            assert ti['layout'] == (0 if kind == 'det' else 2)
            self.k2_wgs = ti['nrb'] * (1 if kind == 'parts' else want_g)
            self.group_col = [int(v) for v in ti['group_col']]
        assert eng.scaled == (kind != 'dealt-general') and eng.fixed_sums == (kind == 'fixed')
        assert eng.P.k1_atomic == 0
        # stage 15 folds the atomic K1's r initialisation (bb.hip k1_init_folded)
        self.folds = eng.A_til is not None

    # -- device <-> host
    def put(self, t, a):
        import torch
        a = np.ascontiguousarray(a, dtype=np.float64)
        t[:a.size].copy_(torch.from_numpy(a))

    def get(self, t, count=None):
        return t[:count if count is not None else t.numel()].cpu().numpy().copy()

    def sentinels(self, **slots):
        """scal with a distinct sentinel in every slot, STOP = 0 (running)."""
        s = 1000.25 + np.arange(S_COUNT, dtype=np.float64)
        s[S_STOP] = 0.0
        for k, v in slots.items():
            s[globals()['S_' + k]] = v
        return s

    def run(self, s0, stage, it):
        self.put(self.eng.scal, s0)
        self.eng.stage(stage, it)
        return self.get(self.eng.scal)

    def role(self, role):
        rig = self

        class _Role:
            def __enter__(self):
                rig.eng.set_shard_role(role)

            def __exit__(self, *exc):
                rig.eng.P.shard_role = 0
        return _Role()

    # -- K2
    def plant_k2(self, it, r):
        """r, dz, g_prev = (host N'A'r) - d in g[(it - 1) & 1], a filler in the
        buffer K2 writes."""
        self.gh = M.host_gradient(self.A, self.sizes, r)
        self.g_prev = self.gh - self.pl['d']
        self.put(self.eng.g[(it - 1) & 1], self.g_prev)
        self.eng.g[it & 1].fill_(3.0)
        self.put(self.dz, self.pl['dz'])
        self.r_in = np.array(r, dtype=np.float64)
        self.eng.load_r(self.r_in)

    def check_k2_sums(self, it, s1):
        """SUMDG, DZDG, DGDG, GG of s1 against the exact sums over the device's
        g_new; the term-size conditions on what was actually summed."""
        gn = self.get(self.eng.g[it & 1], self.nz)
        assert same_bits(self.get(self.eng.g[(it - 1) & 1], self.nz), self.g_prev)
        if self.kind != 'fixed':
            # g_new is N'A'r (not its filler): within the rounding of two row
            # sums of <= m terms, the device's and SciPy's
            w = self.absAT.dot(np.abs(self.r_in))
            i = M.z_rows(self.sizes)
            tol = 2 * (self.m + 4) * 2.0 ** -53 * (w[i] + w[i + 1])
            assert np.all(np.abs(gn - self.gh) <= tol), float(np.max(np.abs(gn - self.gh)))
        dg = gn - self.g_prev
        dz = self.pl['dz']
        assert M.terms_ok(dg) and M.terms_ok(dz * dg) and M.terms_ok(dg * dg)
        assert M.detectable(gn * gn)[0]
        refs = {S_SUMDG: M.exact_sum(dg), S_DZDG: M.exact_sum(dz, dg),
                S_DGDG: M.exact_sum(dg, dg), S_GG: M.exact_sum(gn, gn)}
        for slot, es in refs.items():
            assert es.k == self.nz
            print('%s m%d it%d slot %d: got %.17g ref %.17g err %.3g bound %.3g'
                  % (self.kind, self.m, it, slot, s1[slot], es.ref, float(M.error(s1[slot], es)),
                     float(M.bound(es))))
            assert M.within(s1[slot], es), (self.kind, it, slot, s1[slot], es.ref)

    def check_rr(self, got, r, what):
        es = M.exact_sum(r, r)
        print('%s m%d %s RR: got %.17g ref %.17g err %.3g bound %.3g'
              % (self.kind, self.m, what, got, es.ref, float(M.error(got, es)),
                 float(M.bound(es))))
        assert M.within(got, es), (self.kind, what, got, es.ref)

    # -- K3
    def plant_k3(self, it):
        """z (the current buffer) in [0, 1], g of iteration it with |g| in
        [0.25, 4], fillers in what K3 writes; returns what was planted."""
        zc, zn = (it - 1) & 1, it & 1
        rs = np.random.RandomState(it)
        st = {'z%d' % zc: self.pl['z'], 'z%d' % zn: np.full(self.nz, 0.5),
              'x': rs.uniform(-2.0, 2.0, size=self.n), 'dz': rs.uniform(-2.0, 2.0, size=self.nz),
              'r': self.pl['r']}
        self.put(self.eng.z[0], st['z0'])
        self.put(self.eng.z[1], st['z1'])
        self.put(self.eng.x, st['x'])
        self.put(self.dz, st['dz'])
        self.put(self.eng.g[zn], self.pl['g_step'])
        self.eng.load_r(st['r'])
        return st

    def k3_state(self):
        return {'z0': self.get(self.eng.z[0], self.nz), 'z1': self.get(self.eng.z[1], self.nz),
                'x': self.get(self.eng.x), 'dz': self.get(self.dz), 'r': self.get(self.eng.r)}


@pytest.fixture(scope='module')
def rigs(cuda):
    """rigs(kind, m): the engine of a kind on a problem, built once per module."""
    cache = {}

    def get(kind, m):
        if (kind, m) not in cache:
            cache[kind, m] = Rig(kind, m)
        return cache[kind, m]
    yield get
    cache.clear()


def roles_of(kind):
    return (0,) if kind == 'fixed' else (0, 1, 2)


# ---- 1. K2's four sums --------------------------------------------------------------

@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', ALL)
def test_k2_sums(rigs, kind, m):
    """Stage 3 at iterations 1 and 2 (both buffer parities): SUMDG, DZDG, DGDG,
    GG within the bound of the exact sums, every other slot untouched; at
    iteration 0 nothing of scal is written; after a stop g and the sums stay
    (shard_role 0, 1) or the sums are zeroed for the all-reduce (shard_role 2:
    stage 3 SUMDG..GG, stage 10 SUMDG..RR)."""
    rig = rigs(kind, m)
    eng, pl = rig.eng, rig.pl
    for it in (1, 2):
        rig.plant_k2(it, pl['r'])
        s0 = rig.sentinels()
        s1 = rig.run(s0, 3, it)
        rig.check_k2_sums(it, s1)
        unchanged(s0, s1, SUMS)
    rig.plant_k2(1, pl['r'])
    s0 = rig.sentinels()
    s1 = rig.run(s0, 3, 0)
    unchanged(s0, s1, [])
    # stopped
    for role in roles_of(kind):
        for stage in ((3,) if kind == 'fixed' else (3, 10)):
            rig.plant_k2(1, pl['r'])
            g0, g1 = rig.get(eng.g[0]), rig.get(eng.g[1])
            s0 = rig.sentinels(STOP=float(M.STOP_MAXITER))
            eng.P.shard_role = role
            try:
                s1 = rig.run(s0, stage, 1)
            finally:
                eng.P.shard_role = 0
            assert same_bits(rig.get(eng.g[0]), g0) and same_bits(rig.get(eng.g[1]), g1)
            zeroed = [] if role != 2 else (SUMS if stage == 3 else SUMS + [S_RR])
            unchanged(s0, s1, zeroed)
            assert same_bits(s1[zeroed], np.zeros(len(zeroed))), (role, stage, s1)


# ---- 2. the K1 finish ---------------------------------------------------------------

def check_finish(rig, s0, s1, it, r, what):
    """RR within the bound of sum r^2 over the device's r, FX from the device's
    own RR bit for bit, ITER / ZBUF written only inside an iteration."""
    rig.check_rr(s1[S_RR], r, what)
    assert same_bits(s1[S_FX], M.fx_of(float(s1[S_RR])))
    written = [S_RR, S_FX]
    if it > 0:
        written += [S_ITER, S_ZBUF]
        assert s1[S_ITER] == it and s1[S_ZBUF] == (it & 1)
    unchanged(s0, s1, written)


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', ALL)
def test_k1_finish(rigs, kind, m):
    """Stage 7 (r = A x + target from a planted x) at iterations 0 and 3;
    stages 9 (r as it is) and 2 (r += target) on the one-rank shard."""
    rig = rigs(kind, m)
    eng, pl = rig.eng, rig.pl
    x = pl['x']
    xg = eng.colv.cpu().numpy() * x if eng.scaled else x
    for it in (0, 3):
        rig.put(eng.x, xg)
        if eng.fixed_sums:
            eng.set_x_bound(float(np.max(np.abs(xg))))
        eng.r.fill_(-7.0)
        s0 = rig.sentinels()
        s1 = rig.run(s0, 7, it)
        r = rig.get(eng.r)
        want = rig.A.dot(x) + rig.target
        if not eng.fixed_sums:
            # (r itself: test_gpu_handoffs.py; here only that K1 ran on the planted x)
            tol = 2 * (rig.n + 4) * 2.0 ** -53 * (abs(rig.A).dot(np.abs(x)) + np.abs(rig.target))
            assert np.all(np.abs(r - want) <= tol)
        assert M.terms_ok(r * r)
        check_finish(rig, s0, s1, it, r, 'stage 7 it %d' % it)
    for it in (0, 3):
        eng.load_r(pl['r'])
        s0 = rig.sentinels()
        if kind == 'fixed':
            s1 = rig.run(s0, 9, it)
        else:
            with rig.role(1):
                s1 = rig.run(s0, 9, it)
        r = rig.get(eng.r)
        assert same_bits(r, pl['r'])
        check_finish(rig, s0, s1, it, r, 'stage 9 it %d' % it)
    if kind != 'fixed':
        eng.load_r(pl['r'])
        s0 = rig.sentinels()
        with rig.role(1):
            s1 = rig.run(s0, 2, 3)
        r = rig.get(eng.r)
        assert same_bits(r, pl['r'] + rig.target)
        assert M.detectable(r * r) == (True, 0)
        check_finish(rig, s0, s1, 3, r, 'stage 2')


# ---- 3. the slices of ||r||^2 ---------------------------------------------------------

@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', SLICED)
def test_rr_slices(rigs, kind, m):
    """Stage 8: ||r||^2 over the whole of r, f and the record of iteration
    iter - 1, then the four sums.  Stage 10 (on the link-part engine:
    bsls_bb_k2_part 0 .. 2): ||r||^2 over rows [rr_lo, rr_hi) only -- the rows
    just outside at +-64 -- the four sums as stage 3's, and the previous sums
    kept in PSUMDG..PGG bit for bit."""
    rig = rigs(kind, m)
    eng, pl = rig.eng, rig.pl
    parts = kind == 'parts'
    with rig.role(1):
        if not parts:
            for it in (1, 2):
                rig.plant_k2(it, pl['r'])
                s0 = rig.sentinels()
                s1 = rig.run(s0, 8, it)
                rig.check_k2_sums(it, s1)
                rig.check_rr(s1[S_RR], pl['r'], 'stage 8 it %d' % it)
                assert same_bits(s1[S_FX], M.fx_of(float(s1[S_RR])))
                written = SUMS + [S_RR, S_FX]
                if it - 1 > 0:
                    written += [S_ITER, S_ZBUF]
                    assert s1[S_ITER] == it - 1 and s1[S_ZBUF] == ((it - 1) & 1)
                unchanged(s0, s1, written)
        assert M.SHORT[1] - M.SHORT[0] < rig.k2_wgs
        if parts:
            # a slice across a bound of the link parts
            assert any(107 < c < 214 for c in rig.group_col)
        try:
            for k, (lo, hi) in enumerate(M.slices(m)):
                it = 1 + (k & 1)
                a, c = M.slice_rows(m, lo, hi)
                r = M.slice_r(pl['r'], lo, hi)
                rig.plant_k2(it, r)
                eng.set_rr_slice(lo, hi)
                s0 = rig.sentinels()
                rig.put(eng.scal, s0)
                if parts:
                    for q in range(3):
                        eng.k2_part(it, q)
                else:
                    eng.stage(10, it)
                s1 = rig.get(eng.scal)
                assert M.terms_ok(r[a:c] * r[a:c])
                rig.check_rr(s1[S_RR], r[a:c], 'slice (%d, %d)' % (lo, hi))
                rig.check_k2_sums(it, s1)
                assert same_bits(s1[PSUMS], s0[SUMS])
                unchanged(s0, s1, SUMS + PSUMS + [S_RR])
        finally:
            eng.set_rr_slice(0, 0)


# ---- 4. the step ----------------------------------------------------------------------

def step_stages(rig):
    """(stage, shard_role) of every K3 entry: stage 4, and on the one-rank shard
    stage 13 (stage 12 folded in) and stage 15 (and the next K1's r
    initialisation, where the engine folds it)."""
    return [(4, 0)] if rig.kind == 'fixed' else [(4, 0), (13, 1), (15, 1)]


def run_step(rig, s0, stage, role, it):
    rig.eng.P.shard_role = role
    try:
        return rig.run(s0, stage, it)
    finally:
        rig.eng.P.shard_role = 0


def step_written(stage, it):
    """What a K3 entry writes beside T and WARN: the folded stage 12 records f,
    and the iteration it closes when there is one."""
    if stage == 4:
        return []
    return [S_FX] + ([S_ITER, S_ZBUF] if it - 1 > 0 else [])


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', ALL)
def test_step_t_and_warn(rigs, kind, m):
    """T = DZDG / DGDG bit for bit; WARN grows by exactly one at |t| = 1e-10,
    at nextafter(1e10, inf) and at 1e300, and not at nextafter(1e-10, 1) or
    1e10 (BB.py:27), either sign.  No inf or NaN t."""
    rig = rigs(kind, m)
    table = [(3.7 / 1.3, False, 3.7, 1.3)] + [(t, w, t, 1.0) for t, w in M.warn_table()]
    for stage, role in step_stages(rig):
        for k, (t, grows, dzdg, dgdg) in enumerate(table):
            it = 2 + (k & 1)
            st = rig.plant_k3(it)
            s0 = rig.sentinels(SUMDG=1.5, DZDG=dzdg, DGDG=dgdg, RR=6.0, PGG=1e6, PDGDG=1.0)
            s1 = run_step(rig, s0, stage, role, it)
            assert dzdg / dgdg == t and math.isfinite(t)
            assert same_bits(s1[S_T], t), (stage, t, s1[S_T])
            assert s1[S_WARN] == s0[S_WARN] + (1.0 if grows else 0.0), (stage, t, s1[S_WARN])
            assert s1[S_STOP] == 0.0
            written = [S_T, S_WARN] + step_written(stage, it)
            if stage != 4:
                assert same_bits(s1[S_FX], M.fx_of(6.0))
                assert s1[S_ITER] == it - 1 and s1[S_ZBUF] == ((it - 1) & 1)
            unchanged(s0, s1, written)
            got = rig.k3_state()
            zn = got['z%d' % (it & 1)]
            assert same_bits(got['z%d' % ((it - 1) & 1)], st['z%d' % ((it - 1) & 1)])
            assert np.all((zn >= 0.0) & (zn <= 1.0)) and not same_bits(zn, st['z%d' % (it & 1)])
            if stage == 15 and rig.folds:
                assert same_bits(got['r'], rig.target)
            else:
                assert same_bits(got['r'], st['r'])


@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', ALL)
def test_step_no_change_exit(rigs, kind, m):
    """BB.py:22: SUMDG = 0.0 or -0.0 with early_exit on stops with
    STOP_NOCHANGE, ITER = iter, ZBUF = (iter - 1) & 1 and leaves both z
    buffers, x, dz (and r) as they were; with early_exit off the step is
    taken."""
    rig = rigs(kind, m)
    eng = rig.eng
    for stage, role in step_stages(rig):
        for k, sumdg in enumerate((0.0, -0.0)):
            it = 2 + k
            st = rig.plant_k3(it)
            s0 = rig.sentinels(SUMDG=sumdg, DZDG=0.5, DGDG=1.0, RR=6.0, PGG=1e6, PDGDG=1.0)
            s1 = run_step(rig, s0, stage, role, it)
            assert s1[S_STOP] == M.STOP_NOCHANGE and s1[S_ITER] == it
            assert s1[S_ZBUF] == ((it - 1) & 1)
            if stage != 4:
                assert same_bits(s1[S_FX], M.fx_of(6.0))
            unchanged(s0, s1, [S_STOP, S_ITER, S_ZBUF] + ([S_FX] if stage != 4 else []))
            got = rig.k3_state()
            for key in st:
                assert same_bits(got[key], st[key]), (stage, key)
        eng.P.early_exit = 0
        try:
            it = 2
            st = rig.plant_k3(it)
            s0 = rig.sentinels(SUMDG=0.0, DZDG=0.5, DGDG=1.0, RR=6.0, PGG=1e6, PDGDG=1.0)
            s1 = run_step(rig, s0, stage, role, it)
        finally:
            eng.P.early_exit = 1
        assert s1[S_STOP] == 0.0 and same_bits(s1[S_T], 0.5)
        unchanged(s0, s1, [S_T] + step_written(stage, it))
        got = rig.k3_state()
        assert not same_bits(got['z0'], st['z0']) and same_bits(got['z1'], st['z1'])
        # z - t g projected: a step was taken from the planted z
        assert not same_bits(got['z0'], got['z1'])


# ---- 5. the stop rule -----------------------------------------------------------------

@pytest.mark.parametrize('m', MS)
@pytest.mark.parametrize('kind', ALL)
def test_stop_rule(rigs, orc, kind, m):
    """bb_stop_reason through its three callers -- stage 9 (bb_record_f, on GG /
    DGDG), stage 12 and stage 13's fold (on PGG / PDGDG) -- against
    oracle.stopping on vectors with the rows' norms.  The pair of slots the
    caller must not read holds a gg that decides the other way.  On a stop
    stages 12 and 13 put SUMDG..GG back to PSUMDG..PGG, and stage 13 leaves z
    untouched."""
    rig = rigs(kind, m)
    eng = rig.eng
    try:
        for row in M.stop_table():
            want = M.oracle_reason(row, orc.stopping)
            decoy = 0.0 if want == 0 else 1e6
            eng.P.max_iter, eng.P.opt_tol, eng.P.early_exit = row.max_iter, row.opt_tol, \
                row.early_exit
            fx = M.fx_of(row.rr)
            it = row.it
            # stage 9
            eng.load_r(M.r_with_sq(m, row.rr))
            s0 = rig.sentinels(GG=row.gg, DGDG=row.dgdg, PGG=decoy, PDGDG=1.0)
            s1 = run_step(rig, s0, 9, 0 if kind == 'fixed' else 1, it)
            assert s1[S_STOP] == want, (row, 9, s1[S_STOP])
            assert s1[S_RR] == row.rr and same_bits(s1[S_FX], fx)
            assert s1[S_ITER] == it and s1[S_ZBUF] == (it & 1)
            unchanged(s0, s1, [S_STOP, S_RR, S_FX, S_ITER, S_ZBUF])
            if kind == 'fixed':
                continue
            for stage in (12, 13):
                st = rig.plant_k3(it + 1)
                s0 = rig.sentinels(SUMDG=1.5, DZDG=0.5, DGDG=1.0, GG=decoy, RR=row.rr,
                                   PGG=row.gg, PDGDG=row.dgdg)
                s1 = run_step(rig, s0, stage, 1, it + 1)
                assert s1[S_STOP] == want, (row, stage, s1[S_STOP])
                assert same_bits(s1[S_FX], fx)
                assert s1[S_ITER] == it and s1[S_ZBUF] == (it & 1)
                written = [S_STOP, S_FX, S_ITER, S_ZBUF]
                got = rig.k3_state()
                if want:
                    assert same_bits(s1[SUMS], s0[PSUMS])
                    written += SUMS
                    for key in st:
                        assert same_bits(got[key], st[key]), (row, stage, key)
                elif stage == 13:
                    assert same_bits(s1[S_T], 0.5)
                    written += [S_T]
                    zn = 'z%d' % ((it + 1) & 1)
                    assert not same_bits(got[zn], st[zn])
                unchanged(s0, s1, written)
    finally:
        eng.P.max_iter, eng.P.opt_tol, eng.P.early_exit = OPTS['max_iter'], OPTS['opt_tol'], 1
