"""The small x-space kernels of csrc/misc.hip and csrc/spmv.hip, each through
the C ABI (ctypes) against a plain high-precision restatement.  Needs an MI355X.

Mirror descent (bsls_md_update, _gated, _packs, bsls_md_step): the step
restated in np.longdouble (64-bit significand; three blocks spot-checked with
mpmath at 50 digits).  u = 2^-53 below.

  * per entry, relative: (k_b + 16 + 8 max_b|g t|) u for a block of k_b
    entries.  exp <= 2 ulp = 4u; its argument g t carries <= 4 ulp of t (log,
    sqrt, the division by the step scale) plus the product's rounding, an
    absolute error <= ~4.5 |g t| 2u that exp turns into a relative one -- once
    in the numerator and once in the block sum: 8 max|g t| u with the 16 u
    covering both exps, the multiply x * exp (twice) and the divide; the block
    sum of k_b positive terms in any order adds <= (k_b - 1) u.
  * singleton blocks stay exactly 1.0 (t = sqrt(2 ln 1) = 0);
  * every block sums to 1 within k_b u (math.fsum): the computed sum S is
    within (k_b - 1) u of the exact sum of the stored numerators and each
    quotient adds u/2;
  * the reported norm is bit-identical to max|x_new - x_old| taken on the host
    from the device's own arrays: the kernels form fabs(xn - xo) from the
    doubles they store and max is exact, so a dropped lane, workgroup or ticket
    shard shows as a different number.

N z, N' w, x <-> z: one subtraction (or a sequential running sum) per entry,
bit-identical to NumPy.

CSR SpMV: rows by math.fsum over the long-double products; per row
|out - ref| <= (nnz_row + 4) u (|alpha| sum_j |a_ij x_j| + |add_i|), the
left-to-right worst case, which any fixed summation order stays within.
"""
import math

import numpy as np
import pytest

from conftest import SEED

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
STEP_SCALE = 1.7
STEP_T = 0.37                 # bsls_md_step's own t
PREFIX = [1, 1, 2, 63, 1, 64, 65, 128, 129, 200, 1000, 32, 32, 2, 3]
FORMS = ('update', 'gated', 'packs', 'step')
NORM_FORMS = ('update', 'gated', 'packs')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ layouts

def _layout_sizes():
    tail = np.random.RandomState(SEED).randint(1, 40, 2500)
    r2 = np.random.RandomState(SEED + 1)
    return {
        # lane-63 block end (63 + 1), a full-wave block, long blocks (one with
        # a ragged last stride), 32 + 32, 64 singletons, ~800 packs / 2579 blocks
        'main': np.concatenate((PREFIX, np.ones(64, dtype=np.int64), tail)),
        'one5': [5],
        'one70': [70],
        'packs16': r2.randint(33, 65, 16),      # no two fit one wave: 16 packs
        'packs17': r2.randint(33, 65, 17),
        'blocks256': r2.randint(1, 9, 256),
        'blocks257': r2.randint(1, 9, 257),
        # the greedy planner starts a pack at the 64 singletons here (in 'main'
        # they share packs with their neighbours): mask of all ones, after a
        # pack whose last block starts on lane 63
        'aligned': [63, 1] + [1] * 64 + [32, 32, 5],
    }


class Layout:
    def __init__(self, name, sizes, seed):
        from mirror_descent import pack_blocks
        self.name = name
        self.sizes = np.asarray(sizes, dtype=np.int64)
        self.nb = int(self.sizes.size)
        self.n = int(self.sizes.sum())
        self.starts = np.concatenate(([0], np.cumsum(self.sizes)[:-1])).astype(np.int64)
        self.ends = self.starts + self.sizes
        self.block_of = np.repeat(np.arange(self.nb), self.sizes)
        self.packs = pack_blocks(self.sizes)
        self.npacks = int(self.packs[0].size)
        rs = np.random.RandomState(seed)
        x = rs.rand(self.n) + 0.05
        self.x0 = self.normalised(x)
        self.g = [3.0 * rs.randn(self.n) for _ in range(4)]
        self.lead_x = rs.rand(11) + 0.05
        self.lead_g = 3.0 * rs.randn(11)
        self.z = rs.randn(self.n - self.nb)
        self.w = rs.randn(self.n)

    def normalised(self, x):
        return x / np.repeat(np.add.reduceat(x, self.starts), self.sizes)

    def pack_of_block(self, b):
        return int(np.searchsorted(self.packs[0], self.starts[b], side='right') - 1)


_LAYOUTS = {}


def layout(name):
    if name not in _LAYOUTS:
        sizes = _layout_sizes()
        _LAYOUTS[name] = Layout(name, sizes[name], SEED + 7 + sorted(sizes).index(name))
    return _LAYOUTS[name]


LAYOUT_NAMES = sorted(_layout_sizes())


def test_layouts_reach_the_edges():
    """The shapes the tests below rely on (host only)."""
    lay = layout('main')
    assert lay.nb == 2579 and lay.n <= 60_000
    assert lay.npacks >= 9 * 16 and lay.nb >= 9 * 256         # sharded tickets: >= 9 workgroups
    x0, mask, ln = lay.packs
    m64 = [int(v) for v in mask.view(np.uint64)]
    assert x0[1] == 4 and ln[1] == 64 and m64[1] == (1 | (1 << 63))     # 63 + 1
    assert ln[2] == 64 and m64[2] == 1                                   # a full-wave block
    assert [int(v) for v in ln[3:8]] == [65, 128, 129, 200, 1000]
    assert ln[8] == 64 and m64[8] == (1 | (1 << 32))                     # 32 + 32
    assert layout('packs16').npacks == 16 and layout('packs17').npacks == 17
    assert layout('blocks256').nb == 256 and layout('blocks257').nb == 257
    assert layout('one5').npacks == 1 and layout('one70').npacks == 1
    al = layout('aligned')
    assert [int(v) for v in al.packs[1]] == [(1 | (1 << 63)) - (1 << 64), -1, 1 | (1 << 32), 1]
    for b in nan_blocks(lay):
        assert 0 <= b < lay.nb


def nan_blocks(lay):
    """Blocks that receive the NaN: 0; 100 (wave 1 of workgroup 0 of the
    lane-per-block grid); the first block of pack 48 (the fourth workgroup of
    the pack grid); block 800 (the fourth workgroup, blocks 768 .. 1023, of the
    lane-per-block grid -- its pack lies in an interior workgroup of the pack
    grid: with ~3 blocks per pack no block >= 768 falls in packs 48 .. 63)."""
    b48 = int(np.searchsorted(lay.starts, lay.packs[0][48]))
    assert lay.pack_of_block(b48) // 16 == 3
    assert 800 // 256 == 3 and 3 <= lay.pack_of_block(800) // 16 < (lay.npacks - 1) // 16
    return [0, 100, b48, 800]


# ------------------------------------------------------------------ reference

def t_update(lay, scale=STEP_SCALE):
    """t_b = sqrt(2 ln k_b) / scale per block, long double."""
    assert np.finfo(LD).nmant >= 63, 'np.longdouble is not the 80-bit format here'
    return np.sqrt(LD(2) * np.log(lay.sizes.astype(LD))) / LD(scale)


def ref_step(lay, x, g, tb):
    """x * exp(-g t_b), every block divided by its sum -- in long double."""
    t = np.repeat(np.asarray(tb, dtype=LD), lay.sizes)
    v = x.astype(LD) * np.exp(-(g.astype(LD) * t))
    return v / np.repeat(np.add.reduceat(v, lay.starts), lay.sizes)


def entry_bound(lay, g, tb, unit=U):
    """(k_b + 16 + 8 max_b|g t|) u per entry."""
    gt = np.abs(g * np.repeat(np.asarray(tb, dtype=np.float64), lay.sizes))
    return np.repeat((lay.sizes + 16 + 8.0 * np.maximum.reduceat(gt, lay.starts)) * unit,
                     lay.sizes)


def check_step(parity, tag, lay, x_old, g, x_new, tb):
    """Per-entry bound, singletons, block sums of one step's output."""
    assert np.all(np.isfinite(x_new)), tag
    ref = ref_step(lay, x_old, g, tb)
    rel = (np.abs(x_new.astype(LD) - ref) / ref).astype(np.float64)
    bound = entry_bound(lay, g, tb)
    i = int(np.argmax(rel / bound))
    parity('%s/entry_ratio' % tag, rel[i] / bound[i], 1.0)
    j = int(np.argmax(rel))
    parity('%s/entry_rel' % tag, rel[j], bound[j])
    single = lay.starts[lay.sizes == 1]
    assert np.all(x_new[single] == 1.0), tag
    worst = 0.0
    for s, e in zip(lay.starts.tolist(), lay.ends.tolist()):
        worst = max(worst, abs(math.fsum(x_new[s:e].tolist()) - 1.0) / ((e - s) * U))
    parity('%s/blocksum_ratio' % tag, worst, 1.0)


def host_norm(x_new, x_old):
    return np.max(np.abs(x_new - x_old))


def test_long_double_reference_against_mpmath(parity):
    """Three blocks (63, 1000 and a short tail block) of the long-double
    restatement against mpmath at 50 digits, at the same bound with the long
    double's unit 2^-64 in place of 2^-53."""
    import mpmath
    lay = layout('main')
    x, g = lay.x0, lay.g[0]
    tb = t_update(lay)
    ref = ref_step(lay, x, g, tb)
    bound = entry_bound(lay, g, tb, unit=2.0 ** -64)
    with mpmath.workdps(50):
        for b in (3, 10, 1000):
            s, e = int(lay.starts[b]), int(lay.ends[b])
            t = mpmath.sqrt(2 * mpmath.log(e - s)) / mpmath.mpf(STEP_SCALE)
            v = [mpmath.mpf(float(x[i])) * mpmath.exp(-(mpmath.mpf(float(g[i])) * t))
                 for i in range(s, e)]
            tot = mpmath.fsum(v)
            worst = 0.0
            for i in range(s, e):
                hi = float(ref[i])
                lo = float(ref[i] - LD(hi))
                want = v[i - s] / tot
                worst = max(worst, float(abs(mpmath.mpf(hi) + mpmath.mpf(lo) - want) / want)
                            / bound[i])
            parity('md_ref_mpmath_block%d' % b, worst, 1.0)


# ------------------------------------------------------------------ device calls

def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class MDRunner:
    """One of the three norm-reporting forms on one layout: the workspace and
    the state words are zeroed once, here, and reused by every launch."""

    def __init__(self, form, lay):
        import torch
        import _native
        self.form, self.lay = form, lay
        L = _native.lib()
        self.starts = _dev(lay.starts)
        if form == 'packs':
            self.pk = [_dev(a) for a in lay.packs]
            wb = L.bsls_md_pack_workspace_size(lay.npacks)
        else:
            wb = L.bsls_md_workspace_size(lay.nb)
        self.ws = torch.zeros(wb, dtype=torch.uint8, device='cuda')
        self.state = torch.zeros(3, dtype=torch.float64, device='cuda')
        self.dx = torch.full((1,), -1.0, dtype=torch.float64, device='cuda')

    def launch(self, x, g, tol=0.0, it=1, scale=STEP_SCALE):
        """x_new and the norm word ('update') or the three state words."""
        import _native
        from _native import check, ptr, stream_handle
        L = _native.lib()
        lay = self.lay
        xd, gd = _dev(x.copy()), _dev(g)
        if self.form == 'update':
            check(L.bsls_md_update(ptr(xd), ptr(gd), ptr(self.starts), lay.nb, lay.n, scale,
                                   ptr(self.dx), ptr(self.ws), self.ws.numel(), stream_handle()),
                  'bsls_md_update')
            return xd.cpu().numpy(), self.dx.cpu().numpy().copy()
        if self.form == 'gated':
            check(L.bsls_md_update_gated(ptr(xd), ptr(gd), ptr(self.starts), lay.nb, lay.n,
                                         scale, float(tol), it, ptr(self.state), ptr(self.ws),
                                         self.ws.numel(), stream_handle()), 'bsls_md_update_gated')
        else:
            check(L.bsls_md_update_packs(ptr(xd), ptr(gd), ptr(self.pk[0]), ptr(self.pk[1]),
                                         ptr(self.pk[2]), lay.npacks, scale, float(tol), it,
                                         ptr(self.state), ptr(self.ws), self.ws.numel(),
                                         stream_handle()), 'bsls_md_update_packs')
        return xd.cpu().numpy(), self.state.cpu().numpy().copy()


def norm_word(form, out):
    return out[0] if form == 'update' else out[1]


def md_step(starts, n, x, g, t, alias):
    """bsls_md_step: (y, x afterwards); y is x's own buffer with `alias`, else
    a separate one filled with NaN beforehand."""
    import torch
    import _native
    from _native import check, ptr, stream_handle
    L = _native.lib()
    xd = _dev(x.copy())
    gd = _dev(g) if g is not None else None
    yd = xd if alias else torch.full((n,), float('nan'), dtype=torch.float64, device='cuda')
    check(L.bsls_md_step(ptr(xd), ptr(gd), ptr(yd), ptr(_dev(starts)), int(starts.size), n,
                         float(t), stream_handle()), 'bsls_md_step')
    return yd.cpu().numpy(), xd.cpu().numpy()


def n_op(name, lay, src, nout, with_x0=None):
    """bsls_n_apply / bsls_nt_apply / bsls_z2x / bsls_x2z into a NaN-filled
    output of nout entries."""
    import torch
    import _native
    from _native import check, ptr, stream_handle
    L = _native.lib()
    sd, st = _dev(src), _dev(lay.starts)
    out = torch.full((max(nout, 1),), float('nan'), dtype=torch.float64, device='cuda')
    if name == 'bsls_n_apply':
        rc = L.bsls_n_apply(ptr(out), ptr(sd), ptr(st), lay.nb, lay.n, with_x0, stream_handle())
    elif name == 'bsls_z2x':
        rc = L.bsls_z2x(ptr(out), ptr(sd), ptr(st), lay.nb, lay.n, stream_handle())
    else:
        rc = getattr(L, name)(ptr(sd), ptr(out), ptr(st), lay.nb, lay.n, stream_handle())
    check(rc, name)
    return out.cpu().numpy()[:nout]


class SpmvRunner:
    """A hand-built CSR matrix and one tile plan on the device; the reduction
    workspace is zeroed once and reused by every launch."""

    def __init__(self, M, tiles):
        import torch
        import _native
        self.m = M['m']
        self.ip, self.ix, self.dv = _dev(M['indptr']), _dev(M['indices']), _dev(M['data'])
        self.x = _dev(M['x'])
        self.add = _dev(M['add'])
        self.tiles = _dev(tiles)
        self.ntiles = int(tiles.size - 1)
        wb = _native.lib().bsls_spmv_workspace_size(self.ntiles)
        self.ws = torch.zeros(wb, dtype=torch.uint8, device='cuda')

    def launch(self, G, alpha, with_add):
        import torch
        import _native
        from _native import check, ptr, stream_handle
        out = torch.full((self.m,), float('nan'), dtype=torch.float64, device='cuda')
        sq = torch.full((1,), float('nan'), dtype=torch.float64, device='cuda')
        check(_native.lib().bsls_csr_spmv(
            self.m, ptr(self.ip), ptr(self.ix), ptr(self.dv), ptr(self.tiles), self.ntiles,
            ptr(self.x), ptr(self.add if with_add else None), float(alpha), ptr(out), ptr(sq),
            G, ptr(self.ws), self.ws.numel(), stream_handle()), 'bsls_csr_spmv')
        return out.cpu().numpy(), float(sq.item())


# ------------------------------------------------------------------ mirror descent

@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', LAYOUT_NAMES)
def test_md_step_forms(cuda, parity, name, form):
    """Three steps in a row (each from the device's previous output, with a
    fresh g) on one workspace zeroed once: per-entry bound, singletons, block
    sums, and the norm bit for bit -- so the tickets are reset by every launch."""
    lay = layout(name)
    tag = 'md_%s_%s' % (form, name)
    x = lay.x0
    if form == 'step':
        tb = np.full(lay.nb, STEP_T)
        for k in range(3):
            y, _ = md_step(lay.starts, lay.n, x, lay.g[k], STEP_T, alias=bool(k % 2))
            check_step(parity, '%s_%d' % (tag, k), lay, x, lay.g[k], y, tb)
            x = y
        return
    run = MDRunner(form, lay)
    tb = t_update(lay)
    for k in range(3):
        xn, out = run.launch(x, lay.g[k], tol=0.0, it=k + 1)
        check_step(parity, '%s_%d' % (tag, k), lay, x, lay.g[k], xn, tb)
        want = host_norm(xn, x)
        assert same_bits(norm_word(form, out), want), (tag, k, norm_word(form, out), want)
        if form != 'update':
            assert out[0] == 0.0 and out[2] == 0.0, (tag, k)      # tol = 0: never stopped
        x = xn


def test_md_pack_form_against_lane_form(cuda, parity):
    """Same input, the two forms differ by the order of the block sums only."""
    lay = layout('main')
    tb = t_update(lay)
    xp, _ = MDRunner('packs', lay).launch(lay.x0, lay.g[0])
    xl, _ = MDRunner('gated', lay).launch(lay.x0, lay.g[0])
    xu, _ = MDRunner('update', lay).launch(lay.x0, lay.g[0])
    assert same_bits(xl, xu)                                      # one kernel, two entries
    ratio = np.abs(xp - xl) / xl / entry_bound(lay, lay.g[0], tb)
    parity('md_packs_vs_lane_ratio', float(ratio.max()), 1.0)


@pytest.mark.parametrize('form', ('gated', 'packs'))
def test_md_gate(cuda, form):
    """The stop test is a strict <: tol = the norm itself does not stop, the
    next double does, with the iteration recorded; a stopped state makes the
    next launch a no-op on x and on all three words."""
    lay = layout('main')
    x, g = lay.x0, lay.g[0]
    xa, sa = MDRunner(form, lay).launch(x, g, tol=0.0, it=1)
    nu = sa[1]
    assert same_bits(nu, host_norm(xa, x)) and nu > 0.0
    assert same_bits(sa, [0.0, nu, 0.0])
    xb, sb = MDRunner(form, lay).launch(x, g, tol=nu, it=7)
    assert same_bits(sb, [0.0, nu, 0.0]) and same_bits(xb, xa)
    run = MDRunner(form, lay)
    tol = np.nextafter(nu, np.inf)
    xc, sc = run.launch(x, g, tol=tol, it=7)
    assert same_bits(sc, [1.0, nu, 7.0]) and same_bits(xc, xa)
    xd, sd = run.launch(xc, lay.g[1], tol=tol, it=8)
    assert same_bits(xd, xc) and same_bits(sd, sc)


@pytest.mark.parametrize('form', NORM_FORMS)
def test_md_nan_in_g(cuda, form):
    """One NaN in g: its block becomes NaN, every other entry keeps the bits of
    the NaN-free run, the norm is NaN, and with tol = inf the run is not
    stopped -- np.linalg.norm(x - x_prev, inf) is NaN and NaN < tol is false
    (mirror_descent.py:50)."""
    lay = layout('main')
    x = lay.x0
    clean, _ = MDRunner(form, lay).launch(x, lay.g[0], tol=0.0, it=5)
    for b in nan_blocks(lay):
        s, e = int(lay.starts[b]), int(lay.ends[b])
        g = lay.g[0].copy()
        g[s + (e - s) // 2] = np.nan
        xn, out = MDRunner(form, lay).launch(x, g, tol=np.inf, it=5)
        inside = lay.block_of == b
        assert np.all(np.isnan(xn[inside])), (form, b)
        assert same_bits(xn[~inside], clean[~inside]), (form, b)
        assert np.isnan(norm_word(form, out)), (form, b, out)
        if form != 'update':
            assert out[0] == 0.0 and out[2] == 0.0, (form, b, out)


def test_md_step_leading_entries_alias_and_null_g(cuda, parity):
    """bsls_md_step with starts[0] = 11: the leading entries get the
    elementwise update only (within 4 ulp of the long-double value), the
    blocks the full step; d_y == d_x and a separate d_y agree bit for bit and
    the separate call leaves d_x alone; g = NULL normalises only.  2579 blocks:
    eleven workgroups."""
    base = layout('main')
    lead = 11
    starts = base.starts + lead
    n = base.n + lead
    x = np.concatenate((base.lead_x, base.x0 * 1.25))            # blocks not normalised yet
    g = np.concatenate((base.lead_g, base.g[0]))
    tb = np.full(base.nb, STEP_T)
    y_sep, x_after = md_step(starts, n, x, g, STEP_T, alias=False)
    y_al, _ = md_step(starts, n, x, g, STEP_T, alias=True)
    assert same_bits(x_after, x)
    assert same_bits(y_sep, y_al)
    want = x[:lead].astype(LD) * np.exp(-(LD(STEP_T) * g[:lead].astype(LD)))
    ulps = np.abs(y_sep[:lead].astype(LD) - want) / np.spacing(want.astype(np.float64))
    parity('md_step_lead_ulps', float(ulps.max()), 4.0)
    check_step(parity, 'md_step_lead11', base, x[lead:], g[lead:], y_sep[lead:], tb)
    # g = NULL: y = x / block sum; the leading entries are copied
    y0, x_after = md_step(starts, n, x, None, STEP_T, alias=False)
    y0a, _ = md_step(starts, n, x, None, STEP_T, alias=True)
    assert same_bits(x_after, x) and same_bits(y0, y0a)
    assert same_bits(y0[:lead], x[:lead])
    check_step(parity, 'md_step_null_g', base, x[lead:], np.zeros(base.n), y0[lead:],
               np.zeros(base.nb))


# ------------------------------------------------------------------ N, N', x <-> z

def n_apply_ref(lay, z, last):
    x = np.empty(lay.n)
    for b, (s, e) in enumerate(zip(lay.starts.tolist(), lay.ends.tolist())):
        zb = z[s - b:e - 1 - b]
        if zb.size:
            x[s:e - 1] = zb - np.concatenate(([0.0], zb[:-1]))
        x[e - 1] = last - (zb[-1] if zb.size else 0.0)
    return x


@pytest.mark.parametrize('name', LAYOUT_NAMES)
def test_n_nt_z2x_x2z(cuda, parity, name):
    """bsls_n_apply (with and without x0), bsls_nt_apply, bsls_z2x and
    bsls_x2z bit-identical to NumPy, singletons included (no z entry); and
    <N z, w> against <z, N' w> as a check of the two index maps on each other."""
    lay = layout(name)
    nz = lay.n - lay.nb
    z, w = lay.z, lay.w
    last_of = np.zeros(lay.n, dtype=bool)
    last_of[lay.ends - 1] = True
    nz_dev = {}
    for with_x0 in (0, 1):
        got = n_op('bsls_n_apply', lay, z, lay.n, with_x0=with_x0)
        assert same_bits(got, n_apply_ref(lay, z, float(with_x0))), (name, with_x0)
        nz_dev[with_x0] = got
    assert same_bits(n_op('bsls_z2x', lay, z, lay.n), n_apply_ref(lay, z, 1.0)), name
    ntw = n_op('bsls_nt_apply', lay, w, nz)
    assert same_bits(ntw, (w[:-1] - w[1:])[~last_of[:-1]]), name
    x = lay.x0
    zx = n_op('bsls_x2z', lay, x, nz)
    want = np.concatenate([np.cumsum(x[s:e - 1]) for s, e in
                           zip(lay.starts.tolist(), lay.ends.tolist())] + [np.zeros(0)])
    assert same_bits(zx, want), name
    lhs = (nz_dev[0] * w).tolist()
    rhs = (z * ntw).tolist()
    scale = math.fsum(abs(v) for v in lhs) + math.fsum(abs(v) for v in rhs)
    parity('n_nt_adjoint_%s' % name, abs(math.fsum(lhs) - math.fsum(rhs)), lay.n * U * scale)


# ------------------------------------------------------------------ CSR SpMV

def _rows_matrix(nnz_rows, ncols, rs):
    ip = np.concatenate(([0], np.cumsum(nnz_rows))).astype(np.int64)
    ix = np.concatenate([np.sort(rs.permutation(ncols)[:k]) for k in nnz_rows]
                        + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    m = int(nnz_rows.size)
    return dict(m=m, n=ncols, indptr=ip, indices=ix, data=rs.randn(ix.size), x=rs.randn(ncols),
                add=rs.randn(m))


def _spmv_reference(M):
    """Per row: the sum of the long-double products a_ij x_j by math.fsum (as a
    long double: the rounded sum plus its remainder), and sum_j |a_ij x_j|."""
    ip = M['indptr']
    p = M['data'].astype(LD) * M['x'][M['indices']].astype(LD)
    hi = p.astype(np.float64)
    lo = (p - hi.astype(LD)).astype(np.float64)
    pa = np.abs(hi)
    R = np.zeros(M['m'], dtype=LD)
    S = np.zeros(M['m'])
    for i in range(M['m']):
        a, b = int(ip[i]), int(ip[i + 1])
        if a == b:
            continue
        parts = hi[a:b].tolist() + lo[a:b].tolist()
        s1 = math.fsum(parts)
        R[i] = LD(s1) + LD(math.fsum(parts + [-s1]))
        S[i] = math.fsum(pa[a:b].tolist()) * (1.0 + 2.0 * U)
    M['R'], M['S'] = R, S
    return M


_SPMV = {}


def spmv_case(case):
    """(matrix with its reference, tile plan)."""
    import _native
    if 'big' not in _SPMV:
        rs = np.random.RandomState(SEED)
        nnz = rs.poisson(6, 3000)
        nnz[0:10] = 0
        nnz[1100:2300] = 0                 # with row 1099 alone in its tile: a tile of nothing
        nnz[-1] = 0
        nnz[500], nnz[700], nnz[1099] = 5000, 2048, 2049
        _SPMV['big'] = _spmv_reference(_rows_matrix(nnz, 7001, rs))
        _SPMV['one'] = _spmv_reference(_rows_matrix(np.array([7]), 9, rs))
        _SPMV['ends'] = np.cumsum(rs.randint(1, 40, 400))
    if case == 'm1':
        M = _SPMV['one']
        return M, _native.plan_tiles(M['indptr'])
    M = _SPMV['big']
    if case == 'plan2048':
        tiles = _native.plan_tiles(M['indptr'])
    elif case == 'plan4':
        tiles = _native.plan_tiles(M['indptr'], nzt=4)
        assert tiles.size - 1 > 1024         # the grid is 1024: workgroups walk several tiles
    else:
        ends = _SPMV['ends']
        ends = ends[ends < M['m']]
        tiles = _native.plan_tiles(M['indptr'], ends=ends)
        assert np.all(np.isin(tiles[1:-1], ends))
    assert tiles[0] == 0 and tiles[-1] == M['m'] and np.all(np.diff(tiles) > 0)
    assert np.all(np.diff(tiles) <= 1024)
    if case != 'ends':
        ip = M['indptr']
        assert np.any(ip[tiles[1:]] == ip[tiles[:-1]])         # a tile made only of empty rows
    return M, tiles


@pytest.mark.parametrize('case', ('plan2048', 'plan4', 'ends', 'm1'))
def test_csr_spmv(cuda, parity, case):
    """bsls_csr_spmv on hand-built rows (empty runs, a whole empty tile, rows
    of 5000 / 2048 / 2049 entries, Poisson(6) elsewhere) under the default
    plan, a 4-nonzero plan (> 1024 tiles: the persistent loop), a plan
    constrained by `ends`, and m = 1; every G, alpha 1 and -0.5, with and
    without `add`, the sum of squares on."""
    import _native
    M, tiles = spmv_case(case)
    run = SpmvRunner(M, tiles)
    nnz = np.diff(M['indptr'])
    empty = nnz == 0
    for alpha in (1.0, -0.5):
        for with_add in (True, False):
            add = M['add'] if with_add else np.zeros(M['m'])
            ref = LD(alpha) * M['R'] + add.astype(LD)
            bound = (nnz + 4) * U * (abs(alpha) * M['S'] + np.abs(add))
            # alpha * (+0.0) where nothing is added: +0.0, or -0.0 for alpha < 0
            # (IEEE, and what alpha * A.dot(x) gives); == 0.0 either way
            nothing = add[empty] if with_add else np.full(int(empty.sum()), alpha * 0.0)
            for G in (1, 2, 4, 8, 16, 32, 64):
                tag = 'spmv_%s_a%g_add%d_G%d' % (case, alpha, with_add, G)
                out, sq = run.launch(G, alpha, with_add)
                err = np.abs(out.astype(LD) - ref).astype(np.float64)
                ok = ~empty
                parity('%s/row_ratio' % tag, float(np.max(err[ok] / bound[ok])), 1.0)
                assert same_bits(out[empty], nothing), tag
                if not with_add:
                    assert np.all(out[empty] == 0.0), tag
                want_sq = math.fsum((out * out).tolist())
                parity('%s/sq' % tag, abs(sq - want_sq), (M['m'] + 2) * U * want_sq)
                out2, sq2 = run.launch(G, alpha, with_add)
                assert same_bits(out2, out) and same_bits(sq2, sq), tag
    # a group size that is no power of two is refused before any launch
    from _native import ptr
    assert _native.lib().bsls_csr_spmv(
        run.m, ptr(run.ip), ptr(run.ix), ptr(run.dv), ptr(run.tiles), run.ntiles, ptr(run.x),
        None, 1.0, ptr(run.add), None, 3, None, 0, None) == _native.BSLS_E_ARG
