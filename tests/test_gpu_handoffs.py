"""The hand-offs between the kernels of a fused BB iteration (csrc/bb.hip): the
split K1's partials (write-through stores), bb_k1_sum (rows in 16-B pairs, its
loads ahead of its stop test), the LDS clear under the dealt walks' first
loads, and the dz = z - z_prev that K3 leaves for the next K2 -- the fused
loop bsls_bb_iterate against the same iterations driven stage by stage
(bsls_bb_stage 3, 4, 7), over one call and over consecutive calls.

Small problems (a few hundred links, ~3k routes) with every edge the kernels
branch on: blocks of 2, 3, 63, 64, 65, 66, 130, 150 routes among random 2..40
(packs of one lane up to a full wave, and the long / serial K3 paths above 64;
a block of one route is refused by the engine, as by the reference's
projection -- checked below -- and every block's last route is an x row with
no z entry); an odd n_z; m odd with m = 1 (mod H), so the last K1 row block
is one row (scalar bb_k1_sum), and m even (the 16-B pairs); K1 in four column
groups, K2 in one; a K1 tile and a K2 tile with no entries, tiles of one
quad-step (fewer than the walk's prefill depth BSLS_TILE_P = 4) and tiles of
more than four.  Needs an MI355X.
"""
import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

SPECIAL = [2, 3, 63, 64, 65, 66, 130, 150]
K1_PLAN, K2_PLAN = (64, 4, 0), (512, 1, 0)
ENGINES = {'det': dict(deterministic=True, fmt='tiles'),
           'dealt': dict(),
           'dealt-general': dict(general=True)}


def make_problem(m, seed, noise=0.02):
    """A scaled incidence (integer flows per route) of m links; see the module
    docstring for what its pattern holds."""
    rs = np.random.RandomState(seed)
    sizes = np.concatenate([rs.randint(2, 41, size=110), SPECIAL])
    rs.shuffle(sizes)
    if (int(sizes.sum()) - len(sizes)) % 2 == 0:
        sizes = np.concatenate([sizes, [2]])           # n_z odd
    n = int(sizes.sum())
    assert (n - len(sizes)) % 2 == 1 and n > 2048
    pat = sps.random(m, n, density=0.03, random_state=rs, format='lil')
    # one K1 tile (rows 0..63, column group 0) and one K2 tile (routes 0..511)
    # of more than four quad-steps (4096 entries each)
    dense = sps.random(64, 600, density=0.6, random_state=rs, format='lil')
    pat[0:64, 0:600] = dense
    gc = np.round(np.linspace(0, n, K1_PLAN[1] + 1)).astype(int)
    pat[64:128, gc[1]:gc[2]] = 0                        # K1 tile (1, 1): no entries
    pat[:, 1024:1537] = 0                               # K2 tile 2 (its halo row too): no entries
    pat = sps.csr_matrix(pat)
    pat.eliminate_zeros()
    pat.data[:] = 1.0
    colv = rs.randint(1, 6, size=n).astype(np.float64)
    A = sps.csr_matrix(pat.multiply(colv[None, :]))
    A.sort_indices()
    # a vertex of the block simplices: one route per block carries the flow
    xv = np.zeros(n)
    xv[np.concatenate(([0], np.cumsum(sizes)[:-1])) + rs.randint(0, sizes)] = 1.0
    b = A.dot(xv)
    if noise:
        b = b * (1.0 + noise * rs.randn(m))
    return A, b, sizes


def make_engine(A, b, sizes, kind, options=None, **kw):
    from device import BBEngine
    opts = {'max_iter': 10 ** 6, 'opt_tol': 1e-30}
    opts.update(options or {})
    eng = BBEngine(A, b, sizes, options=opts, tile_plans=(K1_PLAN, K2_PLAN), **ENGINES[kind],
                   **kw)
    assert eng.fmt_A == eng.fmt_AT == 'tiles'
    assert eng.A_til.img['ngroups'] == K1_PLAN[1] and eng.AT_til.img['ngroups'] == 1
    return eng


def restart(eng):
    """The engine as new: workspace (tickets, dz, K3's warm-start masks) zeroed,
    z0 = 0, prologue."""
    import torch
    eng.work.zero_()
    eng.set_z0(torch.zeros(eng.nz, dtype=torch.float64))
    eng.prologue()


def staged(eng, first, count):
    for i in range(first, first + count):
        eng.stage(3, i)
        eng.stage(4, i)
        eng.stage(7, i)


def state(eng, with_dz=True):
    import _native
    nz = eng.nz
    out = {'z0': eng.z[0][:nz], 'z1': eng.z[1][:nz], 'g0': eng.g[0][:nz], 'g1': eng.g[1][:nz],
           'x': eng.x, 'r': eng.r, 'scal': eng.scal}
    if with_dz:
        off = _native.load().bsls_bb_dz_offset(eng.m, eng.n, nz)
        out['dz'] = eng.work[off:off + 8 * nz].view(eng.z[0].dtype)
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def compare(got, ref, exact, what):
    for k in ref:
        a, b = got[k], ref[k]
        if exact:
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (what, k)
        else:
            err = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
            assert err <= 1e-12, (what, k, err)


@pytest.fixture(scope='module', params=[321, 320], ids=['m321', 'm320'])
def problem(request):
    m = request.param
    assert m % K1_PLAN[0] == (1 if m % 2 else 0)
    return make_problem(m, seed=31 + m)


@pytest.fixture(scope='module', params=sorted(ENGINES))
def pair(request, cuda, problem):
    """(kind, the engine driven by bsls_bb_iterate, the engine driven by stages)"""
    A, b, sizes = problem
    kind = request.param
    return kind, make_engine(A, b, sizes, kind), make_engine(A, b, sizes, kind)


def tile_steps(til):
    """Quad-steps of every tile [row block, group] of an image: a dealt tile's
    walk makes wave_off[t + 1] - wave_off[t] steps of 4096 entries; a
    thread-stream tile's wave w makes (its 64-lane quads) / 64."""
    img = til.img
    wo = np.asarray(img['wave_off'], dtype=np.int64)
    nt = img['nrb'] * img['ngroups']
    if img['layout'] in (1, 2):
        steps = np.diff(wo[:nt + 1])
    else:
        steps = (np.diff(wo[:nt * 16 + 1]) >> 6).reshape(nt, 16).max(axis=1)
    return steps.reshape(img['nrb'], img['ngroups'])


def test_images_hold_the_tile_edge_cases(pair):
    """What the problem was built for is in the engine's images: a K1 tile and
    a K2 tile with no entries, and (dealt walks, prefill depth BSLS_TILE_P = 4)
    tiles of fewer steps than the prefill and tiles of more."""
    kind, fused, _ = pair
    k1, k2 = tile_steps(fused.A_til), tile_steps(fused.AT_til)
    assert k1.shape == (-(-fused.m // K1_PLAN[0]), K1_PLAN[1]) and k2.shape[1] == 1
    assert k1[1, 1] == 0 and k2[2, 0] == 0
    assert k1[0, 0] > 0 and k2[0, 0] > 0
    if kind != 'det':
        assert k1[0, 0] > 4 and k2[0, 0] > 4
        assert np.any((k1 > 0) & (k1 < 4)) and np.any((k2 > 0) & (k2 < 4))


@pytest.mark.parametrize('calls', [(1,), (2,), (3,), (7,), (3, 4), (2, 1)],
                         ids=lambda c: '+'.join(str(k) for k in c))
def test_fused_loop_matches_stage_loop(pair, calls):
    """bsls_bb_iterate(first, k) against stages 3, 4, 7 over the same
    iterations: k = 1, 2, 3, 7 (both buffer parities), and two consecutive
    calls (the second starts from the dz the first's last K3 left in the
    workspace).  z, g, x, r, dz and every scal slot: bit for bit on the
    fixed-order engine, within 1e-12 max(1, |ref|) on the dealt ones (LDS
    atomic row sums: the order varies run to run)."""
    kind, fused, ref = pair
    restart(fused)
    restart(ref)
    first = 1
    for k in calls:
        fused.iterate(first, k)
        staged(ref, first, k)
        first += k
        compare(state(fused), state(ref), kind == 'det', (kind, calls, first - 1))
    s = fused.scalars()
    import _native
    assert s[_native.S_STOP] == 0.0 and s[_native.S_ITER] == first - 1


def test_stop_by_max_iter_inside_a_call(pair):
    """max_iter below the call's count: iteration 5 of a call of 9 stops the run;
    the later kernels of the call return at their stop tests.  Stop iteration,
    reason, z, g, x, r and scal as the stage-driven loop's (w.dz is not read
    after a stop and is not compared)."""
    import _native
    kind, fused, ref = pair
    for e in (fused, ref):
        e.P.max_iter = 5
        restart(e)
    try:
        fused.iterate(1, 9)
        staged(ref, 1, 9)
        sf, sr = fused.scalars(), ref.scalars()
        assert sf[_native.S_STOP] == sr[_native.S_STOP] == _native.STOP_MAXITER
        assert sf[_native.S_ITER] == sr[_native.S_ITER] == 5
        assert sf[_native.S_ZBUF] == sr[_native.S_ZBUF] == 1
        compare(state(fused, False), state(ref, False), kind == 'det', (kind, 'max_iter'))
    finally:
        for e in (fused, ref):
            e.P.max_iter = 10 ** 6


@pytest.mark.parametrize('vi', [0, 1, 2])
def test_early_exit_inside_a_call(cuda, golden, vi):
    """A noise-free b (the three tests/fast problems: 5 links, 100 routes): the
    run ends after some hundreds of iterations by one of the reference's early
    exits -- on all three the exact-zero sum(delta_g) of BB.py:22, K3's
    STOP_NOCHANGE, at iterations 444, 567 and 775 when measured -- in the
    middle of a call of 64 iterations.  On the fixed-order engine the fused
    loop stops at the stage-driven loop's iteration with its reason (message),
    and leaves its z, g, x, r and scal, bit for bit."""
    import _native
    G = golden('solvers.npz')
    tag = 'main%d' % vi
    A = sps.csr_matrix((G[tag + '_A_data'], G[tag + '_A_indices'], G[tag + '_A_indptr']),
                       shape=tuple(G[tag + '_A_shape']))
    b, sizes = G[tag + '_b'], G[tag + '_block_sizes']
    fused = make_engine(A, b, sizes, 'det', options={'max_iter': 20000})
    ref = make_engine(A, b, sizes, 'det', options={'max_iter': 20000})
    restart(fused)
    restart(ref)
    first = 1
    while first < 20000:
        fused.iterate(first, 64)
        staged(ref, first, 64)
        first += 64
        sf, sr = fused.scalars(), ref.scalars()
        assert sf[_native.S_STOP] == sr[_native.S_STOP], (first, sf, sr)
        if sf[_native.S_STOP] != 0.0:
            break
    stop = int(sf[_native.S_STOP])
    print('early exit: reason %d (%s) at iteration %d' % (stop, _native.STOP_TEXT[stop],
                                                         int(sf[_native.S_ITER])))
    assert stop == _native.STOP_NOCHANGE, stop
    assert _native.STOP_TEXT[stop] == _native.STOP_TEXT[int(sr[_native.S_STOP])]
    assert sf[_native.S_ITER] == sr[_native.S_ITER]
    assert int(sf[_native.S_ITER]) % 64 != 0            # inside the call
    compare(state(fused, False), state(ref, False), True, 'early exit')
    zb = int(sf[_native.S_ZBUF])
    assert np.array_equal(fused.current_z(zb).cpu().numpy(), ref.current_z(zb).cpu().numpy())


@pytest.mark.parametrize('it', [0, 1])
def test_k1_sum_pairs_with_a_single_last_row(cuda, it):
    """bb_k1_sum over a row part with an odd row count in an even m (row blocks
    of 65 rows: parts of 195 rows from rows 0 and 130): 16-B pairs, then the
    single last row; and an even part.  r = A x to rounding, rows outside the
    part untouched."""
    import torch
    from device import BBEngine
    rs = np.random.RandomState(5)
    sizes = rs.randint(2, 41, size=120)
    n, m = int(sizes.sum()), 390
    pat = sps.random(m, n, density=0.03, random_state=rs, format='csr')
    pat.data[:] = 1.0
    colv = rs.randint(1, 6, size=n).astype(np.float64)
    A = sps.csr_matrix(pat.multiply(colv[None, :]))
    eng = BBEngine(A, rs.randn(m), sizes, options={'max_iter': 10, 'opt_tol': 1e-30},
                   tile_plans=((65, 2, 0), (512, 1, 0)))
    assert eng.fmt_A == 'tiles' and eng.A_til.img['ngroups'] == 2 and eng.scaled
    assert eng.row_blocks() == (6, 65)
    x = rs.rand(n)
    eng.x.copy_(torch.from_numpy(colv * x).cuda())
    want = A.dot(x)
    for rb0, rb1 in ((0, 3), (2, 5), (0, 6), (5, 6)):
        eng.r.fill_(-7.0)
        eng.residual_rows(it, rb0, rb1)
        got = eng.r.cpu().numpy()
        lo, hi = 65 * rb0, 65 * rb1
        assert np.max(np.abs(got[lo:hi] - want[lo:hi])) <= 1e-12 * np.max(np.abs(want))
        assert np.all(got[:lo] == -7.0) and np.all(got[hi:] == -7.0)


def test_one_route_block_is_refused(cuda):
    """A block of one route has no z coordinate: the engine refuses it (as the
    reference's projection asserts on it), so the fused loop never sees one."""
    from device import BBEngine
    sizes = np.array([3, 1, 4])
    A = sps.random(8, 8, density=0.5, random_state=np.random.RandomState(1), format='csr')
    with pytest.raises(ValueError):
        BBEngine(A, np.ones(8), sizes)
