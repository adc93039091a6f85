"""BBEngine(fixed_sums=True): the dealt K1 / K2 walks with order-free
fixed-point row sums (bsls_bb_problem.fx_sums, csrc/tiles.hpp fx_add).

The row sums are integers, so the bits of r and g follow from a rule that a
NumPy model can apply in any order: per term v = term * fxs, h = rint(v),
l = rint((v - h) 2^s) with s = fx_lo_shift(cols); int64 sums HI, LO; value =
HI inv + LO inv 2^-s.  Needs an MI355X."""
import os

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

SEED = 237423433


def elem_err(a, b):
    """max over elements of |a - b| / max(1, |b|) (the project's iterate contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the NumPy model of the documented rule ---------------------------------
def fx_lo_shift(cols):
    return min(50, 62 - int(cols).bit_length())


def fx_scales(B):
    """fxs = 2^(50 - e), inv = 2^(e - 50) with B = f 2^e, f in [0.5, 1)."""
    e = int(np.frexp(B)[1]) if B > 0 else 0
    e = max(e, -900)
    return np.ldexp(1.0, 50 - e), np.ldexp(1.0, e - 50)


def fx_row_sums(M, vec, B, general, group_col):
    """Per column group, every row's fixed-point sum of M's terms over `vec`
    (values times gathered entries for `general`, the gathered entries
    themselves for a scaled incidence) converted back to a double."""
    M = sps.csr_matrix(M)
    rows, cols = M.shape
    fxs, inv = fx_scales(B)
    s = fx_lo_shift(cols)
    out = []
    for g in range(len(group_col) - 1):
        sub = M[:, group_col[g]:group_col[g + 1]].tocsr()
        sub.sort_indices()
        x = vec[group_col[g] + sub.indices]
        term = sub.data * x if general else x
        v = term * fxs
        h = np.rint(v)
        lo = np.rint((v - h) * np.ldexp(1.0, s))
        ri = np.repeat(np.arange(rows), np.diff(sub.indptr))
        HI = np.zeros(rows, dtype=np.int64)
        LO = np.zeros(rows, dtype=np.int64)
        np.add.at(HI, ri, h.astype(np.int64))
        np.add.at(LO, ri, lo.astype(np.int64))
        out.append(HI.astype(np.float64) * inv + LO.astype(np.float64) * np.ldexp(inv, -s))
    return out


def model_k1(eng, A, x, general):
    """r = the group values added in group order, then + target."""
    gc = eng.A_til.img['group_col']
    vals = fx_row_sums(A, x, eng.P.fx_a1 * eng.P.x_bound, general, gc)
    o = vals[0].copy()
    for v in vals[1:]:
        o = o + v
    return o + eng.target.cpu().numpy()


def model_k2(eng, AT, r, general):
    """w_i = colv_i value_i (scaled incidence), g = N'w."""
    gc = eng.AT_til.img['group_col']
    vals = fx_row_sums(AT, r, eng.P.fx_a2 * float(np.max(np.abs(r))), general, gc)
    if len(vals) == 1:
        o = vals[0]
    else:
        o = np.zeros_like(vals[0])
        for v in vals:
            o = o + v
    w = o if general else eng.colv.cpu().numpy() * o
    xz = eng.layout.xz.cpu().numpy()
    i = np.nonzero(xz >= 0)[0]
    g = np.zeros(eng.nz)
    g[xz[i]] = w[i] - w[i + 1]
    return g


@pytest.fixture(scope='module')
def small():
    from synthetic import make_shard, add_noise
    sh = make_shard(5_000, 250, 500, per_col=16)
    b = add_noise(sh['Ax'], 0.02)
    return sh, b


def small_engine(small, general, plans, **kw):
    from device import BBEngine
    sh, b = small
    return BBEngine(sh['A'], b, sh['block_sizes'], options={'max_iter': 5, 'opt_tol': 1e-30},
                    general=general, tile_plans=plans, fixed_sums=True, **kw)


def k1_of(eng, xg):
    """Stage 7 on x as K1 gathers it."""
    import torch
    eng.x.copy_(torch.from_numpy(xg))
    eng.set_x_bound(float(np.max(np.abs(xg))))
    eng.stage(7, 0)
    torch.cuda.synchronize()
    return eng.r.cpu().numpy()


def k2_of(eng, r):
    import torch
    eng.load_r(torch.from_numpy(r).cuda())
    eng.stage(3, 0)
    torch.cuda.synchronize()
    return eng.g[0][:eng.nz].cpu().numpy()


# ---- 1. bits predicted on the host ------------------------------------------
# K1: 4 column groups, H = 192 does not divide m = 500 (and one group, finished
# in the kernel); K2: one and two groups, H = 768 does not divide n = 5000, so
# every block's halo row is the next block's first
@pytest.mark.parametrize('general', [False, True])
@pytest.mark.parametrize('layouts', [(2, 2), (1, 1)])
@pytest.mark.parametrize('g1,g2', [(4, 1), (1, 2)])
def test_bits_match_the_host_model(cuda, small, general, layouts, g1, g2):
    sh, _ = small
    eng = small_engine(small, general, ((192, g1, 0), (768, g2, 0)), tile_layouts=layouts)
    assert eng.P.fx_sums == 1 and eng.A_til.img['ngroups'] == g1
    assert eng.AT_til.img['ngroups'] == g2 and 500 % 192 and 5000 % 768
    rs = np.random.RandomState(7)
    x = rs.rand(eng.n)
    xg = x if general else eng.colv.cpu().numpy() * x
    A = sps.csr_matrix(sh['A'])
    got = k1_of(eng, xg)
    want = model_k1(eng, A, xg, general)
    assert np.array_equal(bits(got), bits(want)), float(np.max(np.abs(got - want)))
    r = rs.randn(eng.m)
    got = k2_of(eng, r)
    want = model_k2(eng, A.T.tocsr(), r, general)
    assert np.array_equal(bits(got), bits(want)), float(np.max(np.abs(got - want)))


# ---- 2. order-freeness without relying on a race -----------------------------
@pytest.mark.parametrize('general', [False, True])
def test_bits_do_not_depend_on_the_row_blocks(cuda, small, general):
    """The same column groups cut into different row blocks deal the entries to
    other lanes and steps: other orders of the LDS adds, the same r and g."""
    rs = np.random.RandomState(11)
    outs = []
    x, r = rs.rand(5_000), rs.randn(500)
    for plans in (((192, 4, 0), (768, 1, 0)), ((128, 4, 0), (1344, 1, 0))):
        eng = small_engine(small, general, plans)
        xg = x if general else eng.colv.cpu().numpy() * x
        outs.append((k1_of(eng, xg), k2_of(eng, r)))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0]))
    assert np.array_equal(bits(outs[0][1]), bits(outs[1][1]))


# ---- 3. parity, 4. repeatability ---------------------------------------------
@pytest.fixture(scope='module')
def shard50k(orc):
    from synthetic import make_shard, add_noise
    sh = make_shard(50_000, 2_500, 5_000, per_col=16, seed=3)
    b = add_noise(sh['Ax'], 0.02, seed=3)
    ref = orc.bb_trace(sh['A'], b, sh['block_sizes'], 30, record_every=1)
    return sh, b, ref


def run30(A, b, sizes, **kw):
    from device import BBEngine
    eng = BBEngine(A, b, sizes, options={'max_iter': 30, 'opt_tol': 1e-30}, fixed_sums=True, **kw)
    rec = {}

    def log(i, s, dt):
        rec[i] = s
        return 0.0
    eng.solve(log=log, record_every=1, poll=1)
    return eng, rec


@pytest.mark.parametrize('general', [False, True])
def test_iterates_match_oracle(cuda, shard50k, general, parity):
    sh, b, ref = shard50k
    eng, rec = run30(sh['A'], b, sh['block_sizes'], general=general)
    assert eng.P.fx_sums == 1 and eng.scaled == (not general)
    for i in (1, 10, 30):
        parity('bb_fixed_sums_%s_%d' % ('general' if general else 'scaled', i),
               elem_err(rec[i], ref[i]), 1e-12)


def test_iterates_match_oracle_f16_values(cuda, orc, parity):
    """Stored values that travel as _Float16 (BSLS_TILE_VAL16), as
    test_stored_value_codecs_vs_oracle sets them up."""
    from synthetic import make_shard, add_noise
    sh = make_shard(50_000, 2_500, 5_000, per_col=16, seed=3)
    A = sps.csr_matrix(sh['A'])
    b = add_noise(A.dot(sh['x_true']), 0.02, seed=3)
    ref = orc.bb_trace(A, b, sh['block_sizes'], 30, record_every=1)
    eng, rec = run30(A, b, sh['block_sizes'], general=True, fmt='tiles')
    assert eng.A_til.val_codec == 'f16' and eng.AT_til.val_codec == 'f16'
    for i in (1, 10, 30):
        parity('bb_fixed_sums_f16_%d' % i, elem_err(rec[i], ref[i]), 1e-12)


def test_two_engines_repeat_bit_for_bit(cuda, shard50k):
    sh, b, _ = shard50k
    e1, r1 = run30(sh['A'], b, sh['block_sizes'])
    e2, r2 = run30(sh['A'], b, sh['block_sizes'])
    assert np.array_equal(bits(r1[30]), bits(r2[30]))
    assert np.array_equal(bits(e1.scalars()), bits(e2.scalars()))


# ---- 5. exits ------------------------------------------------------------------
def _csr(G, tag):
    return sps.csr_matrix((G['%s_A_data' % tag], G['%s_A_indices' % tag],
                           G['%s_A_indptr' % tag]), shape=tuple(G['%s_A_shape' % tag]))


# the exit iterations of the three main problems in this mode, measured on an
# MI355X (the same on every run: the reference 454 / 569 / 745, the fixed-order
# engine 443 / 572 / 774)
FIXED_EXIT = [451, 570, 762]


@pytest.mark.parametrize('vi', [0, 1, 2])
def test_main_problems_exit_repeats(cuda, golden, vi):
    from device import BBEngine
    from c_extensions.c_extensions import z2x_c
    G = golden('solvers.npz')
    A = _csr(G, 'main%d' % vi)
    b, bs = G['main%d_b' % vi], G['main%d_block_sizes' % vi]
    runs = []
    for _ in range(2):
        eng = BBEngine(A, b, bs, options={'max_iter': 300000, 'opt_tol': 1e-30}, fixed_sums=True)
        z = eng.solve(poll=25).cpu().numpy().copy()
        runs.append((eng.iterations, z))
    print('fixed_sums exit main%d: %d' % (vi, runs[0][0]))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(bits(runs[0][1]), bits(runs[1][1]))
    xs = np.zeros(eng.n)
    z2x_c(xs, runs[0][1].copy(), eng.layout.xstarts_h)
    err = 0.5 * np.linalg.norm(A.dot(xs) - b) ** 2
    assert err < 1e-16, (vi, err)
    ref_last = int(G['main%d_iters' % vi][-1])
    assert abs(runs[0][0] - ref_last) <= max(10, ref_last // 4), (runs[0][0], ref_last)
    assert runs[0][0] == FIXED_EXIT[vi], (runs[0][0], FIXED_EXIT[vi])


# ---- 6. hard inputs ------------------------------------------------------------
def test_dense_link_of_thirds(cuda, small):
    """One row of A holds all 5000 routes and x = 1/3 everywhere: every
    remainder of that row has one sign, the worst case for the low word
    (csrc/tiles.hpp fx_lo_shift)."""
    from device import BBEngine, scaled_incidence_scale
    sh, b = small
    colv = scaled_incidence_scale(sh['A'])
    # (row 3 of column j holds that column's scale: still a scaled incidence)
    A = sps.lil_matrix(sh['A'])
    A[3, :] = colv
    A = sps.csr_matrix(A)
    ones = A.copy()
    ones.data[:] = 1.0          # the pattern alone: K1 gathers exactly 1/3
    x = np.full(A.shape[1], 1.0 / 3.0)
    for M, general in ((A, False), (A, True), (ones, False)):
        eng = BBEngine(M, b, sh['block_sizes'], options={'max_iter': 5, 'opt_tol': 1e-30},
                       general=general, fixed_sums=True)
        assert eng.scaled == (not general)
        assert int(np.max(np.diff(M.indptr))) == 5_000
        xg = x if general else eng.colv.cpu().numpy() * x
        got = k1_of(eng, xg)
        want = M.dot(x) + eng.target.cpu().numpy()
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize('general', [False, True])
def test_wide_range_residual(cuda, orc, small, general):
    sh, _ = small
    eng = small_engine(small, general, (None, None))
    rs = np.random.RandomState(13)
    r = rs.randn(eng.m) * 10.0 ** rs.uniform(-6, 6, size=eng.m)
    got = k2_of(eng, r)
    N = orc.block_sizes_to_N(sh['block_sizes'])
    want = N.T.tocsr().dot(sps.csr_matrix(sh['A']).T.tocsr().dot(r))
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_nan_in_x_reaches_r(cuda, small):
    eng = small_engine(small, False, (None, None))
    x = eng.colv.cpu().numpy() * np.random.RandomState(17).rand(eng.n)
    bound = float(np.max(np.abs(x)))
    x[1234] = np.nan
    import torch
    eng.x.copy_(torch.from_numpy(x))
    eng.set_x_bound(bound)
    eng.stage(7, 0)
    torch.cuda.synchronize()
    assert np.isnan(eng.r.cpu().numpy()).any()


# ---- 7. end to end ---------------------------------------------------------------
def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def test_main_reproducible_end_to_end(cuda, golden, tmp_path):
    import bsls_utils
    import main
    G = golden('solvers.npz')
    np.random.seed(SEED)
    fname = os.path.join(str(tmp_path), 'test_main.mat')
    bsls_utils.generate_data(fname=fname)
    args = main.parser().parse_args(['--file', fname, '--reproducible'])
    args.noise = 0
    iters, times, states, output = main.main(args=args)
    iters2, _, states2, _ = main.main(args=args)
    assert list(iters2) == list(iters)
    assert all(np.array_equal(a, b2) for a, b2 in zip(states, states2))
    err = np.asarray(output['0.5norm(Ax-b)^2'])
    assert err[-1] < 1e-16, err
    ref_iters = list(G['main0_iters'])
    assert list(iters[:-1]) == ref_iters[:-1]
    for k in range(len(ref_iters) - 1):
        assert rel(states[k], G['main0_states'][k]) < 1e-6, k
    assert rel(output['0.5norm(Ax_init-b)^2'], G['main0_err0']) < 1e-12
    assert abs(output['0.5norm(Ax*-b)^2'] - G['main0_errstar']) < 1e-20
    assert rel(err[:-1], G['main0_err'][:-1]) < 1e-6
    assert rel(output['max|f * (x-x_true)|'][:-1], G['main0_maxf'][:-1]) < 1e-6
    assert rel(output['percent flow allocated incorrectly'][:-1], G['main0_pct'][:-1]) < 1e-6
    assert iters[-1] == FIXED_EXIT[0], (iters[-1], FIXED_EXIT[0])


# ---- 8. rejections -------------------------------------------------------------
def test_engine_rejections(cuda, small):
    import _native
    from device import BBEngine
    sh, b = small
    eng = small_engine(small, False, (None, None))
    with pytest.raises(ValueError):
        eng.set_shard_role(1)
    with pytest.raises(ValueError):
        eng.set_r_fixed(2.0 ** 40)
    with pytest.raises(ValueError):
        eng.line_search()
    with pytest.raises(ValueError):
        eng.apply_A(np.zeros(eng.nz))
    # a caller's plan with no room for two words per row: refused by the
    # engine, not at the launch
    tall = _native.TILE_LDS_BYTES // 8 - 2
    with pytest.raises(ValueError, match='fixed_sums'):
        BBEngine(sh['A'], b, sh['block_sizes'], fixed_sums=True, tile_plans=(None, (tall, 1, 0)))
    with pytest.raises(ValueError, match='fixed_sums'):
        BBEngine(sh['A'], b, sh['block_sizes'], fixed_sums=True, tile_plans=((tall, 1, 0), None))


def test_library_rejections(cuda, small):
    """BSLS_E_ARG from the library itself (check() turns it into ValueError):
    the stages and entry points the mode does not cover, and a problem that
    does not meet its conditions."""
    import _native
    from _native import stream_handle
    L = _native.lib()
    eng = small_engine(small, False, (None, None))
    eng.set_z0(np.zeros(eng.nz))
    eng.prologue()
    P = eng.P
    for stage in (1, 2, 8, 10, 11, 12, 13, 14, 15):
        assert L.bsls_bb_stage(P, stage, 1, stream_handle()) == _native.BSLS_E_ARG, stage
    assert L.bsls_bb_k2_part(P, 1, 0, stream_handle()) == _native.BSLS_E_ARG
    assert L.bsls_bb_k1_rows(P, 1, 0, 1, stream_handle()) == _native.BSLS_E_ARG
    assert L.bsls_bb_residual_rows(P, 1, 0, 1, stream_handle()) == _native.BSLS_E_ARG
    for field, bad in (('shard_role', 1), ('k1_atomic', 2), ('fx_a1', 0.0),
                       ('fx_a2', float('inf')), ('x_bound', float('nan')), ('fx_sums', 2)):
        keep = getattr(P, field)
        setattr(P, field, bad)
        assert L.bsls_bb_iterate(P, 1, 1, stream_handle()) == _native.BSLS_E_ARG, field
        setattr(P, field, keep)
    # the float engine's images asked for fixed-point sums: a thread-stream
    # image, and a dealt one planned for one word per row
    from device import BBEngine
    sh, b = small
    det = BBEngine(sh['A'], b, sh['block_sizes'], deterministic=True, fmt='tiles')
    det.P.fx_sums, det.P.fx_a1, det.P.fx_a2, det.P.x_bound = 1, 16.0, 16.0, 1.0
    assert L.bsls_bb_iterate(det.P, 1, 1, stream_handle()) == _native.BSLS_E_ARG
    tall = _native.TILE_LDS_BYTES // 8 - 2
    flt = BBEngine(sh['A'], b, sh['block_sizes'], tile_plans=(None, (tall, 1, 0)))
    flt.P.fx_sums, flt.P.fx_a1, flt.P.fx_a2, flt.P.x_bound = 1, 16.0, 16.0, 1.0
    assert L.bsls_bb_iterate(flt.P, 1, 1, stream_handle()) == _native.BSLS_E_ARG
    # the engine itself still iterates
    eng.iterate(1, 2)
    import torch
    torch.cuda.synchronize()
    assert int(eng.scalars()[_native.S_ITER]) == 2
