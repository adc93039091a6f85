"""The batched BB engine (device.BatchBB, bsls_bbm_*, csrc/bbm.hip): the SpMM
and its row finish alone against SciPy, columns that do not leak into each
other, iterates against the oracle run per problem (a masked problem the way
the reference holds links out: the row subset A[train], b[train]; weights on
rows scaled by their exact square roots), freezing of a stopped problem, blocks
longer than a pack, kfold(batch=) and every refusal.  Needs an MI355X."""
import math

import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def elem_err(a, b):
    """max over elements of |a - b| / max(1, |b|) (the project's iterate contract)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


_SHARDS = {}


def shard(n, p, m):
    """(A csr, block sizes, Ax) of make_shard(n, p, m, per_col=16, seed=3), made once."""
    if (n, p, m) not in _SHARDS:
        from synthetic import make_shard
        sh = make_shard(n, p, m, per_col=16, seed=3)
        _SHARDS[(n, p, m)] = (sps.csr_matrix(sh['A']), np.asarray(sh['block_sizes']), sh['Ax'])
    return _SHARDS[(n, p, m)]


def draws(Ax, count, first=3):
    from synthetic import add_noise
    return [add_noise(Ax, 0.02, seed=first + k) for k in range(count)]


SMALL = (5_000, 250, 501)


# ---- 1. the SpMM and its finish alone ----------------------------------------
def mask_weights(m, shift=0):
    w = np.ones(m)
    w[0] = w[m - 1] = 0.0
    w[100 + shift:140 + shift] = 0.0
    return w


def mixed_weights(m, seed=5):
    w = np.random.RandomState(seed).choice([0.0, 0.25, 1.0, 4.0], size=m)
    w[0], w[m - 1], w[1], w[m - 2] = 0.0, 4.0, 0.25, 0.0
    return w


@pytest.mark.parametrize('R', [1, 2, 3, 5, 8])
def test_spmm_and_finish(cuda, parity, R):
    import torch
    import _native as S
    from device import BatchBB, batch_width
    A, sizes, Ax = shard(*SMALL)
    m, n = A.shape
    bs = draws(Ax, R)
    eng = BatchBB(A, bs, sizes, options={'max_iter': 5, 'opt_tol': 1e-30})
    RP = batch_width(R)
    assert eng.RP == RP and tuple(eng.x.shape) == (n, RP) and tuple(eng.r.shape) == (m, RP)
    assert tuple(eng.z[0].shape) == (RP, eng.nz)
    rs = np.random.RandomState(7)
    X = np.zeros((n, RP))
    X[:, :R] = rs.rand(n, R)
    x0 = np.zeros(n)
    x0[np.cumsum(sizes) - 1] = 1.0
    targets = [A.dot(x0) - b for b in bs]

    def finish(s0=None):
        """stage 1 outside an iteration on X: (r, scalars)."""
        eng.x.copy_(torch.from_numpy(X))
        eng.r.fill_(-7.0)
        eng.stage(0, 0)
        if s0 is not None:
            eng.scal[:R].copy_(torch.from_numpy(s0))
        eng.stage(1, 0)
        torch.cuda.synchronize()
        return eng.r.cpu().numpy().copy(), eng.scalars().copy()

    # A X + target, column by column against SciPy
    s0 = 1000.25 + np.arange(R * S.S_COUNT, dtype=np.float64).reshape(R, S.S_COUNT)
    s0[:, S.S_STOP] = 0.0
    r_plain, s_plain = finish(s0)
    assert eng.P.roww is None
    for j in range(R):
        want = A.dot(X[:, j]) + targets[j]
        parity('bbm_spmm_a_%d_%d' % (R, j), elem_err(r_plain[:, j], want), 1e-12)
        rr = math.fsum(r_plain[:, j] * r_plain[:, j])
        parity('bbm_rr_plain_%d_%d' % (R, j), rel(s_plain[j, S.S_RR], rr), (m + 4) * U)
        nr = np.sqrt(s_plain[j, S.S_RR])
        assert bits(s_plain[j, S.S_FX]) == bits(0.5 * (nr * nr))
        for k in range(S.S_COUNT):                       # unweighted: HELD never written
            if k not in (S.S_RR, S.S_FX):
                assert bits(s_plain[j, k]) == bits(s0[j, k]), (j, k)
    # A' R.  The entries of R are signed and within 0.01: a row of A' has 16
    # values <= 1000, so sum |terms| <= 160, and two orders of summing 16
    # terms differ by at most 2 * 15 * 2^-53 * 160 = 5.4e-13 -- inside the
    # 1e-12 (absolute where |A'R| < 1) whatever cancels; unit-scale entries
    # would put that bound at 5e-11, above the contract for a cancelled row.
    Rm = np.zeros((m, RP))
    Rm[:, :R] = 0.01 * (2.0 * rs.rand(m, R) - 1.0)
    eng.r.copy_(torch.from_numpy(Rm))
    eng.w.fill_(-7.0)
    eng.stage(2, 0)
    torch.cuda.synchronize()
    Wd = eng.w.cpu().numpy()
    AT = A.T.tocsr()
    for j in range(R):
        parity('bbm_spmm_at_%d_%d' % (R, j), elem_err(Wd[:, j], AT.dot(Rm[:, j])), 1e-12)
    # the weighted finish: a 0/1 mask on the even problems, {0, 0.25, 1, 4} on the odd
    ws = [mask_weights(m, j) if j % 2 == 0 else mixed_weights(m, 5 + j) for j in range(R)]
    for j, w in enumerate(ws):
        eng.set_row_weights(j, w)
    assert eng.P.roww == eng.roww.data_ptr()
    r_w, s_w = finish()
    for j, w in enumerate(ws):
        o = r_plain[:, j]
        want = np.where(w == 0.0, 0.0, w * o)
        assert np.array_equal(bits(r_w[:, j]), bits(want)), j
        assert np.array_equal(bits(r_w[w == 0.0, j]), bits(np.zeros(int(np.sum(w == 0.0)))))
        rr = math.fsum(w * o * o)
        held = math.fsum((o * o)[w == 0.0])
        assert held > 0.0
        parity('bbm_rr_%d_%d' % (R, j), rel(s_w[j, S.S_RR], rr), (m + 4) * U)
        parity('bbm_held_%d_%d' % (R, j), rel(s_w[j, S.S_HELD], held), (m + 4) * U)
        nr = np.sqrt(s_w[j, S.S_RR])
        assert bits(s_w[j, S.S_FX]) == bits(0.5 * (nr * nr))
        assert eng.held_out()[j] == 0.5 * s_w[j, S.S_HELD]
    # a NaN in target on a held-out row of the last problem: its r there stays
    # an exact 0.0 and its f finite, its held-out sum shows it, and no other
    # problem changes a bit
    jn = R - 1
    row = int(np.nonzero(ws[jn] == 0.0)[0][1])
    keep = eng.target.clone()
    eng.target[row, jn] = float('nan')
    r_n, s_n = finish()
    eng.target.copy_(keep)
    assert bits(r_n[row, jn]) == bits(0.0) and np.all(np.isfinite(r_n))
    assert np.isfinite(s_n[jn, S.S_RR]) and np.isfinite(s_n[jn, S.S_FX])
    assert np.isnan(s_n[jn, S.S_HELD])
    assert np.array_equal(bits(r_n), bits(r_w))
    others = [j for j in range(R) if j != jn]
    assert np.array_equal(bits(s_n[others]), bits(s_w[others]))
    # one problem's weights off again: ones for it, the rest unchanged
    eng.set_row_weights(0, None)
    r_o, s_o = finish()
    assert np.array_equal(bits(r_o[:, 0]), bits(r_plain[:, 0]))
    assert bits(s_o[0, S.S_RR]) == bits(s_plain[0, S.S_RR]) and s_o[0, S.S_HELD] == 0.0
    assert eng.held_out()[0] == 0.0
    assert np.array_equal(bits(r_o[:, 1:]), bits(r_w[:, 1:]))


# ---- 2. columns do not leak ---------------------------------------------------
def run_batch(A, bs, sizes, iters, weights=None, record=(), eng=None, **kw):
    """solve() with the iterates in `record` kept; (engine, zs, {(j, i): z})."""
    from device import BatchBB
    if eng is None:
        eng = BatchBB(A, bs, sizes, row_weights=weights,
                      options={'max_iter': iters, 'opt_tol': 1e-30}, **kw)
    rec = {}

    def log(j, i, z, dt):
        if i in record:
            rec[(j, i)] = z
        return 0.0
    zs = eng.solve(log=log, record_every=1, poll=max(1, min(iters, 10)))
    return eng, zs, rec


@pytest.mark.parametrize('R', [3, 8])
def test_columns_do_not_leak(cuda, R):
    A, sizes, Ax = shard(*SMALL)
    m = A.shape[0]
    bs = draws(Ax, R)
    ws = [None, mask_weights(m), mixed_weights(m)] + [None] * (R - 3)
    eng, za, _ = run_batch(A, bs, sizes, 10, weights=ws)
    assert eng.iterations == [10] * R
    sa = eng.scalars().copy()
    # the same engine again, and a fresh one: bit for bit
    _, zb, _ = run_batch(A, bs, sizes, 10, eng=eng)
    eng2, zc, _ = run_batch(A, bs, sizes, 10, weights=ws)
    for j in range(R):
        assert np.array_equal(bits(za[j]), bits(zb[j])) and np.array_equal(bits(za[j]), bits(zc[j]))
    assert np.array_equal(bits(sa), bits(eng.scalars())) and np.array_equal(bits(sa),
                                                                            bits(eng2.scalars()))
    # another b for problem 1: every other problem keeps its bits
    other = list(bs)
    other[1] = draws(Ax, 1, first=40)[0]
    eng.set_b(1, other[1])
    _, zd, _ = run_batch(A, other, sizes, 10, eng=eng)
    sd = eng.scalars()
    assert elem_err(zd[1], za[1]) > 1e-6
    for j in range(R):
        if j != 1:
            assert np.array_equal(bits(zd[j]), bits(za[j])), j
            assert np.array_equal(bits(sd[j]), bits(sa[j])), j
    # the problems permuted: the results permuted, bit for bit
    perm = list(np.random.RandomState(11).permutation(R))
    assert perm != sorted(perm)
    engp, zp, _ = run_batch(A, [bs[k] for k in perm], sizes, 10, weights=[ws[k] for k in perm])
    sp = engp.scalars()
    for pos, k in enumerate(perm):
        assert np.array_equal(bits(zp[pos]), bits(za[k])), (pos, k)
        assert np.array_equal(bits(sp[pos]), bits(sa[k])), (pos, k)


# ---- 3. iterates against the oracle -------------------------------------------
BIG = (50_000, 2_500, 5_000)


@pytest.fixture(scope='module')
def five(orc):
    """Five problems on the 50k-route network and the oracle's 30 iterations of
    each: three noise draws, fold 1 of 3 on the first draw (the oracle on the
    train rows), weights from {0.25, 1, 4} on the first draw (the oracle on
    rows scaled by the exact square roots {0.5, 1, 2}); and a sixth,
    b = A x0, whose target is exactly zero."""
    from cross_validation import kfold_masks
    A, sizes, Ax = shard(*BIG)
    m = A.shape[0]
    b3 = draws(Ax, 3)
    mask = kfold_masks(m, 3)[1]
    train = np.nonzero(mask)[0]
    wts = np.random.RandomState(21).choice([0.25, 1.0, 4.0], size=m)
    root = np.sqrt(wts)
    assert np.array_equal(root * root, wts)
    As = sps.csr_matrix(sps.diags(root).dot(A))
    bs = b3 + [b3[0], b3[0]]
    ws = [None, None, None, mask, wts]
    refs = [(A, b3[0]), (A, b3[1]), (A, b3[2]), (A[train], b3[0][train]), (As, root * b3[0])]
    out = dict(A=A, sizes=sizes, bs=bs, ws=ws, ref=[], f=[])
    for Ar, br in refs:
        ref = orc.bb_trace(Ar, br, sizes, 30, record_every=1)
        assert max(ref) == 30
        out['ref'].append(ref)
        out['f'].append(float(orc.solve_in_z_parts(Ar, br, sizes)['f'](ref[30])))
    for a in range(5):
        for c in range(a + 1, 5):                  # a mixed-up column cannot pass
            assert np.max(np.abs(out['ref'][a][30] - out['ref'][c][30])) > 1e-3
    x0 = orc.particular_x0(sizes)
    out['b_zero'] = A.dot(x0)
    Q = orc.solve_in_z_parts(A, out['b_zero'], sizes)
    assert not np.any(Q['target'])
    zero = orc.bb_trace(A, out['b_zero'], sizes, 30, record_every=1)
    assert max(zero) == 1 and not np.any(zero[1])
    # the oracle's reason for that exit, in the order of BB.py:25 / solvers.py:40-63
    g, gp = Q['nabla_f'](Q['z0']), Q['nabla_f'](Q['z0'] + 1)
    if sum(g - gp) == 0:
        out['zero_reason'] = 'Exiting... no change in gradient'
    else:
        assert np.square(np.linalg.norm(g)) <= 1e-30 * (1 + abs(Q['f'](zero[1])))
        out['zero_reason'] = 'Exiting... norm(grad) too small'
    return out


def check_five(P, eng, rec, parity, tag):
    import _native
    S = eng.scalars()
    for j in range(5):
        assert eng.iterations[j] == 30
        assert _native.STOP_TEXT[eng.stop_reasons[j]] == 'max_iter'
        for i in (1, 10, 30):
            parity('%s_%d_%d' % (tag, j, i), elem_err(rec[(j, i)], P['ref'][j][i]), 1e-12)
        parity('%s_%d_f' % (tag, j), rel(S[j, _native.S_FX], P['f'][j]), 1e-12)


def test_iterates_match_oracle(cuda, five, parity):
    P = five
    eng, zs, rec = run_batch(P['A'], P['bs'], P['sizes'], 30, weights=P['ws'], record=(1, 10, 30))
    assert eng.R == 5 and eng.RP == 8
    check_five(P, eng, rec, parity, 'bbm_bb')
    for j in range(5):
        assert np.array_equal(bits(zs[j]), bits(rec[(j, 30)]))


# ---- 4. freezing ----------------------------------------------------------------
def test_freezing(cuda, five, parity):
    import _native
    P = five
    eng, zs, rec = run_batch(P['A'], P['bs'] + [P['b_zero']], P['sizes'], 30,
                             weights=P['ws'] + [None], record=(1, 10, 30))
    assert eng.R == 6
    assert eng.iterations[5] == 1
    assert _native.STOP_TEXT[eng.stop_reasons[5]] == P['zero_reason']
    assert not np.any(zs[5]) and not np.any(rec[(5, 1)]) and (5, 10) not in rec
    S = eng.scalars()
    assert S[5, _native.S_ITER] == 1 and S[5, _native.S_FX] == 0.0
    check_five(P, eng, rec, parity, 'bbm_freeze')
    # enqueued past every stop: nothing of any problem moves
    before = [eng.z[k].clone() for k in range(2)], eng.scal.clone(), eng.x.clone(), eng.r.clone()
    eng.iterate(31, 3)
    after = [eng.z[k] for k in range(2)], eng.scal, eng.x, eng.r
    import torch
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0]))
    assert all(torch.equal(a, b) for a, b in zip(before[1:], after[1:]))


# ---- 5. blocks longer than a pack -----------------------------------------------
def test_long_blocks(cuda, orc, parity):
    A, sizes, Ax = shard(5_000, 40, 501)
    assert sizes.max() > 65
    bs = draws(Ax, 2)
    eng, zs, rec = run_batch(A, bs, sizes, 10, record=(1, 10))
    assert eng.nlong > 0 and eng.iterations == [10, 10]
    for j in range(2):
        ref = orc.bb_trace(A, bs[j], sizes, 10, record_every=1)
        for i in (1, 10):
            parity('bbm_long_%d_%d' % (j, i), elem_err(rec[(j, i)], ref[i]), 1e-12)


# ---- 6. kfold(batch=) -------------------------------------------------------------
@pytest.mark.parametrize('k,batch,chunks', [(3, 3, [3]), (5, 2, [2, 2, 1])])
def test_kfold_batch(cuda, orc, parity, k, batch, chunks):
    from cross_validation import kfold, kfold_masks
    from device import batch_groups
    A, sizes, Ax = shard(*BIG)
    b = draws(Ax, 1)[0]
    x0 = orc.particular_x0(sizes)
    N = orc.block_sizes_to_N(sizes)
    opts = {'max_iter': 100, 'opt_tol': 1e-30}
    assert batch_groups(k, batch) == chunks
    folds = kfold(A, b, x0, N, sizes, k, options=opts, batch=batch)
    seq = kfold(A, b, x0, N, sizes, k, options=opts, deterministic=True)
    assert len(folds) == k
    for i, (fold, ref, w) in enumerate(zip(folds, seq, kfold_masks(A.shape[0], k))):
        assert set(fold) == {'iters', 'stop', 'f_train', 'held_out', 'z', 'seconds'} == set(ref)
        assert fold['iters'] == 100 and fold['stop'] == 'max_iter'
        x = x0 + N.dot(fold['z'])
        test, train = np.nonzero(w == 0.0)[0], np.nonzero(w)[0]
        want = 0.5 * np.linalg.norm(A[test].dot(x) - b[test]) ** 2
        parity('bbm_kfold_held_out_%d_%d' % (k, i), rel(fold['held_out'], want), 1e-10)
        want = 0.5 * np.linalg.norm(A[train].dot(x) - b[train]) ** 2
        parity('bbm_kfold_f_train_%d_%d' % (k, i), rel(fold['f_train'], want), 1e-10)
        parity('bbm_kfold_z_%d_%d' % (k, i), elem_err(fold['z'], ref['z']), 1e-12)
    secs = [f['seconds'] for f in folds]
    lo = 0
    for size in chunks:                              # a chunk's time, shared evenly
        assert len(set(secs[lo:lo + size])) == 1
        lo += size


# ---- 7. rejections ------------------------------------------------------------------
def test_rejections(cuda, monkeypatch):
    import _native
    import main
    from device import BatchBB
    A, sizes, Ax = shard(*SMALL)
    m = A.shape[0]
    bs = draws(Ax, 2)
    # nothing below may reach the library
    monkeypatch.setattr(_native, 'lib', lambda: pytest.fail('the device was touched'))
    w = mask_weights(m)
    for bad in ([], [bs[0]] * 9, np.zeros((m, 9)), [bs[0], bs[1][:-1]], [np.ones(m + 1)]):
        with pytest.raises(ValueError):
            BatchBB(A, bad, sizes)
    for badw in (-w, np.where(w == 0, np.nan, w), np.ones(m - 1)):
        with pytest.raises(ValueError):
            BatchBB(A, bs, sizes, row_weights=[None, badw])
    with pytest.raises(ValueError):
        BatchBB(A, bs, sizes, row_weights=[w])              # one entry for two problems
    with pytest.raises(ValueError):
        main.solve_many(A, bs, None, None, sizes, batch=9)
    monkeypatch.undo()
    eng = BatchBB(A, bs, sizes, options={'max_iter': 2, 'opt_tol': 1e-30})
    for call in (lambda: eng.set_b(2, bs[0]), lambda: eng.set_b(0, bs[0][:-1]),
                 lambda: eng.set_row_weights(0, -w), lambda: eng.set_row_weights(5, w),
                 lambda: eng.set_z0([None]), lambda: eng.set_z0([np.zeros(3), None])):
        with pytest.raises(ValueError):
            call()
    assert eng.P.roww is None                               # a refused swap changes nothing


def test_solve_many(cuda, orc):
    """main.solve_many: three right-hand sides two at a time, in the order given."""
    import main
    A, sizes, Ax = shard(*SMALL)
    bs = draws(Ax, 3)
    x0 = orc.particular_x0(sizes)
    out = main.solve_many(A, bs, x0, None, sizes, options={'max_iter': 10, 'opt_tol': 1e-30},
                          batch=2)
    assert len(out) == 3
    for (iters, stop, z), b in zip(out, bs):
        assert iters == 10 and stop == 'max_iter'
        ref = orc.bb_trace(A, b, sizes, 10, record_every=10)[10]
        assert elem_err(z, ref) <= 1e-12
