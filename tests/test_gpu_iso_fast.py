"""The fast standalone PAVA on the MI355X (bsls_isotonic_packs_fast /
bsls_isotonic_multi_fast, BSLS_ISO=fast, csrc/pava_fast.hpp) against the
oracle's isotonic_regression_multi (variant 1, fresh unit weights, expanded).

Two accuracy tiers (include/bsls_hip.h): tier 1, |d| <= 1e-12 max(1, |ref|)
per element (close12 of test_gpu_kernels.py, the projection contract); tier 2,
|d| <= 1e-12 max(1, max |y| over the element's block), on any finite input.
Every comparison goes through the `parity` fixture (bit identity as a count of
differing elements against 0); measured errors: profiles/iso_fast_parity.jsonl.
"""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sps

from conftest import SEED

pytestmark = pytest.mark.gpu

TOL = 1e-12


@pytest.fixture(scope='module')
def cx(cuda):
    from c_extensions import c_extensions
    return c_extensions


@pytest.fixture
def fast(monkeypatch):
    monkeypatch.setenv('BSLS_ISO', 'fast')


def ends_of(starts, n):
    return np.append(starts[1:], n)


def tier1(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def block_scale(y, starts):
    """max(1, max |y| over the element's block), per element (1 before starts[0])."""
    n = y.shape[0]
    bmax = np.maximum.reduceat(np.abs(y[starts[0]:]), starts - starts[0])
    s = np.ones(n)
    s[starts[0]:] = np.repeat(bmax, np.diff(np.append(starts, n)))
    return np.maximum(1.0, s)


def tier2(got, ref, y, starts):
    return float(np.max(np.abs(got - ref) / block_scale(y, starts)))


def nbits(a, b):
    """Elements whose bits differ."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.count_nonzero(a.view(np.int64) != b.view(np.int64)))


def inversions(out, starts):
    """Neighbours inside a block with out[i + 1] < out[i] (or a NaN)."""
    bad = ~(np.diff(out) >= 0)
    bad[starts[1:] - 1] = False
    bad[:starts[0]] = False
    return float(np.count_nonzero(bad))


def oracle_fit(orc, y, starts):
    ref = y.copy()
    orc.isotonic_regression_multi_c(ref, np.ascontiguousarray(starts, dtype=np.int64))
    return ref


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def packs_call(name, y, P):
    """bsls_isotonic_packs{,_fast} on a host plan dict(start, mask, len, longs)."""
    import torch
    import _native
    L = _native.lib()
    n = y.shape[0]
    yd = torch.from_numpy(y.copy()).cuda()
    st, mk, ln = (torch.from_numpy(np.ascontiguousarray(P[k])).cuda() for k in ('start', 'mask', 'len'))
    nlong = int(P['longs'].shape[0])
    lg = torch.from_numpy(P['longs'] if nlong else np.zeros(1, np.int32)).cuda()
    ws = torch.zeros(max(L.bsls_isotonic_workspace_size(n), 16), dtype=torch.uint8, device='cuda')
    rc = getattr(L, name)(_ptr(yd), _ptr(st), _ptr(mk), _ptr(ln), int(ln.shape[0]), _ptr(lg), nlong,
                          n, _ptr(ws), ws.numel(), _native.stream_handle())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return yd.cpu().numpy()


def packs_fast(y, starts):
    import _native
    return packs_call('bsls_isotonic_packs_fast', y, _native.pack_plan(starts, y.shape[0]))


def multi_fast(y, starts):
    import torch
    import _native
    L = _native.lib()
    n = y.shape[0]
    yd = torch.from_numpy(y.copy()).cuda()
    st = torch.from_numpy(np.array(starts, dtype=np.int64)).cuda()
    ws = torch.zeros(L.bsls_isotonic_workspace_size(n), dtype=torch.uint8, device='cuda')
    mb = int(np.max(ends_of(starts, n) - starts))
    rc = L.bsls_isotonic_multi_fast(_ptr(yd), _ptr(st), len(starts), n, mb, _ptr(ws), ws.numel(),
                                    _native.stream_handle())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return yd.cpu().numpy()


# ------------------------------------------------------------------ 1. golden

def test_golden_fast_then_exact_in_one_process(cx, golden, parity, monkeypatch):
    G = golden('isotonic.npz')
    for mode in ('fast', 'exact', 'fast'):
        monkeypatch.setenv('BSLS_ISO', mode)
        for ci in range(int(G['ncases'])):
            yy = G['c%d_y' % ci].copy()
            cx.isotonic_regression_multi_c(yy, G['c%d_blocks' % ci])
            ref = G['c%d_v1_u1' % ci]
            if mode == 'fast':
                parity('iso_fast/golden/c%d' % ci, tier1(yy, ref), TOL)
            else:
                parity('iso_fast/golden/c%d/exact_bits' % ci, nbits(yy, ref), 0.0)
        y = np.array([4., 5., 1., 6., 8., 7.])
        cx.isotonic_regression_c(y, 0, 6)
        if mode == 'fast':
            parity('iso_fast/golden/kat_single', tier1(y, G['kat_single']), TOL)
        else:
            parity('iso_fast/golden/kat_single/exact_bits', nbits(y, G['kat_single']), 0.0)


# ------------------------------------------------------------------ 2. pack edges

@pytest.mark.parametrize('kind', ['randn', 'ties', 'decreasing'])
def test_pack_window_edges(cx, orc, parity, monkeypatch, kind):
    """The layout of test_isotonic_wave_path_size_classes: blocks of 1..130
    elements incl. 31/32/33, 63/64/65 and 130, 200 one-element blocks,
    blocks[0] = 7.  Blocks longer than a wave take the exact long-block kernel."""
    rs = np.random.RandomState(17)
    sizes = np.concatenate([rs.randint(1, 40, 3000), [31, 32, 33, 63, 64, 65, 130, 1, 1, 1],
                            np.ones(200, dtype=np.int64), rs.randint(30, 70, 300)])
    rs.shuffle(sizes)
    first = 7
    starts = (first + np.concatenate(([0], np.cumsum(sizes)[:-1]))).astype(np.int64)
    n = int(first + sizes.sum())
    if kind == 'randn':
        y = rs.randn(n)
    elif kind == 'ties':
        y = np.round(rs.randn(n), 0)
        y[rs.rand(n) < 0.1] = -0.0
    else:
        y = -np.arange(n, dtype=np.float64) + 0.25 * rs.randn(n)
    ref = oracle_fit(orc, y, starts)
    monkeypatch.setenv('BSLS_ISO', 'exact')
    ex = y.copy(); cx.isotonic_regression_multi_c(ex, starts)
    parity('iso_fast/edges/%s/exact_bits' % kind, nbits(ex, ref), 0.0)
    long_el = np.repeat(sizes > 64, sizes)
    assert long_el.sum() >= 65 + 130
    monkeypatch.setenv('BSLS_ISO', 'fast')
    got = y.copy(); cx.isotonic_regression_multi_c(got, starts)
    for tag, out in (('public', got), ('packs', packs_fast(y, starts)),
                     ('multi', multi_fast(y, starts))):
        parity('iso_fast/edges/%s/%s' % (kind, tag), tier1(out, ref), TOL)
        parity('iso_fast/edges/%s/%s/first_bits' % (kind, tag), nbits(out[:first], y[:first]), 0.0)
        parity('iso_fast/edges/%s/%s/long_bits' % (kind, tag),
               nbits(out[first:][long_el], ex[first:][long_el]), 0.0)
        parity('iso_fast/edges/%s/%s/inversions' % (kind, tag), inversions(out, starts), 0.0)


def _hand_plan(packs):
    """Plan arrays and block starts of packs given as lists of block sizes."""
    start, mask, ln, starts = [], [], [], []
    at = 0
    for blocks in packs:
        assert 1 <= sum(blocks) <= 64
        start.append(at)
        m, off = 0, 0
        for k in blocks:
            m |= 1 << off
            starts.append(at + off)
            off += k
        mask.append(np.uint64(m).astype(np.int64))
        ln.append(off)
        at += off
    P = dict(start=np.array(start, np.int64), mask=np.array(mask, np.int64),
             len=np.array(ln, np.int32), longs=np.zeros(0, np.int32))
    return P, np.array(starts, np.int64), at


def _random_packs(rs, npacks):
    out = []
    for _ in range(npacks):
        tot, blocks = int(rs.randint(1, 65)), []
        while tot > 0:
            k = int(min(tot, rs.randint(1, 40)))
            blocks.append(k)
            tot -= k
        out.append(blocks)
    return out


@pytest.mark.parametrize('case', ['one64', 'ones64', 'lane63_then1', 'n1', 'n5', 'n4097'])
def test_hand_made_plans_through_the_c_abi(cuda, orc, parity, case):
    """bsls_isotonic_packs_fast on plans written by hand: a full wave as one
    block, 64 one-element blocks, a block ending on lane 63 followed by a pack
    of one element, and 1 / 5 / 4097 packs (the last workgroup's waves with no
    pack)."""
    rs = np.random.RandomState(17)
    packs = {'one64': [[64]], 'ones64': [[1] * 64], 'lane63_then1': [[40, 24], [1]],
             'n1': _random_packs(rs, 1), 'n5': _random_packs(rs, 5),
             'n4097': _random_packs(rs, 4097)}[case]
    P, starts, n = _hand_plan(packs)
    for kind in ('randn', 'ties'):
        y = rs.randn(n) if kind == 'randn' else np.round(rs.randn(n), 0)
        ref = oracle_fit(orc, y, starts)
        got = packs_call('bsls_isotonic_packs_fast', y, P)
        parity('iso_fast/hand/%s/%s' % (case, kind), tier1(got, ref), TOL)
        parity('iso_fast/hand/%s/%s/inversions' % (case, kind), inversions(got, starts), 0.0)
        ex = packs_call('bsls_isotonic_packs', y, P)
        parity('iso_fast/hand/%s/%s/exact_bits' % (case, kind), nbits(ex, ref), 0.0)


# ------------------------------------------------------------------ 3. pass-loop shapes

def _shape(name, k):
    i = np.arange(k, dtype=np.float64)
    if name == 'decreasing':
        return k - i
    if name == 'equal':
        return np.full(k, 0.3)
    if name == 'sawtooth':
        return 1.0 - (np.arange(k) % 2)
    if name == 'stair_pairs':                       # [1, 0, 2, 1, 3, 2, ...]
        return (np.arange(k) // 2 + 1.0) - (np.arange(k) % 2)
    if name == 'low_last':
        v = i.copy()
        v[-1] = -100.0
        return v
    if name == 'pm1e8':
        return 1.0 + 1e8 * (1.0 - 2.0 * (np.arange(k) % 2))
    raise KeyError(name)


@pytest.mark.parametrize('name', ['decreasing', 'equal', 'sawtooth', 'stair_pairs', 'low_last',
                                  'pm1e8'])
def test_shapes_that_stress_the_pass_loop(cx, orc, parity, fast, name):
    """One block per pack, ~300 packs per length (64: a full wave; 50: the lanes
    past L idle; 17: one lane past a DPP row), tile t scaled by 1 + t % 5."""
    ys, sizes = [], []
    for k in (64, 50, 17):
        for t in range(100):
            ys.append(_shape(name, k) * (1.0 + t % 5))
            sizes.append(k)
    y = np.concatenate(ys)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    ref = oracle_fit(orc, y, starts)
    got = y.copy(); cx.isotonic_regression_multi_c(got, starts)
    if name == 'pm1e8':
        # |y| ~ 1e8 around a mean of 1: the prefix sums carry 1e8 u, tier 2 only
        parity('iso_fast/shapes/%s/tier2' % name, tier2(got, ref, y, starts), TOL)
    else:
        parity('iso_fast/shapes/%s' % name, tier1(got, ref), TOL)
    if name == 'equal':
        parity('iso_fast/shapes/equal/input_bits', nbits(got, y), 0.0)
    parity('iso_fast/shapes/%s/inversions' % name, inversions(got, starts), 0.0)


# ------------------------------------------------------------------ 4. already isotonic

def test_already_isotonic_input_comes_back_bit_for_bit(cuda, parity):
    """Sorted blocks with duplicated neighbours and signed zeros, C3-like block
    sizes, 20k blocks, elements before starts[0]: both new entries return the
    input's bits."""
    rs = np.random.RandomState(SEED)
    sizes = rs.multinomial(20_000 * 18, np.ones(20_000) / 20_000) + 1
    first = 11
    starts = (first + np.concatenate(([0], np.cumsum(sizes)[:-1]))).astype(np.int64)
    n = int(first + sizes.sum())
    y = np.round(rs.randn(n), 1)
    y[rs.rand(n) < 0.1] = -0.0
    y[rs.rand(n) < 0.1] = 0.0
    bid = np.repeat(np.arange(len(sizes)), sizes)
    y[first:] = y[first:][np.lexsort((y[first:], bid))]    # -0.0 == 0.0: both orders occur
    dup = rs.rand(n) < 0.3
    dup[:first + 1] = False
    dup[starts] = False
    y[dup] = y[np.flatnonzero(dup) - 1]                     # may break order: re-sort
    y[first:] = y[first:][np.lexsort((y[first:], bid))]
    assert inversions(y, starts) == 0
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    parity('iso_fast/sorted/packs/input_bits', nbits(packs_fast(y, starts), y), 0.0)
    parity('iso_fast/sorted/multi/input_bits', nbits(multi_fast(y, starts), y), 0.0)


# ------------------------------------------------------------------ 5. C3 layout

@pytest.fixture(scope='module')
def c3(orc):
    """The C3 z layout of test_isotonic_c3_full_size (950k entries, 50k
    blocks), a late-BB-step-like input and its oracle fit."""
    rs = np.random.RandomState(SEED)
    sizes = rs.multinomial(1_000_000 - 50_000, np.ones(50_000) / 50_000) + 1
    zst = np.concatenate(([0], np.cumsum(sizes - 1)[:-1])).astype(np.int64)
    nz = int((sizes - 1).sum())
    y = rs.rand(nz) - 0.3 * rs.randn(nz)
    ref = oracle_fit(orc, y, zst)
    for a in (zst, y, ref):
        a.setflags(write=False)
    return zst, y, ref


def test_c3_monotone_and_deterministic(cuda, c3, parity):
    zst, y, ref = c3
    a = packs_fast(y, zst)
    parity('iso_fast/c3/packs', tier1(a, ref), TOL)
    parity('iso_fast/c3/packs/inversions', inversions(a, zst), 0.0)
    parity('iso_fast/c3/packs/rerun_bits', nbits(packs_fast(y, zst), a), 0.0)
    b = multi_fast(y, zst)
    parity('iso_fast/c3/multi', tier1(b, ref), TOL)
    parity('iso_fast/c3/multi/inversions', inversions(b, zst), 0.0)
    parity('iso_fast/c3/multi/rerun_bits', nbits(multi_fast(y, zst), b), 0.0)
    # The window plan's packs are not the planned ones, so a block can sit on
    # other lanes and its prefix sum add up in another order: not bit for bit.
    # Each entry is within 9.0e-13 max |y| of the exact fit (the tier-2
    # derivation), so the two differ by at most 1.8e-12 max(1, max |y| of the
    # block).
    print('multi_fast vs packs_fast: %d of %d elements differ in bits' % (nbits(a, b), a.size))
    parity('iso_fast/c3/multi_vs_packs/tier2', tier2(b, a, y, zst), 1.8e-12)


# ------------------------------------------------------------------ 6. wide range

def test_wide_range_meets_tier_2(cuda, orc, parity):
    rs = np.random.RandomState(17)
    sizes = rs.randint(1, 65, 2000)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    n = int(sizes.sum())
    y = rs.randn(n) * 10.0 ** rs.uniform(-6, 6, n)
    ref = oracle_fit(orc, y, starts)
    for tag, got in (('packs', packs_fast(y, starts)), ('multi', multi_fast(y, starts))):
        print('wide range, %s: tier-1 ratio %.3e (logged, not asserted)' % (tag, tier1(got, ref)))
        parity('iso_fast/wide/%s/tier2' % tag, tier2(got, ref, y, starts), TOL)
        parity('iso_fast/wide/%s/inversions' % tag, inversions(got, starts), 0.0)


# ------------------------------------------------------------------ 7. non-finite

def test_non_finite_input_returns_and_spares_the_other_blocks(cuda, orc, parity):
    rs = np.random.RandomState(17)
    sizes = rs.randint(1, 65, 600)                    # ~300 packs
    first = 3
    starts = (first + np.concatenate(([0], np.cumsum(sizes)[:-1]))).astype(np.int64)
    n = int(first + sizes.sum())
    y = rs.randn(n)
    big = np.flatnonzero(sizes >= 20)
    bn, bi = int(big[5]), int(big[40])
    y[starts[bn] + 7] = np.nan
    y[starts[bi] + 2] = np.inf
    clean = y.copy()
    clean[~np.isfinite(clean)] = 0.0
    ref = oracle_fit(orc, clean, starts)
    keep = np.ones(n, bool)
    for b in (bn, bi):
        keep[starts[b]:starts[b] + sizes[b]] = False
    for tag, got in (('packs', packs_fast(y, starts)), ('multi', multi_fast(y, starts))):
        parity('iso_fast/nonfinite/%s' % tag, tier1(got[keep], ref[keep]), TOL)
        parity('iso_fast/nonfinite/%s/first_bits' % tag, nbits(got[:first], y[:first]), 0.0)


# ------------------------------------------------------------------ 8. surface

@pytest.fixture(scope='module')
def shard_engine(cuda):
    from device import BBEngine
    from synthetic import make_shard, add_noise
    sh = make_shard(60000, 3000, 8000, per_col=16, seed=3)
    b = add_noise(sh['Ax'], 0.02, seed=3)
    return BBEngine(sh['A'], b, sh['block_sizes'], AT=sh['AT'])


def test_isoplan_apply_keyword_and_environment(shard_engine, orc, parity, monkeypatch):
    import torch
    eng = shard_engine
    zst, nz = eng.layout.zstarts_h, eng.nz
    rs = np.random.RandomState(5)
    y = rs.rand(nz) - 0.3 * rs.randn(nz)
    ref = oracle_fit(orc, y, zst)
    plan = eng.layout.iso_plan()
    monkeypatch.delenv('BSLS_ISO', raising=False)
    dev = lambda: torch.from_numpy(y.copy()).cuda()
    ex = plan.apply(dev(), fast=False).cpu().numpy()
    fa = plan.apply(dev(), fast=True).cpu().numpy()
    parity('iso_fast/surface/apply/exact_bits', nbits(ex, ref), 0.0)
    parity('iso_fast/surface/apply/default_is_exact', nbits(plan.apply(dev()).cpu().numpy(), ref), 0.0)
    parity('iso_fast/surface/apply/fast_vs_exact', tier1(fa, ex), TOL)
    monkeypatch.setenv('BSLS_ISO', 'fast')
    parity('iso_fast/surface/apply/env_fast_bits', nbits(plan.apply(dev()).cpu().numpy(), fa), 0.0)
    parity('iso_fast/surface/apply/keyword_overrides_env',
           nbits(plan.apply(dev(), fast=False).cpu().numpy(), ex), 0.0)
    monkeypatch.setenv('BSLS_ISO', 'quick')
    with pytest.raises(ValueError, match='BSLS_ISO must be fast or exact'):
        plan.apply(dev())


def test_engine_proj_and_blockproj_follow_the_switch(shard_engine, orc, parity, monkeypatch):
    import torch
    from algorithm_utils import BlockProj
    eng = shard_engine
    zst, nz = eng.layout.zstarts_h, eng.nz
    rs = np.random.RandomState(6)
    y = 0.5 + rs.randn(nz)
    want = np.clip(oracle_fit(orc, y, zst), 0.0, 1.0)
    dev = lambda: torch.from_numpy(y.copy()).cuda()
    monkeypatch.setenv('BSLS_ISO', 'exact')
    pe = eng.proj(dev()).cpu().numpy()
    parity('iso_fast/surface/proj/exact_bits', nbits(pe, want), 0.0)
    monkeypatch.setenv('BSLS_ISO', 'fast')
    pf = eng.proj(dev()).cpu().numpy()
    parity('iso_fast/surface/proj/fast', tier1(pf, want), TOL)
    assert nbits(pf, pe) > 0, 'BSLS_ISO=fast ran the exact kernel'
    monkeypatch.delenv('BSLS_ISO')
    x = dev(); BlockProj(zst, nz, kind='pava', fast=True)(x)
    parity('iso_fast/surface/blockproj/fast', tier1(x.cpu().numpy(), want), TOL)
    parity('iso_fast/surface/blockproj/fast_is_multi_fast',
           nbits(x.cpu().numpy(), np.clip(multi_fast(y, zst), 0.0, 1.0)), 0.0)
    x = dev(); BlockProj(zst, nz, kind='pava')(x)
    parity('iso_fast/surface/blockproj/default_exact_bits', nbits(x.cpu().numpy(), want), 0.0)
    bp = BlockProj(zst, nz, kind='pava')
    monkeypatch.setenv('BSLS_ISO', 'fast')                 # fast=None: resolved per call
    x = dev(); bp(x)
    parity('iso_fast/surface/blockproj/env_fast', tier1(x.cpu().numpy(), want), TOL)
    assert nbits(x.cpu().numpy(), want) > 0


def test_bb_closure_run_fast_against_exact(cuda, golden, parity, monkeypatch):
    """BB.solve over a fixed-order BBEngine's closures (f, nabla_f, proj) on
    the first tests/fast problem of plugins.npz, 20 iterations, every iterate
    under BSLS_ISO=fast within 1e-12 per element of the same run under exact
    (the fixed-order engine repeats itself bit for bit, so the whole difference
    is the projection's).  Measured first, on MI355X: the exact run repeats
    with spread 0, fast against exact grows from 6e-18 at iterate 1 to at most
    3.3e-16 by iterate 20, so the run keeps its 20 iterations
    (profiles/iso_fast_parity.jsonl)."""
    import torch
    import BB
    import solvers
    from bsls_utils import particular_x0, x2z
    from device import BBEngine
    G = golden('plugins.npz')
    A = sps.csr_matrix((G['grad8_A_data'], G['grad8_A_indices'], G['grad8_A_indptr']),
                       shape=tuple(G['grad8_A_shape']))
    b, sizes = G['grad8_b'], G['grad8_block_sizes']
    eng = BBEngine(A, b, sizes, deterministic=True)
    z0 = torch.from_numpy(x2z(particular_x0(sizes), sizes)).cuda()

    def run(mode):
        monkeypatch.setenv('BSLS_ISO', mode)
        rec = {}

        def log(i, s, dt):
            rec[i] = s.detach().cpu().numpy().copy()
            return 0.0
        BB.solve(z0.clone(), eng.f, eng.nabla_f, solvers.stopping, record_every=1, proj=eng.proj,
                 log=log, options={'max_iter': 20, 'verbose': 0, 'opt_tol': 1e-30})
        return rec
    ex, ex2, fa = run('exact'), run('exact'), run('fast')
    assert sorted(fa) == sorted(ex) == list(range(21))
    spread = max(tier1(ex2[i], ex[i]) for i in ex)
    errs = [tier1(fa[i], ex[i]) for i in range(21)]
    print('exact run-to-run spread %.3e; fast vs exact per iterate: %s'
          % (spread, ' '.join('%.1e' % e for e in errs)))
    parity('iso_fast/surface/bb20/exact_rerun', spread, 0.0)
    for i, e in enumerate(errs):
        parity('iso_fast/surface/bb20/iter%d' % i, e, TOL)
