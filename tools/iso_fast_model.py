"""NumPy model of csrc/pava_fast.hpp (pava_fast_wave), lane for lane: the
block-segmented prefix sum in the kernel's DPP order (row_shr 1/2/4/8 inside
rows of 16 lanes, then row_bcast 15 and 31), the cross-multiplied test of every
run head against the previous run, the length-1 rule (a run of one element is
its raw value, never a prefix difference) and the closing check on the divided
means.  All packs of a layout advance together, one array row per pack; the
packs are the planned ones (bsls_isotonic_pack_plan, host only), so the model
needs no GPU.  tests/test_iso_fast_host.py holds it to the two accuracy tiers
against the oracle; run as a script it prints the measured maxima
(profiles/iso_fast_model.txt).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 64
LANES = np.arange(W)


def scan(y, B, L):
    """pi, pe of the kernel: inclusive / exclusive prefix sums inside blocks.
    y [P, 64] (zero from lane L on), B [P, 64] bool block starts (B[:, 0])."""
    b = np.maximum.accumulate(np.where(B, LANES, -1), axis=1)
    s = np.where(LANES[None, :] < L[:, None], y, 0.0)
    for k in (1, 2, 4, 8):                      # row_shr:k, zero from outside the row
        u = np.zeros_like(s)
        u[:, k:] = s[:, :-k]
        u[:, (LANES % 16) < k] = 0.0
        s = s + np.where(LANES - k >= b, u, 0.0)
    u = np.zeros_like(s)                        # row_bcast:15 -> rows 1, 3
    for r in (1, 3):
        u[:, 16 * r:16 * r + 16] = s[:, 16 * r - 1:16 * r]
    row0 = (LANES & ~15) - 1
    s = s + np.where(((LANES & 16) != 0) & (b <= row0), u, 0.0)
    u = np.zeros_like(s)                        # row_bcast:31 -> rows 2, 3
    u[:, 32:] = s[:, 31:32]
    s = s + np.where((LANES >= 32) & (b <= 31), u, 0.0)
    sprev = np.zeros_like(s)
    sprev[:, 1:] = s[:, :-1]
    return s, np.where(LANES == b, 0.0, sprev)


def _take(a, idx):
    return np.take_along_axis(a, np.clip(idx, 0, W - 1), axis=1)


def wave(y, B, L):
    """pava_fast_wave on every row: (fit [P, 64], cross passes per pack incl.
    the one that removes nothing, closing checks per pack)."""
    y = np.where(LANES[None, :] < L[:, None], y, 0.0)
    B = B.copy()
    B[:, 0] = True
    pi, pe = scan(y, B, L)
    yprev = np.zeros_like(y)
    yprev[:, 1:] = y[:, :-1]
    H = LANES[None, :] < L[:, None]
    m = y.copy()
    live = np.ones(y.shape[0], bool)
    npass = np.zeros(y.shape[0], np.int64)
    nclose = np.zeros(y.shape[0], np.int64)
    for _ in range(W):
        if not live.any():
            break
        hidx = np.where(H, LANES, -1)
        h = np.maximum.accumulate(hidx, axis=1)                 # own run's head
        p = np.zeros_like(h)
        p[:, 1:] = np.maximum(h[:, :-1], 0)                     # previous head below
        nxt = np.full_like(h, W)
        nxt[:, :-1] = np.minimum.accumulate(np.where(H, LANES, W)[:, ::-1], axis=1)[:, ::-1][:, 1:]
        e = np.where(nxt < W, nxt - 1, L[:, None] - 1)
        lr, lp = e - LANES + 1, LANES - p
        sr = np.where(lr == 1, y, _take(pi, e) - pe)
        sp = np.where(lp == 1, yprev, pe - _take(pe, p))
        with np.errstate(invalid='ignore', over='ignore'):
            V = (sr * lp.astype(np.float64) < sp * lr.astype(np.float64)) & H & ~B
        V &= live[:, None]
        npass += live
        close = live & ~V.any(axis=1)
        if close.any():
            ln = e - h + 1
            sm = np.where(ln == 1, y, _take(pi, e) - _take(pe, h))
            with np.errstate(invalid='ignore', over='ignore'):
                mm = sm / ln.astype(np.float64)
            mp = np.zeros_like(mm)
            mp[:, 1:] = mm[:, :-1]
            with np.errstate(invalid='ignore'):
                V2 = (mm < mp) & H & ~B & close[:, None]
            m = np.where(close[:, None], mm, m)
            nclose += close
            live &= ~(close & ~V2.any(axis=1))
            V |= V2
        H &= ~V
    return m, npass, nclose


def fit(y, starts, with_counts=False):
    """The fast isotonic fit of y over blocks `starts` (every block <= 64
    elements) through the planned packs, as bsls_isotonic_packs_fast."""
    sys.path.insert(0, os.path.join(ROOT, 'block-simplex-least-squares_amd'))
    import _native
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    P = _native.pack_plan(starts, n)
    if P['longs'].shape[0]:
        raise ValueError('the model covers blocks of at most 64 elements')
    L = P['len'].astype(np.int64)
    idx = P['start'][:, None] + LANES[None, :]
    act = LANES[None, :] < L[:, None]
    Y = np.where(act, y[np.minimum(idx, n - 1)], 0.0)
    B = ((P['mask'].astype(np.uint64)[:, None] >> LANES.astype(np.uint64)[None, :]) & 1) != 0
    m, npass, nclose = wave(Y, B, L)
    out = y.copy()
    out[idx[act]] = m[act]
    return (out, npass, nclose) if with_counts else out


FAMILIES = ('randn', '5*randn', 'U[0,1)', 'rounded randn (ties)', '-arange + 0.25*randn',
            'sorted U[0,1) - 1e-3*randn', 'randn*10^U(-6,6) (wide range)')


def layout(rs, nblocks):
    sizes = rs.randint(1, 65, nblocks)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    return starts, int(sizes.sum())


def family(name, rs, starts, n):
    if name == 'randn':
        return rs.randn(n)
    if name == '5*randn':
        return 5.0 * rs.randn(n)
    if name == 'U[0,1)':
        return rs.rand(n)
    if name == 'rounded randn (ties)':
        return np.round(rs.randn(n), 0)
    if name == '-arange + 0.25*randn':
        return -np.arange(n, dtype=np.float64) + 0.25 * rs.randn(n)
    if name == 'sorted U[0,1) - 1e-3*randn':
        y = rs.rand(n)
        for s, e in zip(starts, np.append(starts[1:], n)):
            y[s:e] = np.sort(y[s:e])
        return y - 1e-3 * rs.randn(n)
    if name == 'randn*10^U(-6,6) (wide range)':
        return rs.randn(n) * 10.0 ** rs.uniform(-6, 6, n)
    raise KeyError(name)


def tiers(got, ref, y, starts):
    """(tier 1, tier 2): max |d| / max(1, |ref|) and max |d| / max(1, max |y|
    over the element's block)."""
    n = y.shape[0]
    d = np.abs(got - ref)
    bmax = np.maximum.reduceat(np.abs(y[starts[0]:]), starts - starts[0])
    scale = np.ones(n)
    scale[starts[0]:] = np.repeat(bmax, np.diff(np.append(starts, n)))
    return (float(np.max(d / np.maximum(1.0, np.abs(ref)))),
            float(np.max(d / np.maximum(1.0, scale))))


def monotone(out, starts):
    """np.diff(out) >= 0 inside every block."""
    ok = np.diff(out) >= 0
    ok[starts[1:] - 1] = True
    return bool(np.all(ok[starts[0]:]))


def main():
    sys.path.insert(0, ROOT)
    from oracle import oracle as orc
    orc.build()
    rs = np.random.RandomState(17)
    print('pava_fast_wave, NumPy model vs the oracle PAVA v1; 3000 random blocks of 1-64, seed 17')
    print('%-34s %10s %10s  %s' % ('input', 'tier 1', 'tier 2', 'passes mean/max + closing mean/max'))
    for name in FAMILIES:
        starts, n = layout(rs, 3000)
        y = family(name, rs, starts, n)
        ref = y.copy()
        orc.isotonic_regression_multi_c(ref, starts)
        got, npass, nclose = fit(y, starts, with_counts=True)
        t1, t2 = tiers(got, ref, y, starts)
        print('%-34s %10.2e %10.2e  %.1f / %d + %.2f / %d%s' % (
            name, t1, t2, npass.mean(), npass.max(), nclose.mean(), nclose.max(),
            '' if monotone(got, starts) else '  NOT MONOTONE'))


if __name__ == '__main__':
    main()
