"""Host side of the fast standalone PAVA (bsls_isotonic_packs_fast /
bsls_isotonic_multi_fast, BSLS_ISO): the ABI, the argument checks that come
before any launch, the mode switch, and the NumPy model of the wave routine
(tools/iso_fast_model.py) against the oracle.  No GPU."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = ('bsls_isotonic_packs_fast', 'bsls_isotonic_multi_fast')


@pytest.fixture(scope='module')
def native():
    import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


@pytest.fixture(scope='module')
def model():
    spec = importlib.util.spec_from_file_location(
        'iso_fast_model', os.path.join(ROOT, 'tools', 'iso_fast_model.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_and_library_exports_the_fast_entries(native):
    syms = native.declared_symbols()
    L = native.load()
    out = subprocess.check_output(['nm', '-D', '--defined-only', native.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    for s in FAST:
        assert s in syms
        assert hasattr(L, s)
        assert s in exported
    text = open(native.HEADER).read()
    assert text.count('isotonic_regression.h:13-58') >= 2     # both entries cite the reference


def test_fast_entries_reject_bad_arguments_before_any_launch(native):
    L = native.load()
    E_ARG, E_WS = native.BSLS_E_ARG, native.BSLS_E_WORKSPACE
    # never dereferenced: every call below returns before a launch
    p = ctypes.c_void_p(0x1000)
    nul = ctypes.c_void_p(0)
    packs = L.bsls_isotonic_packs_fast
    ok = dict(y=p, st=p, mk=p, ln=p, npacks=4, longs=p, nlong=0, n=100, work=nul, wb=0)

    def call(**kw):
        a = dict(ok, **kw)
        return packs(a['y'], a['st'], a['mk'], a['ln'], a['npacks'], a['longs'], a['nlong'],
                     a['n'], a['work'], a['wb'], nul)
    for k in ('y', 'st', 'mk', 'ln'):
        assert call(**{k: nul}) == E_ARG, k
    assert call(npacks=0) == E_ARG
    assert call(npacks=-3) == E_ARG
    assert call(n=0) == E_ARG
    assert call(n=-1) == E_ARG
    assert call(nlong=-1) == E_ARG
    need = L.bsls_isotonic_workspace_size(100)
    assert call(nlong=1, work=p, wb=need - 1) == E_WS
    assert call(nlong=1, work=nul, wb=need) == E_WS
    assert call(nlong=1, longs=nul, work=p, wb=need) == E_WS

    multi = L.bsls_isotonic_multi_fast
    assert multi(nul, p, 3, 100, 10, p, need, nul) == E_ARG
    assert multi(p, nul, 3, 100, 10, p, need, nul) == E_ARG
    assert multi(p, p, 0, 100, 10, p, need, nul) == E_ARG
    assert multi(p, p, 3, 0, 10, p, need, nul) == E_ARG
    assert multi(p, p, 3, -5, 10, p, need, nul) == E_ARG
    assert multi(p, p, 3, 100, 10, p, need - 1, nul) == E_WS
    assert multi(p, p, 3, 100, 10, nul, need, nul) == E_WS
    # the exact twins answer the same
    assert L.bsls_isotonic_packs(p, p, p, p, 0, p, 0, 100, nul, 0, nul) == E_ARG
    assert L.bsls_isotonic_packs(p, p, p, p, 4, p, 1, 100, p, need - 1, nul) == E_WS


def test_iso_mode_reads_the_environment_per_call(monkeypatch):
    import device
    monkeypatch.delenv('BSLS_ISO', raising=False)
    assert device.iso_mode() is False
    monkeypatch.setenv('BSLS_ISO', 'fast')
    assert device.iso_mode() is True
    monkeypatch.setenv('BSLS_ISO', 'exact')
    assert device.iso_mode() is False
    assert device.iso_mode(True) is True              # the keyword overrides
    monkeypatch.setenv('BSLS_ISO', 'fast')
    assert device.iso_mode(False) is False
    monkeypatch.setenv('BSLS_ISO', 'quick')
    with pytest.raises(ValueError, match='BSLS_ISO must be fast or exact, not'):
        device.iso_mode()


def test_cpu_path_ignores_but_validates_bsls_iso(monkeypatch, orc):
    from c_extensions import c_extensions as cx
    monkeypatch.setenv('BSLS_DEVICE', 'cpu')
    rs = np.random.RandomState(3)
    y = rs.randn(200)
    starts = np.array([0, 5, 70, 71, 150], dtype=np.int64)
    ref = y.copy()
    orc.isotonic_regression_multi_c(ref, starts)
    monkeypatch.setenv('BSLS_ISO', 'fast')
    got = y.copy()
    cx.isotonic_regression_multi_c(got, starts)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))
    monkeypatch.setenv('BSLS_ISO', 'quick')
    with pytest.raises(ValueError, match='BSLS_ISO'):
        cx.isotonic_regression_multi_c(y.copy(), starts)


def test_model_meets_both_tiers_on_the_seven_families(model, orc, native):
    """The kernel's rule as built -- scan order, cross-multiplied test,
    length-1 rule, closing check on the means -- against the oracle's v1:
    tier 1 (1e-12 max(1, |ref|)) on the first six families, tier 2 (1e-12
    max(1, max |y| of the block)) on all seven, monotone output on all.
    Measured maxima: profiles/iso_fast_model.txt."""
    rs = np.random.RandomState(17)
    for k, name in enumerate(model.FAMILIES):
        starts, n = model.layout(rs, 2000)
        y = model.family(name, rs, starts, n)
        ref = y.copy()
        orc.isotonic_regression_multi_c(ref, starts)
        got, npass, nclose = model.fit(y, starts, with_counts=True)
        t1, t2 = model.tiers(got, ref, y, starts)
        print('%-34s tier1 %.2e tier2 %.2e passes %.1f/%d' % (name, t1, t2, npass.mean(),
                                                             npass.max()))
        if k < 6:
            assert t1 <= 1e-12, (name, t1)
        assert t2 <= 1e-12, (name, t2)
        assert model.monotone(got, starts), name
        assert npass.max() <= 64


def test_model_returns_sorted_input_with_ties_bit_for_bit(model):
    rs = np.random.RandomState(17)
    starts, n = model.layout(rs, 2000)
    first = 5
    starts = starts + first
    n += first
    y = np.round(rs.randn(n), 1)
    y[rs.rand(n) < 0.1] = -0.0
    y[rs.rand(n) < 0.1] = 0.0
    for s, e in zip(starts, np.append(starts[1:], n)):
        y[s:e] = np.sort(y[s:e])                      # -0.0 and 0.0 compare equal: both orders occur
    got = model.fit(y, starts)
    assert np.array_equal(got.view(np.int64), y.view(np.int64))
