"""Host-only tests of the device layer's split: `device` as the public face of
the dev_* modules, the BB host loop BBEngine.solve and BatchBB.solve share,
and BBEngine's refusals before the device is touched.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   'block-simplex-least-squares_amd')

# what `device` exported before the split, by home module
FACADE = {
    'dev_images': ['DeviceCSR', 'even_bounds', 'chunk_plan', 'PanelOverflow', 'build_panels',
                   'panels_matvec', 'scaled_incidence_scale', 'DevicePanels', 'tile_plan',
                   'spmv_format', 'tiles_matvec', '_dealt_matvec', 'value_codec', 'self_bytes',
                   'DeviceTiles', 'panel_rows', 'k1_plan'],
    'dev_lsq': ['DeviceLSQ', 'lsq_operator', 'XBBEngine'],
    'dev_blocks': ['iso_mode', 'IsoPlan', 'iso_plan', '_iso_plans', '_cur_dev', 'BlockLayout'],
    'dev_bb': ['LineSearch', 'fixed_sum_bounds', 'fixed_sums_check', 'row_weights_check',
               'fixed_plan_fits', 'BBEngine'],
    'dev_batch': ['batch_width', 'batch_groups', '_batch_columns', 'BatchBB'],
}


def test_facade_names():
    """Every name `device` exported is still its attribute, and is the object
    of its home module."""
    import importlib
    import device
    assert sum(len(v) for v in FACADE.values()) == 36
    for mod, names in FACADE.items():
        home = importlib.import_module(mod)
        for name in names:
            assert getattr(device, name) is getattr(home, name), name
    import distributed
    import dev_images
    assert distributed.row_parts is dev_images.row_parts


def test_import_device_without_torch():
    """`import device` in a fresh interpreter does not import torch."""
    code = ('import sys; sys.path.insert(0, %r); import device; '
            'assert "torch" not in sys.modules, "torch was imported"' % PKG)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ---- the shared BB host loop -------------------------------------------------
RECORD, POLL = 5, 2


class StubP:
    def __init__(self, max_iter):
        self.max_iter = max_iter


class StubEngine:
    """What solve() needs of an engine, on the host: problem j stops at
    iteration stops[j][0] with reason stops[j][1] and is frozen there (its
    scalars keep that iteration and its z buffer), as the device does it.
    z[k] holds the value k, so a logged state tells the buffer it came from."""

    def __init__(self, stops, max_iter=1000):
        import torch
        self.stops = stops
        self.R = len(stops)
        self.P = StubP(max_iter)
        self.nz = 2
        self.z = [torch.full((self.R, 2), float(k), dtype=torch.float64) for k in range(2)]
        self.i = 0
        self.calls = []
        self.order = []
        self.stop_reasons = [None] * self.R
        self.iterations = [None] * self.R

    def prologue(self):
        self.order.append('prologue')

    def iterate(self, first, count):
        assert first == self.i + 1 and count >= 1
        self.calls.append((first, count))
        self.i += count

    def _rows(self):
        import _native as N
        S = np.zeros((self.R, N.S_COUNT))
        for j, (at, reason) in enumerate(self.stops):
            if self.i >= at:
                S[j, N.S_STOP], S[j, N.S_ITER], S[j, N.S_ZBUF] = reason, at, at & 1
        return S


class StubBB(StubEngine):            # BBEngine's side of the interface
    def set_z0(self, z0):
        self.z0 = z0

    def scalars(self):
        return self._rows()[0]

    def current_z(self, zbuf):
        return self.z[int(zbuf)][0]


class StubBatch(StubEngine):         # BatchBB's
    def set_z0(self, z0):
        assert z0 is None

    def scalars(self):
        return self._rows()

    def current_z(self, j, zbuf):
        return self.z[int(zbuf)][j]


def reference_logs(stop_at, no_change):
    """Where python/BB.py's solve logs a run that leaves its loop at iteration
    stop_at: the initial state (BB.py:10), every multiple of record_every its
    loop body reaches the end of (BB.py:40-41; the no-change break at
    BB.py:22-24 leaves before that), and the final state (BB.py:44)."""
    done = stop_at - 1 if no_change else stop_at
    return [0] + [i for i in range(1, done + 1) if i % RECORD == 0] + [stop_at]


def check_windows(calls, last, record_every=RECORD):
    """The iterate calls cover 1..last exactly once, in order, and none runs
    past a record boundary."""
    at = 0
    for first, count in calls:
        assert first == at + 1
        at += count
        assert (first - 1) // record_every == (at - 1) // record_every, (first, count)
    assert calls[-1][0] <= last <= at
    return at


def run_one(stop_at, reason, poll=POLL, max_iter=1000, to_host=True):
    from device import BBEngine
    eng = StubBB([(stop_at, reason)], max_iter)
    logs = []

    def log(i, z, dt):
        logs.append((i, float(z[0]), type(z)))
        return 0.0
    out = BBEngine.solve(eng, log=log, record_every=RECORD, poll=poll, to_host=to_host)
    assert eng.order == ['prologue']
    assert (eng.iterations, eng.stop_reason) == (stop_at, reason)
    assert float(out[0]) == stop_at & 1 and out is not None
    # every logged state is the z buffer of its iteration's parity
    assert all(v == (i & 1) for i, v, _ in logs[1:])
    return eng, logs


@pytest.mark.parametrize('stop_at, reason, poll, max_iter', [
    (10, 'STOP_GRAD', POLL, 1000),       # on a boundary: the record and the final log at 10
    (10, 'STOP_NOCHANGE', POLL, 1000),   # no change: the final log only
    (7, 'STOP_GRAD', POLL, 1000),        # inside a record interval, at a window's end
    (6, 'STOP_GRAD', POLL, 1000),        # inside a window: seen at 7, logged as 6 from z[0]
    (8, 'STOP_MAXITER', POLL, 8),        # max_iter off a boundary
    (12, 'STOP_GRAD', 50, 1000),         # poll > record_every: windows still end at boundaries
])
def test_poll_loop_one_problem(stop_at, reason, poll, max_iter, capsys):
    import _native as N
    reason = getattr(N, reason)
    eng, logs = run_one(stop_at, reason, poll, max_iter)
    no_change = reason == N.STOP_NOCHANGE
    assert [i for i, _, _ in logs] == reference_logs(stop_at, no_change)
    end = check_windows(eng.calls, stop_at)
    assert end <= max_iter
    assert all(c <= poll for _, c in eng.calls)
    if poll > RECORD:
        assert eng.calls == [(1, 5), (6, 5), (11, 5)]
    printed = capsys.readouterr().out
    assert ('Exiting... no change in gradient' in printed) == no_change
    assert all(t is np.ndarray for _, _, t in logs[1:])


def test_poll_loop_device_states():
    """to_host=False: the logged states are device-side clones, no host copy."""
    import torch
    import _native as N
    eng, logs = run_one(10, N.STOP_GRAD, to_host=False)
    assert [i for i, _, _ in logs] == [0, 5, 10, 10]
    assert all(t is torch.Tensor for _, _, t in logs[1:])


def test_poll_loop_three_problems(capsys):
    """R = 3 with stops at 4, 10 (no change) and 10: each problem logs where
    BB.solve would log it alone, and a stopped problem is frozen."""
    import _native as N
    from device import BatchBB
    stops = [(4, N.STOP_GRAD), (10, N.STOP_NOCHANGE), (10, N.STOP_GRAD)]
    eng = StubBatch(stops)
    logs = [[] for _ in stops]

    def log(j, i, z, dt):
        assert isinstance(z, np.ndarray) and float(z[0]) == (i & 1 if i else 0)
        logs[j].append(i)
        return 0.0
    out = BatchBB.solve(eng, log=log, record_every=RECORD, poll=POLL)
    for j, (at, reason) in enumerate(stops):
        assert logs[j] == reference_logs(at, reason == N.STOP_NOCHANGE), j
        assert float(out[j][0]) == at & 1
    assert logs[0] == [0, 4, ]                     # nothing after its stop at 4
    assert eng.iterations == [4, 10, 10]
    assert eng.stop_reasons == [r for _, r in stops]
    assert check_windows(eng.calls, 10) == 10
    assert capsys.readouterr().out.count('Exiting... no change in gradient') == 1


def test_poll_loop_warning(capsys):
    """The reference's BB-step warning (BB.py:27-28), once per new warning."""
    import _native as N
    from dev_bb import poll_solve
    eng = StubBB([(6, N.STOP_GRAD)])
    rows = eng._rows

    def scalars():
        S = rows()[0]
        S[N.S_WARN], S[N.S_T] = (1 if eng.i >= 4 else 0), 1e-11
        return S
    eng.scalars = scalars
    poll_solve(eng, 1, 1000, RECORD, POLL, lambda j, i, z, dt: 0.0, first=lambda j: None,
               state=lambda j, zb: None, stopped=lambda j, reason, i: None)
    assert capsys.readouterr().out.count('BB update is having some trouble') == 1


# ---- BBEngine refuses before the device is touched ------------------------------
def test_bbengine_refusals_touch_no_device(monkeypatch):
    import _native
    import dev_bb
    import dev_blocks
    from device import BBEngine
    for env in ('BSLS_FIXED_SUMS', 'BSLS_TILE_LAYOUT', 'BSLS_SPMV_FORMAT', 'BSLS_K1_ATOMIC',
                'BSLS_K3_WARM', 'BSLS_K3_MERGE'):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(_native, 'lib', lambda: pytest.fail('the library was touched'))
    for mod in (dev_bb, dev_blocks):
        monkeypatch.setattr(mod, '_torch', lambda: pytest.fail('torch was touched'))
    sizes = [2, 3, 2, 4]
    m, n = 6, sum(sizes)
    A = sps.random(m, n, density=0.5, random_state=np.random.RandomState(0), format='csr')
    b = np.ones(m)
    w = np.ones(m)
    cases = [
        (dict(fixed_sums=True, deterministic=True), 'two ways to the same end'),
        (dict(fixed_sums=True, fmt='panels'), "fmt='panels' has none"),
        (dict(fixed_sums=True, link_parts=2), 'does not cover link parts'),
        (dict(fixed_sums=True, row_weights=w), 'not covered by fixed_sums'),
        (dict(row_weights=np.ones(m + 1)), 'expected one per row of A'),
        (dict(row_weights=-w), 'must be non-negative'),
    ]
    for kw, text in cases:
        with pytest.raises(ValueError, match=text):
            BBEngine(A, b, sizes, **kw)
    with pytest.raises(ValueError, match='every block needs at least 2 routes'):
        BBEngine(A, b, [2, 3, 1, 5])
    with pytest.raises(ValueError, match='A has 11 columns but the blocks cover 12'):
        BBEngine(A, b, [2, 3, 2, 5])
    # the environment's switches are refused on the same footing
    monkeypatch.setenv('BSLS_K1_ATOMIC', '1')
    with pytest.raises(ValueError, match='BSLS_K1_ATOMIC=1'):
        BBEngine(A, b, sizes, fixed_sums=True)
