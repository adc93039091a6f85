"""The batched BB engine's host side (device.batch_width / batch_groups,
cross_validation.kfold(batch=), main.py --cv-batch, the bsls_bbm_* C ABI):
everything that runs before a device is touched.  No GPU needed."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('bsls_bbm_workspace_size', 'bsls_bbm_prologue', 'bsls_bbm_iterate', 'bsls_bbm_stage')


@pytest.fixture(scope='module')
def native():
    import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_batch_width():
    from device import batch_width
    assert [batch_width(r) for r in range(1, 9)] == [1, 2, 4, 4, 8, 8, 8, 8]
    for bad in (0, 9, -1, 2.0, None, True):
        with pytest.raises(ValueError):
            batch_width(bad)


def test_batch_groups():
    from device import batch_groups
    assert batch_groups(10) == [5, 5]
    assert batch_groups(8) == [8]
    assert batch_groups(17) == [6, 6, 5]
    assert batch_groups(5, cap=2) == [2, 2, 1]
    assert batch_groups(3, cap=3) == [3]
    assert batch_groups(1) == [1]
    for k in range(1, 40):
        for cap in range(1, 9):
            g = batch_groups(k, cap)
            assert sum(g) == k and max(g) <= cap and max(g) - min(g) <= 1
            assert len(g) == -(-k // cap) and g == sorted(g, reverse=True)
    for bad in ((0, 8), (3, 0), (3, 9)):
        with pytest.raises(ValueError):
            batch_groups(*bad)


@pytest.fixture(scope='module')
def tiny(orc):
    from synthetic import make_shard, add_noise
    sh = make_shard(600, 30, 80, per_col=4, seed=3)
    b = add_noise(sh['Ax'], 0.02, seed=3)
    sizes = np.asarray(sh['block_sizes'])
    return sh['A'], b, orc.particular_x0(sizes), orc.block_sizes_to_N(sizes), sizes


def test_kfold_cpu_ignores_batch(tiny):
    from cross_validation import kfold
    opts = {'max_iter': 5, 'opt_tol': 1e-30}
    a = kfold(*tiny, 3, options=opts, device='cpu')
    b = kfold(*tiny, 3, options=opts, device='cpu', batch=2)
    assert len(a) == len(b) == 3
    for fa, fb in zip(a, b):
        assert set(fa) == set(fb)
        for key in ('iters', 'stop', 'f_train', 'held_out'):
            assert fa[key] == fb[key]
        assert np.array_equal(fa['z'], fb['z'])


def test_kfold_bad_batch_raises_before_torch(tiny):
    """In a fresh interpreter: kfold(batch=0) is refused with torch never imported."""
    code = ('import sys, numpy as np, scipy.sparse as sps\n'
            'sys.path[:0] = [%r, %r]\n'
            'from cross_validation import kfold\n'
            'A = sps.identity(4, format="csr")\n'
            'for bad in (0, 9, 2.5):\n'
            '    try:\n'
            '        kfold(A, np.ones(4), np.ones(4), None, np.array([2, 2]), 2, batch=bad)\n'
            '    except ValueError:\n'
            '        pass\n'
            '    else:\n'
            '        raise SystemExit("accepted %%r" %% (bad,))\n'
            'assert "torch" not in sys.modules\n'
            % (ROOT, os.path.join(ROOT, 'block-simplex-least-squares_amd')))
    subprocess.run([sys.executable, '-c', code], check=True)
    from cross_validation import kfold
    with pytest.raises(ValueError, match='batch'):
        kfold(*tiny, 3, batch=0)
    with pytest.raises(ValueError, match='batch'):
        kfold(*tiny, 3, device='cpu', batch=9)


def test_parser_knows_cv_batch():
    import main
    a = main.parser().parse_args(['--cv', '5', '--cv-batch', '4'])
    assert a.cv == 5 and a.cv_batch == 4
    assert main.parser().parse_args([]).cv_batch is None


def test_main_refuses_cv_batch_without_cv():
    import main
    base = dict(noise=0, file='does-not-exist.mat', log='WARN', init=False, eq='CP', method='BB')
    with pytest.raises(ValueError, match='cv'):
        main.main(args=argparse.Namespace(cv_batch=2, **base))
    with pytest.raises(ValueError, match='cv-batch'):
        main.main(args=argparse.Namespace(cv=3, cv_batch=9, **base))


def test_header_declares_and_library_exports(native):
    syms = native.declared_symbols()
    L = native.load()
    out = subprocess.check_output(['nm', '-D', '--defined-only', native.LIB_PATH]).decode()
    exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    for s in ENTRIES:
        assert s in syms and hasattr(L, s) and s in exported, s
    # sizes and refusals need no device
    assert L.bsls_bbm_workspace_size(1000, 5000, 4000, 8) > L.bsls_bbm_workspace_size(
        1000, 5000, 4000, 1) > 0
    assert L.bsls_bbm_workspace_size(1000, 5000, 4000, 9) == 0
    E = native.BSLS_E_ARG
    assert L.bsls_bbm_prologue(None, None) == E
    P = native.BBMProblem()
    P.m, P.n, P.nblocks, P.nz = 10, 20, 4, 16
    for R, RP in ((0, 1), (9, 8), (3, 2)):
        P.R, P.RP = R, RP
        assert L.bsls_bbm_prologue(P, None) == E
        assert L.bsls_bbm_iterate(P, 1, 1, None) == E
        assert L.bsls_bbm_stage(P, 1, 0, None) == E
    P.R, P.RP = 3, 4
    assert L.bsls_bbm_stage(P, 1, 0, None) == E          # null images
    P.nz = 15
    assert L.bsls_bbm_prologue(P, None) == E             # nz != n - nblocks


def test_struct_layout_matches_header(native, tmp_path):
    C = native.BBMProblem
    names = [f[0] for f in C._fields_]
    src = tmp_path / 'lay.c'
    body = ''.join('printf("%%zu\\n", offsetof(bsls_bbm_problem, %s));' % f for f in names)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bsls_hip.h"\n'
                   'int main(void){printf("%%zu\\n", sizeof(bsls_bbm_problem));%s return 0;}\n'
                   % body)
    exe = tmp_path / 'lay'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                   check=True)
    want = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True,
                                           text=True).stdout.split()]
    got = [ctypes.sizeof(C)] + [getattr(C, f).offset for f in names]
    assert got == want
