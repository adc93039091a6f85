"""The block structure of x and z on the device, what the z-space engines
derive from it on the host (the particular x0, the two-routes check) and the
isotonic pack plan of a layout with its cache."""
import os

import numpy as np

import _native
from _native import check, ptr, stream_handle
from dev_images import _torch


def need_two_routes(block_sizes):
    """The block sizes as an int64 vector; ValueError unless every block has
    at least 2 routes: a one-route block has no z coordinate, and the
    reference's projection asserts on it too (strictly increasing z-starts,
    c_extensions.pyx:78).  Pure host."""
    sizes = np.asarray(block_sizes, dtype=np.int64)
    if sizes.ndim != 1 or sizes.size == 0 or np.any(sizes < 2):
        raise ValueError('every block needs at least 2 routes')
    return sizes


def particular_x0(sizes, on_device=False):
    """particular_x0 (bsls_utils.py:327-328): 1 at each block's last entry, as
    a host vector, or formed on the device (zeros, then the ones scattered)."""
    last = np.cumsum(sizes) - 1
    if on_device:
        torch = _torch()
        x0 = torch.zeros(int(np.sum(sizes)), dtype=torch.float64, device='cuda')
        x0[torch.from_numpy(last).cuda()] = 1.0
        return x0
    x0 = np.zeros(int(np.sum(sizes)))
    x0[last] = 1.0
    return x0


def positive_sizes(block_sizes):
    """The block sizes as an int64 vector; ValueError unless it is a non-empty
    vector of sizes >= 1.  Pure host."""
    bs = np.asarray(block_sizes, dtype=np.int64)
    if bs.ndim != 1 or bs.size == 0 or np.any(bs < 1):
        raise ValueError('block_sizes must be positive')
    return bs


class BlockLayout:
    """Block structure of x (sizes k_b) and of z (sizes k_b - 1), on device."""

    def __init__(self, block_sizes):
        torch = _torch()
        self.sizes = bs = positive_sizes(block_sizes)
        self.p = int(bs.size)
        self.n = int(bs.sum())
        self.nz = self.n - self.p
        self.xstarts_h = np.concatenate(([0], np.cumsum(bs)[:-1])).astype(np.int64)
        self.zstarts_h = self.xstarts_h - np.arange(self.p, dtype=np.int64)
        xz = np.arange(self.n, dtype=np.int64)
        xz -= np.repeat(np.arange(self.p, dtype=np.int64), bs)
        xz[np.cumsum(bs) - 1] = -1
        self.xstarts = torch.from_numpy(self.xstarts_h).cuda()
        self.zstarts = torch.from_numpy(self.zstarts_h).cuda()
        self.xz = torch.from_numpy(xz.astype(np.int32)).cuda()
        self.max_block = int(bs.max())
        self.max_zblock = self.max_block - 1
        self._packs = None

    def packs(self):
        """K3 packs (csrc/bb.hip): consecutive whole z-blocks with <= 64 z entries
        for one wave, or a single longer block.  Host-planned once
        (bsls_isotonic_pack_plan over the z-block starts; every z-block holds
        >= 1 entry)."""
        if self._packs is None:
            torch = _torch()
            P = _native.pack_plan(self.zstarts_h, self.nz)
            b0 = np.searchsorted(self.zstarts_h, P['start']).astype(np.int64)
            self._packs = dict(
                z0=torch.from_numpy(P['start']).cuda(),
                b0=torch.from_numpy(b0).cuda(),
                mask=torch.from_numpy(P['mask']).cuda(),
                len=torch.from_numpy(P['len']).cuda(),
                n=int(P['start'].shape[0]))
        return self._packs

    def iso_plan(self):
        """The z-layout's IsoPlan (PAVA v1 over the z-blocks, BBEngine.proj),
        kept by the layout: the content-keyed cache hashes the whole start
        array (C3: 400 KB, ~0.3 ms a call -- most of an LBFGS.solve iteration,
        whose line search projects ~20 times)."""
        plan = getattr(self, '_iso', None)
        if plan is None or getattr(plan, 'device', None) != _cur_dev():
            plan = self._iso = iso_plan(self.zstarts_h, self.nz)
        return plan


def iso_mode(fast=None):
    """True for the prefix-sum PAVA (bsls_isotonic_packs_fast / _multi_fast,
    the 1e-12 contract), False for the bit-identical one.  fast=None reads
    BSLS_ISO -- 'exact' (the default) or 'fast' -- per call, so a test or a
    caller can switch; True / False override it.  Needs no GPU."""
    if fast is not None:
        return bool(fast)
    mode = os.environ.get('BSLS_ISO', 'exact')
    if mode not in ('fast', 'exact'):
        raise ValueError('BSLS_ISO must be fast or exact, not %r' % mode)
    return mode == 'fast'


class IsoPlan:
    """A block layout's pack plan on the device (bsls_isotonic_pack_plan /
    bsls_isotonic_packs): isotonic_regression_multi_c's variant-1 call
    (weight=None, update=1) in one launch, planned once per layout."""

    def __init__(self, starts, n):
        torch = _torch()
        L = _native.lib()
        P = _native.pack_plan(starts, n)
        self.device = _cur_dev()                      # the plan's arrays live there
        self.n = int(n)
        self.npacks = int(P['start'].shape[0])
        self.nlong = int(P['longs'].shape[0])
        self.host = P
        self.start = torch.from_numpy(P['start']).cuda()
        self.mask = torch.from_numpy(P['mask']).cuda()
        self.len = torch.from_numpy(P['len']).cuda()
        self.longs = torch.from_numpy(P['longs'] if self.nlong else np.zeros(1, np.int32)).cuda()
        self.work = (torch.zeros(L.bsls_isotonic_workspace_size(self.n), dtype=torch.uint8,
                                 device='cuda') if self.nlong else None)

    def apply(self, y, stream=None, fast=None):
        """PAVA v1 (expanded) of every block of y[:n], in place: bit-identical
        to the reference, or the prefix-sum form within 1e-12 (iso_mode(fast):
        BSLS_ISO read per call when fast is None)."""
        name = 'bsls_isotonic_packs_fast' if iso_mode(fast) else 'bsls_isotonic_packs'
        L = _native.lib()
        if y.device.index != self.device:
            raise ValueError('IsoPlan built on cuda:%d applied to a tensor on %s'
                             % (self.device, y.device))
        check(getattr(L, name)(ptr(y), ptr(self.start), ptr(self.mask), ptr(self.len),
                               self.npacks, ptr(self.longs), self.nlong, self.n,
                               ptr(self.work), self.work.numel() if self.work is not None
                               else 0, stream_handle(stream)), name)
        return y


_iso_plans = {}


def _cur_dev():
    """Index of the current GPU (-1 without one: host-only tests of the cache)."""
    torch = _torch()
    return torch.cuda.current_device() if torch.cuda.is_available() else -1


def iso_plan(starts_h, n):
    """IsoPlan of a host block-start array, cached by content (a few layouts):
    an entry matches when its own copy of the starts equals these (a compare
    of the arrays, ~30 us at 50k blocks -- hashing them took ~0.5-1 ms a
    call, more than the projection it planned)."""
    st = np.ascontiguousarray(starts_h, dtype=np.int64)
    n = int(n)
    dev = _cur_dev()                         # a plan's arrays belong to one GPU
    for key, (ref, plan) in _iso_plans.items():
        if key[:3] == (st.shape[0], n, dev) and (ref is st or np.array_equal(ref, st)):
            return plan
    if len(_iso_plans) >= 8:
        _iso_plans.pop(next(iter(_iso_plans)))
    plan = IsoPlan(st, n)
    # keyed by (count, n) plus insertion order; the copy guards against a
    # caller that changes its array in place later
    k = (st.shape[0], n, dev)
    while k in _iso_plans:
        k = k + (len(_iso_plans),)
    _iso_plans[k] = (st.copy(), plan)
    return plan
