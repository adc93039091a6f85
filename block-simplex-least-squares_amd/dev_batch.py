"""Batched BB: R problems in lockstep over one image of A (csrc/bbm.hip)."""
import time

import numpy as np
import scipy.sparse as sps

import _native
from _native import check, stream_handle
from dev_bb import poll_solve, reg_lambda_check, row_weights_check
from dev_blocks import BlockLayout, need_two_routes, particular_x0
from dev_images import _torch


def batch_width(R):
    """The interleave width RP of a batch of R problems: R rounded up to 1, 2,
    4 or 8 (struct bsls_bbm_problem).  ValueError outside 1..8.  Pure host."""
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= 8:
        raise ValueError('a batch holds 1..8 problems (got %r)' % (R,))
    return 1 if R == 1 else 2 if R == 2 else 4 if R <= 4 else 8


def batch_groups(k, cap=8):
    """k problems in the fewest groups of at most `cap`, sizes differing by at
    most one, the larger first: 10 -> [5, 5], 8 -> [8], 17 -> [6, 6, 5].  Pure host."""
    k = int(k)
    batch_width(cap)
    if k < 1:
        raise ValueError('nothing to group (k = %d)' % k)
    g = -(-k // int(cap))
    return [k // g + (1 if i < k % g else 0) for i in range(g)]


def _batch_columns(bs, m):
    """The R right-hand sides as host float64 vectors of length m."""
    if hasattr(bs, 'ndim') and getattr(bs, 'ndim') == 2:
        bs = [np.asarray(bs)[:, j] for j in range(np.asarray(bs).shape[1])]
    cols = [np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1)) for b in bs]
    batch_width(len(cols))
    for j, b in enumerate(cols):
        if b.size != m:
            raise ValueError('b[%d] has %d entries, expected one per row of A (%d)'
                             % (j, b.size, m))
    return cols


class BatchBB:
    """R <= 8 z-space BB problems in lockstep over one CSR image of A and A'
    (bsls_bbm_*, csrc/bbm.hip): the problems share A, the block layout and x0
    and differ in b_j, per-link weights / hold-out mask w_j and z0_j.  Each
    follows BB.solve (python/BB.py:14-42) under solvers.stopping with its own
    step, f, held-out error, exit iteration and stop reason; a stopped problem
    is frozen while the others go on.  x- and link-space vectors are
    interleaved (element i of problem j at [i, j] of an (.., RP) tensor), the
    z-space ones stacked ((RP, nz)).  Every sum runs in a fixed order: a run
    repeats bit for bit."""

    def __init__(self, A, bs, block_sizes, row_weights=None, options=None, x0=None,
                 early_exit=True, reg_lambda=0.0, reg_weights=None):
        # everything that can be refused is refused here, before the device is touched
        if reg_lambda_check(reg_lambda) or reg_weights is not None:
            raise ValueError('the batched engine does not cover a regulariser: BBEngine, one '
                             'problem at a time')
        A = sps.csr_matrix(A)
        self.m = int(A.shape[0])
        cols = _batch_columns(bs, self.m)
        self.R = len(cols)
        self.RP = batch_width(self.R)
        sizes = need_two_routes(block_sizes)
        if A.shape[1] != int(sizes.sum()):
            raise ValueError('A has %d columns but the blocks cover %d'
                             % (A.shape[1], int(sizes.sum())))
        if A.shape[1] >= 2 ** 31 or self.m >= 2 ** 31:
            raise ValueError('row or column count exceeds int32 indices')
        if row_weights is None:
            row_weights = [None] * self.R
        if len(row_weights) != self.R:
            raise ValueError('row_weights has %d entries for %d problems'
                             % (len(row_weights), self.R))
        wts = [row_weights_check(w, self.m) for w in row_weights]
        if x0 is None:
            x0h = particular_x0(sizes)
        else:
            x0h = np.asarray(x0, dtype=np.float64).reshape(-1)
            if x0h.size != A.shape[1]:
                raise ValueError('x0 has %d entries, expected %d' % (x0h.size, A.shape[1]))
        torch = _torch()
        L = _native.lib()
        self.layout = lay = BlockLayout(sizes)
        self.n, self.nz = lay.n, lay.nz
        A.sort_indices()
        AT = A.T.tocsr()
        AT.sort_indices()
        self._Ax0 = A.dot(x0h)                          # target_j = A x0 - b_j (main.py:48)
        f64 = dict(dtype=torch.float64, device='cuda')
        RP, m, n, nz = self.RP, self.m, self.n, self.nz

        def up(a, dt):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
        self.a_img = (up(A.indptr, np.int64), up(A.indices, np.int32), up(A.data, np.float64))
        self.at_img = (up(AT.indptr, np.int64), up(AT.indices, np.int32), up(AT.data, np.float64))
        self.target = torch.zeros(m, RP, **f64)
        self.roww = torch.ones(m, RP, **f64)
        self.weighted = [False] * self.R
        self.zx = up(np.arange(nz, dtype=np.int64)
                     + np.repeat(np.arange(lay.p, dtype=np.int64), sizes - 1), np.int32)
        # the pack plan of the stacked layout: the z-block starts, once per column
        starts = (lay.zstarts_h[None, :] + nz * np.arange(RP, dtype=np.int64)[:, None]).reshape(-1)
        pk = _native.pack_plan(starts, RP * nz)
        self.npacks, self.nlong = int(pk['start'].shape[0]), int(pk['longs'].shape[0])
        self.pk = (up(pk['start'], np.int64), up(pk['mask'], np.int64), up(pk['len'], np.int32),
                   up(pk['longs'] if self.nlong else np.zeros(1), np.int32))
        self.iso_work = (torch.zeros(L.bsls_isotonic_workspace_size(RP * nz), dtype=torch.uint8,
                                     device='cuda') if self.nlong else None)
        self.z = [torch.zeros(RP, nz, **f64) for _ in range(2)]
        self.g = [torch.zeros(RP, nz, **f64) for _ in range(2)]
        self.dz = torch.zeros(RP, nz, **f64)
        self.y = torch.zeros(RP, nz, **f64)
        self.x = torch.zeros(n, RP, **f64)
        self.w = torch.zeros(n, RP, **f64)
        self.r = torch.zeros(m, RP, **f64)
        self.scal = torch.zeros(RP, _native.S_COUNT, **f64)
        self.work = torch.zeros(L.bsls_bbm_workspace_size(m, n, nz, self.R), dtype=torch.uint8,
                                device='cuda')
        opts = options or {}
        self.options = dict(opts)
        P = _native.BBMProblem()
        P.m, P.n, P.nz, P.nblocks, P.R, P.RP = m, n, nz, lay.p, self.R, RP
        P.a_indptr, P.a_indices, P.a_val = (t.data_ptr() for t in self.a_img)
        P.at_indptr, P.at_indices, P.at_val = (t.data_ptr() for t in self.at_img)
        P.a_nnz = P.at_nnz = int(A.nnz)
        P.target, P.roww = self.target.data_ptr(), None
        P.xz, P.zx = lay.xz.data_ptr(), self.zx.data_ptr()
        P.pk_start, P.pk_mask, P.pk_len = (t.data_ptr() for t in self.pk[:3])
        P.npacks = self.npacks
        if self.nlong:
            P.long_packs, P.nlong = self.pk[3].data_ptr(), self.nlong
            P.iso_work, P.iso_work_bytes = self.iso_work.data_ptr(), self.iso_work.numel()
        for k in range(2):
            P.z[k], P.g[k] = self.z[k].data_ptr(), self.g[k].data_ptr()
        P.dz, P.y, P.x, P.w, P.r = (t.data_ptr() for t in (self.dz, self.y, self.x, self.w, self.r))
        P.scal, P.work, P.work_bytes = self.scal.data_ptr(), self.work.data_ptr(), self.work.numel()
        P.max_iter = int(opts.get('max_iter', 300000))
        P.opt_tol = float(opts.get('opt_tol', 1e-6))
        P.early_exit = 1 if early_exit else 0
        self.P = P
        for j, b in enumerate(cols):
            self.set_b(j, b)
        for j, w in enumerate(wts):
            self.set_row_weights(j, w)
        self.iterations = [None] * self.R
        self.stop_reasons = [None] * self.R

    def _col(self, j):
        j = int(j)
        if not 0 <= j < self.R:
            raise ValueError('problem %d of a batch of %d' % (j, self.R))
        return j

    def set_b(self, j, b):
        """Problem j's right-hand side for what runs next: target_j = A x0 - b."""
        j = self._col(j)
        b = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
        if b.size != self.m:
            raise ValueError('b has %d entries, expected one per row of A (%d)' % (b.size, self.m))
        self.target[:, j] = _torch().from_numpy(self._Ax0 - b).cuda()

    def set_row_weights(self, j, w):
        """Problem j's per-link weights (row_weights_check; None: unweighted).
        The batch runs the weighted finish as soon as one problem has weights;
        the others then carry ones, which change none of their bits."""
        j = self._col(j)
        w = row_weights_check(w, self.m)
        if w is None:
            self.roww[:, j] = 1.0
        else:
            self.roww[:, j] = _torch().from_numpy(w).cuda()
        self.weighted[j] = w is not None
        self.P.roww = self.roww.data_ptr() if any(self.weighted) else None

    def set_z0(self, z0s=None):
        """The starting points: None (zeros: x2z(particular_x0)), or R entries,
        each None or a vector of nz."""
        torch = _torch()
        self.z[0].zero_()
        if z0s is None:
            return
        if len(z0s) != self.R:
            raise ValueError('z0 has %d entries for %d problems' % (len(z0s), self.R))
        for j, z0 in enumerate(z0s):
            if z0 is None:
                continue
            z0 = torch.as_tensor(z0, dtype=torch.float64).reshape(-1)
            if z0.numel() != self.nz:
                raise ValueError('z0[%d] has %d entries, expected %d' % (j, z0.numel(), self.nz))
            self.z[0][j].copy_(z0)

    def prologue(self):
        check(_native.lib().bsls_bbm_prologue(self.P, stream_handle()), 'bsls_bbm_prologue')

    def iterate(self, first, count):
        check(_native.lib().bsls_bbm_iterate(self.P, int(first), int(count), stream_handle()),
              'bsls_bbm_iterate')

    def stage(self, k, it):
        """One kernel of the step (bsls_bbm_stage, include/bsls_hip.h)."""
        check(_native.lib().bsls_bbm_stage(self.P, int(k), int(it), stream_handle()),
              'bsls_bbm_stage %d' % k)

    def scalars(self):
        """R x S_COUNT: row j is problem j's scal[] (the slots of BBEngine's)."""
        return self.scal[:self.R].cpu().numpy()

    def held_out(self):
        """Per problem, 0.5 sum of r_i^2 over its rows with weight 0 at the
        last finish (0.0 for an unweighted problem)."""
        s = self.scalars()
        return [0.5 * float(s[j, _native.S_HELD]) if self.weighted[j] else 0.0
                for j in range(self.R)]

    def current_z(self, j, zbuf):
        return self.z[int(zbuf)][j]

    def solve(self, z0=None, log=None, record_every=500, poll=50):
        """Run every problem to its own stop; log(j, i, z_j, dt) wherever
        BB.solve (python/BB.py:16,39-41) would log problem j.  Returns the R
        final z as host arrays; iterations[j] and stop_reasons[j] afterwards."""
        self.set_z0(z0)
        keep = lambda t: t.cpu().numpy().copy()
        if log is None:
            log = lambda j, i, s, d: time.time()

        def stopped(j, reason, last):
            self.stop_reasons[j], self.iterations[j] = reason, last
        ends = poll_solve(self, self.R, self.P.max_iter, record_every, poll, log,
                          first=lambda j: keep(self.z[0][j]),
                          state=lambda j, zb: keep(self.current_z(j, zb)), stopped=stopped)
        return [z for _, z in ends]
