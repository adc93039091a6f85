"""The x-space side: the operator pair DeviceLSQ (residual and gradient on
panel or tile images of A and A') and the fused x-space BB / L-BFGS engine
XBBEngine that runs on it."""
import ctypes
import os
import time

import numpy as np
import scipy.sparse as sps

import _native
from _native import check, ptr, stream_handle
from dev_images import (DevicePanels, DeviceTiles, PanelOverflow, _torch, k1_plan, panel_rows,
                        scaled_incidence_scale, set_images, tile_plan)


class DeviceLSQ:
    """The x-space operator pair (csrc/lsq.hip, struct bsls_lsq_op): residual
    r = A x + add with ||r||^2, gradient g = A' r -- sparse_least_squares_obj's
    two SciPy products (algorithm_utils.py:88-94).  The residual walks column
    groups of panels (fixed order: f repeats bit for bit at the same x, which
    the reference's exits rely on -- BATCH.solve_LBFGS's revert stops on
    |f_old - f| < prog_tol with delta_x = 0); k1='tiles' (or
    BSLS_LSQ_K1=tiles) walks a dealt tile image of A instead (the z-space
    K1's walk: LDS atomic row sums, faster, the same sums to rounding only);
    k1='tiles_fixed' walks it with 64-bit fixed-point row sums (order-free:
    bit-repeatable like the panels, at the dealt walk's speed).
    A' is one group of panels (every row in CSR order: g bit-identical to
    SciPy's csr_matvec); k2='tiles' (or BSLS_LSQ_K2=tiles) walks a dealt tile
    image of A' instead (one group, LDS atomic row sums scaled by colv once per
    row: the same sums to rounding).  A scaled incidence drops the values
    (colv * x formed once per residual, A' entries scaled by colv row by row)."""

    def __init__(self, A, AT=None, general=False, k1=None, k2=None):
        torch = _torch()
        L = _native.lib()
        A = sps.csr_matrix(A)
        AT = sps.csr_matrix(AT) if AT is not None else A.T.tocsr()
        self.m, self.n = A.shape
        colv = None if general else scaled_incidence_scale(A)
        self.scaled = colv is not None
        k1 = k1 or os.environ.get('BSLS_LSQ_K1', 'panels')
        self.A_pan = self.A_til = None
        if k1 in ('tiles', 'tiles_fixed'):
            # (the fixed-point walk keeps two words per row: plan for twice the LDS)
            plan = (tile_plan(self.m, self.n, 0, colv_lds=True, layout=2, nnz=A.nnz)
                    if k1 == 'tiles_fixed' else None)
            self.A_til = DeviceTiles(A, 0, values=not self.scaled, layout=2, plan=plan)
            groups, npanels = self.A_til.img['ngroups'], 0
        else:
            prow, groups = k1_plan(self.m)
            self.A_pan = DevicePanels(A, prow, False, groups, values=not self.scaled)
            groups, npanels = self.A_pan.img['ngroups'], self.A_pan.img['npanels']
        self.k1 = k1
        k2 = k2 or os.environ.get('BSLS_LSQ_K2', 'panels')
        self.AT_pan = self.AT_til = None
        if k2 == 'tiles':
            # one group of row blocks as tall as the LDS holds, whole rounds of
            # 256 workgroups (the z-space K2's plan)
            hmax = _native.TILE_LDS_BYTES // 8 - 1
            nrb = -(-max(256, -(-self.n // hmax)) // 256) * 256
            # (a tile holds at least 64 rows: bsls_tiles_build_dealt3)
            self.AT_til = DeviceTiles(AT, 0, values=not self.scaled,
                                      plan=(max(64, -(-self.n // nrb)), 1, 0), layout=2)
        else:
            self.AT_pan = DevicePanels(AT, panel_rows(self.n, 256), False, 1,
                                       values=not self.scaled)
        self.k2 = k2
        dev = dict(dtype=torch.float64, device='cuda')
        self.colv = torch.from_numpy(colv).cuda() if self.scaled else None
        # max |colv| (1 unscaled): with |x| <= 1, the bound on the gathered colv * x
        self.colv_max = float(np.max(np.abs(colv))) if (self.scaled and colv.size) else 1.0
        self.xs = torch.empty(self.n, **dev) if self.scaled else None
        self.rpart = torch.zeros(groups * self.m, **dev)
        self.work = torch.zeros(L.bsls_lsq_workspace_size(self.m, npanels),
                                dtype=torch.uint8, device='cuda')
        op = _native.LsqOp()
        op.m, op.n = self.m, self.n
        set_images(op, self.A_pan, self.A_til, self.AT_pan, self.AT_til)
        op.colv = ptr(self.colv)
        op.rpart = self.rpart.data_ptr()
        op.xs = ptr(self.xs)
        op.work, op.work_bytes = self.work.data_ptr(), self.work.numel()
        if k1 == 'tiles_fixed':
            # fixed-point row sums: the bound of a row's |terms| per unit of
            # max|x| -- its entry count for a scaled incidence (the walk
            # gathers colv * x), else sum_j |A_ij|.  (dev_bb.fixed_sum_bounds
            # is the same bound summed by SciPy: the two differ in their last
            # bits and the bound feeds the fixed-point scale, so each engine
            # keeps its own expression)
            op.fixed = 1
            if self.scaled:
                op.fx_amax = float(max(1, int(np.max(np.diff(A.indptr))) if A.nnz else 1))
            else:
                rows = np.repeat(np.arange(self.m), np.diff(A.indptr))
                ra = np.bincount(rows, weights=np.abs(A.data), minlength=self.m)
                op.fx_amax = float(max(np.max(ra) if ra.size else 0.0, 1e-300))
        self.op = op

    def residual(self, x, out, add=None, sq=None):
        check(_native.lib().bsls_lsq_residual(self.op, ptr(x), ptr(add), ptr(out), ptr(sq),
                                              stream_handle()), 'bsls_lsq_residual')
        return out

    def gradient(self, r, out):
        check(_native.lib().bsls_lsq_gradient(self.op, ptr(r), ptr(out), stream_handle()),
              'bsls_lsq_gradient')
        return out


def lsq_operator(A, AT=None, general=False, k1=None, k2=None):
    """DeviceLSQ (residual walk `k1`, gradient walk `k2`: 'panels' or 'tiles',
    see DeviceLSQ), or None (the caller keeps the general CSR kernels) when the
    panel format cannot hold the matrix (dense rows)."""
    try:
        return DeviceLSQ(A, AT, general=general, k1=k1, k2=k2)
    except PanelOverflow:
        return None


class XBBEngine:
    """Fused x-space projected BB (python/BATCH.py:55-106 over
    algorithm_utils.get_solver_parts(is_sparse=True), python/algorithm_utils.py:
    182-271): the step, projection, objective, Armijo backtracking
    (line_search_np, :113-137) and stopping test (:158-172) run as device rounds
    (csrc/xbb.hip, bsls_xbb_rounds); the host polls the mode every `poll`
    rounds."""

    def __init__(self, obj, proj, A_dev=None, lbfgs=0):
        """lbfgs = C > 0: BATCH.solve_LBFGS (python/BATCH.py:110-214) with C
        corrections -- the BB step of iterations i > 5 replaced by
        LBFGS_helper's two-loop recursion on the device (csrc/xbb.hip
        xlb_step / xlb_dir)."""
        torch = _torch()
        L = _native.lib()
        self.obj, self.proj = obj, proj
        m, n = obj.m, obj.n
        if proj.n != n:
            raise ValueError('projection covers %d entries, A has %d columns' % (proj.n, n))
        dev = dict(dtype=torch.float64, device='cuda')
        self.m, self.n = m, n
        self.x = torch.zeros(n, **dev)
        self.g = torch.zeros(n, **dev)
        self.xn = torch.zeros(n, **dev)
        self.gn = torch.zeros(n, **dev)
        self.r = torch.zeros(m, **dev)
        self.scal = torch.zeros(_native.XS_COUNT, **dev)
        self.work = torch.zeros(L.bsls_xbb_workspace_size(m, n, obj.A.ntiles, obj.AT.ntiles),
                                dtype=torch.uint8, device='cuda')
        self.hist = None
        P = _native.XBBProblem()
        P.m, P.n, P.nblocks, P.max_block = m, n, proj.p, proj.max_block
        # bit 0: the l1 ball; bit 1: the sort-free projection (BSLS_PROJ=fast,
        # as c_extensions' proj_multi_*_c take it: 1e-12, not bit-identical)
        P.ball = ((1 if proj.kind == 'ball' else 0)
                  | (2 if os.environ.get('BSLS_PROJ', 'exact') == 'fast' else 0))
        for dst, M in ((P.A, obj.A), (P.AT, obj.AT)):
            dst.rows = M.m
            dst.indptr, dst.indices, dst.data = (M.indptr.data_ptr(), M.indices.data_ptr(),
                                                 M.data.data_ptr())
            dst.tiles, dst.ntiles, dst.group = M.tiles.data_ptr(), M.ntiles, M.group
        P.neg_b = obj.neg_b.data_ptr()
        P.starts = proj.starts.data_ptr()
        P.x, P.g, P.xn, P.gn = (self.x.data_ptr(), self.g.data_ptr(), self.xn.data_ptr(),
                                self.gn.data_ptr())
        P.r, P.scal = self.r.data_ptr(), self.scal.data_ptr()
        P.proj_work, P.proj_work_bytes = proj.ws.data_ptr(), proj.ws.numel()
        P.work, P.work_bytes = self.work.data_ptr(), self.work.numel()
        lsq = getattr(obj, 'lsq', None)
        P.lsq = ctypes.pointer(lsq.op) if lsq is not None else None
        self._lsq, self._xb = lsq, 0.0
        self.lbfgs = int(lbfgs)
        if self.lbfgs < 0:
            raise ValueError('corrections must be >= 0')
        if self.lbfgs:
            self.s = torch.zeros(n, **dev)
            self.y = torch.zeros(n, **dev)
            self.lb = torch.zeros(max(1, L.bsls_xbb_lbfgs_size(self.lbfgs) // 8), **dev)
            P.lbfgs, P.s, P.y, P.lb = (self.lbfgs, self.s.data_ptr(), self.y.data_ptr(),
                                       self.lb.data_ptr())
        self.P = P

    def start(self, x_init, f_min=None, opt_tol=1e-6, max_iter=2000, prog_tol=1e-12,
              hist_cap=None):
        torch = _torch()
        x0 = torch.as_tensor(np.asarray(x_init, dtype=np.float64) if not hasattr(x_init, 'cpu')
                             else x_init, dtype=torch.float64).cuda().reshape(-1)
        if x0.numel() != self.n:
            raise ValueError('x_init has %d entries, expected %d' % (x0.numel(), self.n))
        self.x.copy_(x0)
        # every iterate the rounds evaluate is x_init, a projection onto the
        # simplex / l1 ball (entries within [-1, 1]) or a convex combination of
        # those: its entries stay within max(1, max|x_init|), which lets a
        # fixed-point residual skip its per-call max pass (bsls_lsq_op.x_bound)
        self._xb = 0.0
        lsq = self._lsq
        if lsq is not None and lsq.op.fixed:
            xm = float(x0.abs().max()) if x0.numel() else 0.0
            if np.isfinite(xm):
                self._xb = max(1.0, xm) * lsq.colv_max
        cap = int(hist_cap if hist_cap is not None else min(max(int(max_iter), 1) + 1, 1 << 22))
        if self.hist is None or self.hist.numel() < cap:
            self.hist = torch.zeros(cap, dtype=torch.float64, device='cuda')
        P = self.P
        P.hist, P.hist_cap = self.hist.data_ptr(), cap
        P.max_iter = int(min(max_iter, 2 ** 62))
        P.opt_tol, P.prog_tol = float(opt_tol), float(prog_tol)
        P.has_fmin = 0 if f_min is None else 1
        P.f_min = 0.0 if f_min is None else float(f_min)
        self.f_min = f_min
        check(_native.lib().bsls_xbb_init(P, stream_handle()), 'bsls_xbb_init')

    def rounds(self, count):
        lsq = self._lsq
        if lsq is not None and self._xb > 0.0:
            lsq.op.x_bound = self._xb          # read by the launches enqueued below only
        try:
            check(_native.lib().bsls_xbb_rounds(self.P, int(count), stream_handle()),
                  'bsls_xbb_rounds')
        finally:
            if lsq is not None:
                lsq.op.x_bound = 0.0

    def scalars(self):
        return self.scal.cpu().numpy()

    def solve(self, x_init, f_min=None, opt_tol=1e-6, max_iter=2000, prog_tol=1e-12, poll=8):
        """BATCH.solve_BB's result dict: f, x (NumPy), stop, iterations, progress
        ([time, f] per iteration; the time is the wall clock of the poll that
        saw the iteration finish), plus rounds / backtracks."""
        self.start(x_init, f_min, opt_tol, max_iter, prog_tol)
        t0 = time.time()
        seen, times = 0, [0.0]
        while True:
            self.rounds(poll)
            s = self.scalars()
            it = int(s[_native.XS_ITER])
            now = time.time() - t0
            times.extend([now] * max(0, it - 1 - seen))
            seen = max(seen, it - 1)
            if int(s[_native.XS_MODE]) == _native.XM_STOPPED:
                break
        f, f_old = float(s[_native.XS_F]), float(s[_native.XS_FOLD])
        reason = int(s[_native.XS_STOP])
        if reason == _native.XSTOP_MAXITER:
            stop = 'max_iter'
        elif reason == _native.XSTOP_OPT:
            stop = 'f-f_min = {} < opt_tol'.format(f - f_min)
        else:
            stop = '|f_old-f| = {} < prog_tol'.format(abs(f_old - f))
        k = min(it, self.P.hist_cap)
        fh = self.hist[:k].cpu().numpy()
        progress = [[times[j] if j < len(times) else times[-1], float(fh[j])] for j in range(k)]
        return {'f': f, 'x': self.xn.cpu().numpy(), 'stop': stop, 'iterations': it,
                'progress': progress, 'rounds': int(s[_native.XS_ROUNDS]),
                'backtracks': int(s[_native.XS_BACKTRACKS])}
