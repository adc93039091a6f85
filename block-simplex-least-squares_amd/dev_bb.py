"""The fused z-space BB engine: its option checks, BBEngine (set up in named
stages), the device line search that runs on it, and the BB host loop that
BBEngine.solve and BatchBB.solve share."""
import contextlib
import ctypes
import os
import time
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sps

import _native
from _native import BBProblem, check, ptr, stream_handle
from dev_blocks import BlockLayout, need_two_routes, particular_x0, positive_sizes
from dev_images import (DeviceCSR, DevicePanels, DeviceTiles, PanelOverflow, _torch, k1_plan,
                        panel_rows, row_parts, scaled_incidence_scale, set_images, spmv_format,
                        tile_plan, value_codec)


def poll_solve(eng, R, max_iter, record_every, poll, log, first, state, stopped):
    """The BB host loop over R problems in lockstep: logs exactly where the
    reference's BB.solve does (python/BB.py:10,22-24,40-44) -- at 0, at every
    multiple of record_every and once more at the end; a 'no change in
    gradient' exit logs the final state only.

    eng: prologue(), iterate(first, count) and scalars() (S_COUNT slots, or R
    rows of them).  Each window runs to min(next record boundary, i + poll,
    max_iter), at least one iteration, then reads the scalars once.
    log(j, i, state, dt) returns the time the next dt counts from; first(j) is
    problem j's starting state and state(j, zbuf) a copy of its current one;
    stopped(j, reason, i) is called before a stopped problem's final log,
    after which the problem is frozen.  Returns (zbuf, final state) per
    problem."""
    start = [log(j, 0, first(j), 0) for j in range(R)]
    eng.prologue()
    i = 0
    warned = [0] * R
    ends = [None] * R
    while any(e is None for e in ends):
        nxt = min((i // record_every + 1) * record_every, i + poll, max_iter)
        if nxt <= i:
            nxt = i + 1
        eng.iterate(i + 1, nxt - i)
        i = nxt
        S = np.atleast_2d(eng.scalars())
        for j in range(R):
            if ends[j] is not None:
                continue
            s = S[j]
            if s[_native.S_WARN] > warned[j]:
                print('BB update is having some trouble, implement fix! t=%8.5e'
                      % s[_native.S_T])
                warned[j] = s[_native.S_WARN]
            stop = int(s[_native.S_STOP])
            last = int(s[_native.S_ITER]) if stop else i
            zb = int(s[_native.S_ZBUF]) if stop else (i & 1)
            if stop != _native.STOP_NOCHANGE and last % record_every == 0:
                start[j] = log(j, last, state(j, zb), time.time() - start[j])
            if stop:
                if stop == _native.STOP_NOCHANGE:
                    print('Exiting... no change in gradient')
                stopped(j, stop, last)
                z = state(j, zb)
                log(j, last, z, time.time() - start[j])
                ends[j] = (zb, z)
    return ends


def fixed_sum_bounds(A, AT, scaled):
    """(fx_a1, fx_a2) of bsls_bb_problem.fx_sums: per unit of the gathered
    vector's max, a bound on the sum of |terms| of any row -- the longest row
    for a scaled incidence (K1 gathers colv * x, K2 scales each row sum once:
    every term is a gathered entry), else the largest row sum of |values|;
    fx_a1 over the rows of A (K1), fx_a2 over those of A' (K2)."""
    def one(M):
        M = sps.csr_matrix(M)
        if M.nnz == 0:
            return 1.0
        if scaled:
            return float(max(1, int(np.max(np.diff(M.indptr)))))
        return float(max(np.max(np.asarray(abs(M).sum(axis=1)).ravel()), 1e-300))
    return one(A), one(AT)


def _env_tile_layouts():
    """BSLS_TILE_LAYOUT="a,at" as a tuple, or None when unset."""
    env = os.environ.get('BSLS_TILE_LAYOUT')
    return tuple(int(v) for v in env.split(',')) if env else None


def _fmt_or_env(fmt):
    """The SpMV format asked for: the argument, else the environment's, else 'auto'."""
    return fmt or os.environ.get('BSLS_SPMV_FORMAT') or 'auto'


def _env_flag(name):
    """An A/B switch of the environment: None when unset, else its integer."""
    v = os.environ.get(name)
    return None if v is None else int(v)


def fixed_sums_check(deterministic, tile_layouts, fmt, link_parts):
    """The engine choices fixed_sums cannot be combined with (ValueError).
    tile_layouts / fmt None fall back to the environment (direct callers;
    BBEngine passes the values it resolved)."""
    if deterministic:
        raise ValueError('fixed_sums and deterministic are two ways to the same end: choose one')
    lay = tile_layouts if tile_layouts is not None else _env_tile_layouts()
    if lay is not None and not (lay[0] in (1, 2) and lay[1] in (1, 2)):
        raise ValueError('fixed_sums needs the dealt tile layouts (1 or 2) for K1 and K2')
    if _fmt_or_env(fmt) == 'panels':
        raise ValueError("fixed_sums needs tile images: fmt='panels' has none")
    if link_parts is not None and int(link_parts) > 1:
        raise ValueError('fixed_sums does not cover link parts')


def row_weights_check(w, m):
    """Per-link weights as m finite, non-negative float64 values on the host
    (None stays None); anything else is a ValueError.  Pure host: runs before
    anything touches the device."""
    if w is None:
        return None
    if hasattr(w, 'detach'):              # a tensor, host or device
        w = w.detach().cpu().numpy()
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
    if w.size != int(m):
        raise ValueError('row_weights has %d entries, expected one per row of A (%d)'
                         % (w.size, int(m)))
    if not np.all(np.isfinite(w)):
        raise ValueError('row_weights must be finite (no NaN or inf)')
    if np.any(w < 0):
        raise ValueError('row_weights must be non-negative')
    return w


def reg_lambda_check(lam):
    """The regulariser's lambda as a float: finite and >= 0 (None is 0);
    anything else is a ValueError.  Pure host."""
    if lam is None:
        return 0.0
    if isinstance(lam, bool) or not np.isscalar(lam) or isinstance(lam, (str, bytes)):
        raise ValueError('reg_lambda must be a number (got %r)' % (lam,))
    lam = float(lam)
    if not np.isfinite(lam) or lam < 0:
        raise ValueError('reg_lambda must be finite and >= 0 (got %r)' % (lam,))
    return lam


def reg_weights_check(d, n):
    """The regulariser's per-route weights d as n finite, non-negative float64
    values on the host (None stays None: ones); anything else is a ValueError.
    Pure host."""
    if d is None:
        return None
    if hasattr(d, 'detach'):
        d = d.detach().cpu().numpy()
    d = np.ascontiguousarray(np.asarray(d, dtype=np.float64).reshape(-1))
    if d.size != int(n):
        raise ValueError('reg_weights has %d entries, expected one per route (%d)'
                         % (d.size, int(n)))
    if not np.all(np.isfinite(d)):
        raise ValueError('reg_weights must be finite (no NaN or inf)')
    if np.any(d < 0):
        raise ValueError('reg_weights must be non-negative')
    return d


def _wave_tree(v):
    """block_sum's sums (bsls_common.hpp) over rows of 256 thread values: the
    xor butterfly inside each wave of 64, then the waves left to right."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def reg_model(z, layout, w):
    """NumPy model of the bb_reg kernel (csrc/bb_reg.hpp): for the block layout
    `layout` (a BlockLayout or the block sizes), z (nz) and w (n per-route
    weights lambda d^2), returns (reg_g, total) -- reg_g = N'(w * (N z + x0)),
    the roundings NumPy's NT.dot(w * (N.dot(z) + x0)) has, and total = sum_i
    w_i (N z + x0)_i^2 added in the kernel's order (256 entries to a
    workgroup, block_sum's tree, then last_block_sum over the workgroups)."""
    sizes = np.asarray(getattr(layout, 'sizes', layout), dtype=np.int64)
    need_two_routes(sizes)
    n, p = int(sizes.sum()), int(sizes.size)
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if z.size != n - p or w.size != n:
        raise ValueError('reg_model: z has %d entries and w %d for n = %d, nz = %d'
                         % (z.size, w.size, n, n - p))
    xz = np.arange(n, dtype=np.int64) - np.repeat(np.arange(p, dtype=np.int64), sizes)
    xz[np.cumsum(sizes) - 1] = -1
    jp = np.concatenate(([-1], xz[:-1]))
    zp = np.where(jp >= 0, z[np.maximum(jp, 0)], 0.0)
    xh = np.where(xz >= 0, z[np.maximum(xz, 0)] - zp, (0.0 - zp) + 1.0)
    q = w * xh
    live = xz >= 0
    reg_g = np.zeros(n - p)
    reg_g[xz[live]] = (0.0 + q[live]) - q[np.nonzero(live)[0] + 1]
    # the sum: per workgroup, then thread t of the last workgroup adds slots
    # t, t + 256, .. in order before one more tree
    nb = -(-n // 256)
    t = np.zeros(nb * 256)
    t[:n] = q * xh
    part = _wave_tree(t)
    acc = np.zeros(256)
    for lo in range(0, nb, 256):
        seg = part[lo:lo + 256]
        acc[:seg.size] = acc[:seg.size] + seg
    return reg_g, float(_wave_tree(acc)[0])


def fixed_plan_fits(plan, halo):
    """Whether a tile plan (H, groups, order) leaves the LDS room for the two
    words per row of the fixed-point sums."""
    return 2 * (int(plan[0]) + halo + 1) * 8 <= _native.TILE_LDS_BYTES


class LineSearch:
    """LBFGS.solve's weak Wolfe line search (python/LBFGS.py:9-53) on a BBEngine,
    decided on the device (bsls_lbfgs_ls_begin / _trials): trials enqueued in
    chunks, the state read once per chunk.  search() returns (t, exit, trials,
    ||d||); after the accepted exit take() gives x_next, nabla_f(x_next) and
    f(x_next)."""

    CHUNK = int(os.environ.get('BSLS_LS_CHUNK', '4'))   # trials per state read

    def __init__(self, eng, c1=1e-3, c2=0.9):
        torch = _torch()
        L = _native.lib()
        nz = eng.nz
        f64 = dict(dtype=torch.float64, device='cuda')
        self.eng = eng
        self.pt = torch.empty(nz, **f64)
        self.gpt = torch.empty(nz, **f64)
        self.zero = torch.zeros(nz, **f64)
        self.fx = torch.zeros(1, **f64)
        self.st = torch.zeros(_native.LS_COUNT, **f64)
        self.S = torch.zeros(2, _native.S_COUNT, **f64)
        self.part = torch.zeros(max(1, L.bsls_lbfgs_ls_work_size(nz) // 8), **f64)
        self.tickets = torch.zeros(max(1, L.bsls_ticket_bytes() // 4), dtype=torch.int32,
                                   device='cuda')
        self.c1, self.c2 = float(c1), float(c2)

    def _state(self, x, d, gx, fx):
        return _native.LsState(x.data_ptr(), d.data_ptr(), gx.data_ptr(), self.pt.data_ptr(),
                               self.gpt.data_ptr(), self.zero.data_ptr(), fx.data_ptr(),
                               self.st.data_ptr(), self.S[0].data_ptr(), self.S[1].data_ptr(),
                               self.part.data_ptr(), self.tickets.data_ptr(), self.c1, self.c2)

    def search(self, x, d, gx, fx, y_out=None, s_out=None):
        """x (projected), d, gx = nabla_f(x): contiguous device vectors of nz;
        fx: f(x) as a one-element device tensor.  Returns (t, exit, trials,
        ||d||) after one host read per chunk of trials.  On the accepted exit
        the same read also brings f(x_next), y.s and g(x_next).g(x_next)
        (self.last = (f, ys, gg); bsls_lbfgs_ls_finish), with y = g(x_next) -
        gx and s = t d written into y_out / s_out when given."""
        L = _native.lib()
        S = self._state(x, d, gx, fx)
        P = self.eng.P
        st_h = stream_handle()
        yp = y_out.data_ptr() if y_out is not None else None
        sp = s_out.data_ptr() if s_out is not None else None
        self.last = None
        check(L.bsls_lbfgs_ls_begin(P, S, st_h), 'bsls_lbfgs_ls_begin')
        while True:
            check(L.bsls_lbfgs_ls_trials(P, S, self.CHUNK, st_h), 'bsls_lbfgs_ls_trials')
            check(L.bsls_lbfgs_ls_finish(P, S, yp, sp, st_h), 'bsls_lbfgs_ls_finish')
            st = self.st.cpu().numpy()
            if st[_native.LS_STOP] != 0:
                if st[_native.LS_DONE] != 0:
                    self.last = (float(st[_native.LS_FT]), float(st[_native.LS_YS]),
                                 float(st[_native.LS_GG]))
                return (float(st[_native.LS_T]), int(st[_native.LS_STOP]),
                        int(st[_native.LS_NTRIAL]), float(st[_native.LS_DNORM]))

    def take(self):
        """(x_next, nabla_f(x_next), f(x_next) as a one-element device tensor)
        of the accepted trial: the search's own buffers, handed over (fresh
        ones are allocated for the next search, no copies); f(x_next) is a
        view of the state's f(pt) slot, which the next search reads first."""
        torch = _torch()
        pt, gpt = self.pt, self.gpt
        self.pt, self.gpt = torch.empty_like(pt), torch.empty_like(gpt)
        return pt, gpt, self.st[_native.LS_FT:_native.LS_FT + 1]


class BBEngine:
    """Fused z-space projected BB (python/BB.py:7-45 over python/main.py:53-65).

    The device runs K2 -> K3 -> K1 per iteration (bsls_bb_iterate); the stop
    test, the BB step and every reduction stay on the device.  The host polls
    the scalar block every `poll` iterations and at each `record_every`
    boundary, to log states exactly where BB.solve logs them.
    """

    def __init__(self, A, b, block_sizes, options=None, early_exit=True, A_dev=None,
                 AT_dev=None, AT=None, target=None, x0=None, general=False, fmt=None,
                 tile_plans=(None, None), colv=None, deterministic=False, tile_layouts=None,
                 link_parts=None, fixed_sums=None, row_weights=None, reg_lambda=0.0,
                 reg_weights=None):
        # reg_lambda / reg_weights: the reference's weighted L2 regulariser,
        # + 0.5 lambda ||d o (N z + x0)||^2 (bsls_bb_problem.reg_w;
        # set_regulariser changes lambda or d between solves on the same images).
        # fixed_sums: order-free fixed-point row sums on the dealt tiles
        # (bsls_bb_problem.fx_sums) -- bit-reproducible iterates and exit
        # iterations from the default engine's walks.  row_weights: per-link
        # weights w (bsls_bb_problem.roww; f = 0.5 sum w r^2), a 0/1 mask for a
        # held-out fold -- set_row_weights swaps them between solves on the
        # same images.  The stages, in the order the device sees them:
        o = self._resolve(A, AT, block_sizes, general, fmt, colv, deterministic, tile_layouts,
                          link_parts, fixed_sums, row_weights, target, reg_lambda, reg_weights,
                          x0)
        _native.lib()                      # (a missing library fails before any upload)
        self.layout = BlockLayout(o.sizes)
        self._A_dev, self._AT_dev = A_dev, AT_dev
        self._build_images(o, tile_plans)
        self.options = dict(options or {})
        xin = self._allocate(o, b, x0, target)
        self._fill_problem(o, early_exit)
        self._form_target(xin, o.row_weights)
        if o.reg_lambda > 0.0:
            self.set_regulariser(o.reg_lambda, o.reg_weights)
        elif o.reg_weights is not None:
            self.set_regulariser(0.0, o.reg_weights)      # (d kept for a later lambda)

    def _resolve(self, A, AT, block_sizes, general, fmt, colv, deterministic, tile_layouts,
                 link_parts, fixed_sums, row_weights, target, reg_lambda=0.0, reg_weights=None,
                 x0=None):
        """Stage 1, host only (no library call, no torch): every option and
        environment switch resolved once, and everything that can be refused
        on them refused.  Sets the engine's option attributes and returns the
        host values the later stages work from."""
        parts = int(link_parts) if link_parts is not None else 1
        # fixed_sums None reads BSLS_FIXED_SUMS (1 = on) for the whole-problem
        # default engine; the engines built for something else (deterministic,
        # link parts, a column shard's target) do not take the default
        if fixed_sums is None:
            fixed_sums = (os.environ.get('BSLS_FIXED_SUMS', '0') not in ('', '0')
                          and not deterministic and target is None and not parts > 1)
        self.fixed_sums = bool(fixed_sums)
        # tile layouts (K1, K2): the dealt images (column-sorted gathers, LDS
        # atomic sums: the same sums to rounding, not run-to-run bit-identical;
        # C5 K1 1334 -> 374 us, K2 984 -> 503 us), with 3-byte entries (layout
        # 2: C5 K1 359 -> 331, K2 358 -> 345 us against 4-byte layout 1)
        # unless `deterministic`, which keeps the thread streams (every row
        # summed in CSR order: K2 bit-identical to SciPy with one group).
        # BSLS_TILE_LAYOUT="a,at" overrides.
        if tile_layouts is None:
            tile_layouts = _env_tile_layouts() or ((0, 0) if deterministic else (2, 2))
        self.tile_layouts = tile_layouts
        fmt = _fmt_or_env(fmt)
        # K3's warm start (pava_wave.hpp pava_warm_repair: within ulps of the reference
        # PAVA, not bit-identical): on unless deterministic; BSLS_K3_WARM=0/1
        warm = _env_flag('BSLS_K3_WARM')
        # K1's group sums by atomics (column shards) / K3's pack form: the
        # defaults (0) unless BSLS_K1_ATOMIC / BSLS_K3_MERGE = 0 / 1
        k1_atomic, k3_merge = (0 if v is None else (2 if v else 1)
                               for v in (_env_flag('BSLS_K1_ATOMIC'), _env_flag('BSLS_K3_MERGE')))
        if self.fixed_sums:
            fixed_sums_check(deterministic, tile_layouts, fmt, link_parts)
        A = sps.csr_matrix(A)
        self.row_weights = None
        row_weights = row_weights_check(row_weights, A.shape[0])
        if row_weights is not None and self.fixed_sums:
            raise ValueError('row_weights are not covered by fixed_sums: build the engine '
                             'without one of them')
        if self.fixed_sums and k1_atomic == 2:
            raise ValueError('fixed_sums keeps the ordered group sums: BSLS_K1_ATOMIC=1 '
                             'does not go with it')
        sizes = positive_sizes(block_sizes)
        if A.shape[1] != int(sizes.sum()):
            raise ValueError('A has %d columns but the blocks cover %d'
                             % (A.shape[1], int(sizes.sum())))
        need_two_routes(sizes)
        # the regulariser: the device forms N z + x0 with the particular x0
        # (1 at each block's last entry), so an engine built on another x0, or
        # on a column shard's target, cannot carry it
        self.reg_lambda, self.reg_d, self.reg_w = 0.0, None, None
        self._reg_ok = target is None and (
            x0 is None or np.array_equal(np.asarray(x0, dtype=np.float64).reshape(-1),
                                         particular_x0(sizes)))
        reg_lambda = reg_lambda_check(reg_lambda)
        reg_weights = reg_weights_check(reg_weights, A.shape[1])
        if reg_lambda > 0.0:
            self._reg_refusals(k1_atomic)
        AT = sps.csr_matrix(AT) if AT is not None else A.T.tocsr()
        # values dropped for a scaled incidence (colv: the caller's column
        # scales, else detected)
        if general:
            colv = None
        elif colv is None:
            colv = scaled_incidence_scale(A)
        self.scaled = colv is not None
        # per matrix: panels or streamed tiles (spmv_format)
        self.fmt_A = spmv_format(A, fmt, dealt=tile_layouts[0] in (1, 2))
        self.fmt_AT = spmv_format(AT, fmt, dealt=tile_layouts[1] in (1, 2))
        return SimpleNamespace(
            A=A, AT=AT, sizes=sizes, colv=colv, row_weights=row_weights, parts=parts,
            reg_lambda=reg_lambda, reg_weights=reg_weights,
            pava_warm=warm if warm is not None else (0 if deterministic else 1),
            k1_atomic=k1_atomic, k3_merge=k3_merge)

    def _build_images(self, o, tile_plans):
        """Stage 2: the fused kernels' images -- A (K1) and A' with halo rows
        (K2), each as panels or tiles (tiles when the panels overflow), under
        fixed_sums on plans with room for two words per row, and with
        link_parts the K1 row blocks cut into runs with K2's column groups
        over the same link ranges."""
        A, AT, lay, tile_layouts = o.A, o.AT, self.layout, self.tile_layouts
        # the general CSR copies (closures f / nabla_f, DORE, LBFGS, LS_postprocess)
        # are uploaded on first use: the fused loop never reads them
        self._A_host, self._AT_host = A, AT
        self.m, self.n, self.nz = A.shape[0], lay.n, lay.nz
        self.A_pan = self.AT_pan = self.A_til = self.AT_til = None
        if self.fixed_sums:
            # two words per row: plans for half the rows per block (as
            # DeviceLSQ's tiles_fixed); a caller's plan must leave that room
            tile_plans = (
                tile_plans[0] or tile_plan(self.m, self.n, 0, colv_lds=True,
                                           env='BSLS_TILE_PLAN_A', layout=tile_layouts[0],
                                           nnz=A.nnz),
                tile_plans[1] or tile_plan(self.n, self.m, 1, colv_lds=True,
                                           env='BSLS_TILE_PLAN_AT', layout=tile_layouts[1],
                                           nnz=AT.nnz))
            for plan, halo, name in ((tile_plans[0], 0, 'K1'), (tile_plans[1], 1, 'K2')):
                if not fixed_plan_fits(plan, halo):
                    raise ValueError('fixed_sums: the %s tile plan H = %d leaves no room for two '
                                     'words per row in the LDS' % (name, plan[0]))
        if self.fmt_A == 'panels':
            prow, groups = k1_plan(self.m)
            try:
                self.A_pan = DevicePanels(A, prow, False, groups, values=not self.scaled)
            except PanelOverflow:
                self.fmt_A = 'tiles'      # dense rows: the tiles have no such limit
        if self.fmt_A == 'tiles':
            self.A_til = DeviceTiles(A, 0, values=not self.scaled, plan=tile_plans[0],
                                     layout=tile_layouts[0])
        if self.fmt_AT == 'panels':
            try:
                self.AT_pan = DevicePanels(AT, panel_rows(self.n, 256), True, 1,
                                           values=not self.scaled)
            except PanelOverflow:
                self.fmt_AT = 'tiles'
        # link parts (the sharded schedule's exchange pipelined behind the
        # walks, bsls_bb_shard_iterate_parts): K1's row blocks cut into
        # `link_parts` runs, and K2's image in as many column groups over the
        # same link ranges, so K2 part q reads only the rows of r part q's
        # exchange delivered
        self.k1_part_bounds = None
        k2_gc = None
        if o.parts > 1:
            if self.fmt_A != 'tiles' or self.fmt_AT != 'tiles' or tile_layouts[1] not in (1, 2):
                raise ValueError('link parts need dealt tile images for K1 and K2')
            nrb, H = self.A_til.img['nrb'], self.A_til.img['H']
            self.k1_part_bounds = np.array(row_parts(nrb, o.parts), dtype=np.int64)
            if len(self.k1_part_bounds) - 1 != o.parts:
                raise ValueError('%d link parts need as many K1 row blocks (%d)'
                                 % (o.parts, nrb))
            k2_gc = np.minimum(self.k1_part_bounds * H, self.m)
        if self.fmt_AT == 'tiles':
            # (the thread-stream K2 keeps each row's colv in LDS beside its sum:
            # every term colv_i * r_j, SciPy's product; the dealt K2 scales
            # the row sum once, so its LDS holds twice the rows)
            plan_at = tile_plans[1]
            if k2_gc is not None and plan_at is None:
                H2, _, _ = tile_plan(self.n, self.m, 1, False, layout=tile_layouts[1], nnz=AT.nnz)
                plan_at = (H2, len(k2_gc) - 1, 0)
            self.AT_til = DeviceTiles(AT, 1, values=not self.scaled,
                                      colv_lds=self.scaled and tile_layouts[1] == 0,
                                      plan=plan_at, layout=tile_layouts[1], group_col=k2_gc)

    def _allocate(self, o, b, x, target):
        """Stage 3: every buffer the problem struct points at -- x0, target
        (the caller's, or -b until stage 5 adds A x0), the iterate, gradient
        and work buffers, the column scales and the K3 packs.  Returns the x
        stage 5 forms target from (None with a caller's target)."""
        torch = _torch()
        L = _native.lib()
        lay, colv = self.layout, o.colv
        dev = dict(dtype=torch.float64, device='cuda')
        self.x0 = x0 = particular_x0(lay.sizes, on_device=True)
        self.b = self._b_host = self._x0_own = None
        if target is not None:
            # column-sharded: the caller formed sum_g A_g x0_g - b (distributed.py)
            self.target = torch.as_tensor(target, dtype=torch.float64).cuda().contiguous()
            xin = None
        else:
            # target = A x0 - b (python/main.py:48), formed after the images are
            # up by the engine's own K1; x0 defaults to the particular solution,
            # as BSLSMatrices.initial_solution does
            xin = x0 if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64)).cuda()
            self.target = -torch.as_tensor(np.asarray(b, dtype=np.float64)).cuda()
            self._x0_own = None if x is None else xin.reshape(-1)
        # b stays on the device for link_metrics (target is A x0 - b by stage 5)
        if b is not None:
            self._b_host = np.ascontiguousarray(np.asarray(b, dtype=np.float64).reshape(-1))
            self.b = torch.from_numpy(self._b_host).cuda()
        self.z = [torch.zeros(max(self.nz, 1), **dev) for _ in range(2)]
        self.g = [torch.zeros(max(self.nz, 1), **dev) for _ in range(2)]
        self.x = torch.empty(lay.n, **dev)
        self.r = torch.empty(self.m, **dev)
        self.scal = torch.zeros(_native.S_COUNT, **dev)
        self.work = torch.zeros(L.bsls_bb_workspace_size(self.m, self.n, self.nz),
                                dtype=torch.uint8, device='cuda')
        ga = (self.A_pan or self.A_til).img['ngroups']
        self.rpart = torch.zeros(ga * self.m if ga > 1 or self.A_pan else 1, **dev)
        self.wpart = None
        if self.AT_til is not None and self.AT_til.img['ngroups'] > 1:
            ti = self.AT_til.img
            # + one slot per (group, row block): stage 8's r^2 slices
            self.wpart = torch.zeros(ti['ngroups'] * ti['nrb'] * (ti['H'] + 2), **dev)
        self.colv = torch.from_numpy(colv).cuda() if self.scaled else None
        # max |colv| (1 unscaled): with |x| <= 1, the bound on the gathered colv * x
        self.colv_max = float(np.max(np.abs(colv))) if (self.scaled and colv.size) else 1.0
        # the scales as the kernels read them every iteration: the narrowest
        # exact type (flows are integers: _Float16; value_codec)
        self.colv_codec, self.colv_n = 0, None
        if self.scaled:
            flag, cn = value_codec(np.asarray(colv, dtype=np.float64), 2)
            if flag:
                self.colv_codec = 2 if flag == _native.TILE_VAL16 else 1
                self.colv_n = torch.from_numpy(cn).cuda()
        # packs of one z-block longer than a wave: a workgroup each (bb_k3_long)
        ln = lay.packs()['len'].cpu().numpy()
        longs = np.nonzero(ln > 64)[0].astype(np.int32)
        self.long_packs = None
        if longs.size:
            off = np.concatenate(([0], np.cumsum(ln[longs]))).astype(np.int64)
            self.long_packs = torch.from_numpy(longs).cuda()
            self.long_off = torch.from_numpy(off).cuda()
            self.long_scratch = torch.zeros(L.bsls_bb_long_scratch_size(int(off[-1])),
                                            dtype=torch.uint8, device='cuda')
        return xin

    def _fill_problem(self, o, early_exit):
        """Stage 4: bsls_bb_problem pointed at the images and buffers, with
        the options resolved in stage 1.  Touches no device memory."""
        lay, opts = self.layout, self.options
        P = BBProblem()
        P.m, P.n, P.nz, P.nblocks = self.m, lay.n, lay.nz, lay.p
        set_images(P, self.A_pan, self.A_til, self.AT_pan, self.AT_til)
        P.wpart = self.wpart.data_ptr() if self.wpart is not None else None
        P.work_bytes = self.work.numel()
        P.colv = self.colv.data_ptr() if self.scaled else None
        P.colv_n = self.colv_n.data_ptr() if self.colv_n is not None else None
        P.colv_codec = self.colv_codec
        P.rpart = self.rpart.data_ptr()
        P.target = self.target.data_ptr()
        P.xstarts, P.zstarts, P.xz = (lay.xstarts.data_ptr(), lay.zstarts.data_ptr(),
                                      lay.xz.data_ptr())
        pk = lay.packs()
        P.pk_z0, P.pk_b0, P.pk_mask, P.pk_len = (pk['z0'].data_ptr(), pk['b0'].data_ptr(),
                                                 pk['mask'].data_ptr(), pk['len'].data_ptr())
        P.npacks = pk['n']
        if self.long_packs is not None:
            P.long_packs, P.nlong = self.long_packs.data_ptr(), int(self.long_packs.numel())
            P.long_off, P.long_scratch = self.long_off.data_ptr(), self.long_scratch.data_ptr()
        P.z[0], P.z[1] = self.z[0].data_ptr(), self.z[1].data_ptr()
        P.g[0], P.g[1] = self.g[0].data_ptr(), self.g[1].data_ptr()
        P.x, P.r, P.scal, P.work = (self.x.data_ptr(), self.r.data_ptr(), self.scal.data_ptr(),
                                    self.work.data_ptr())
        P.max_zblock = lay.max_zblock
        P.max_iter = int(opts.get('max_iter', 300000))
        P.opt_tol = float(opts.get('opt_tol', 1e-6))
        P.early_exit = 1 if early_exit else 0
        P.pava_warm, P.k1_atomic, P.k3_merge = o.pava_warm, o.k1_atomic, o.k3_merge
        if self.fixed_sums:
            P.fx_sums = 1
            P.fx_a1, P.fx_a2 = fixed_sum_bounds(o.A, o.AT, self.scaled)
            P.x_bound = self.colv_max
            self._rmax_off = int(_native.lib().bsls_bb_rmax_offset(self.m, self.n, self.nz))
        self.P = P
        self.z0 = None

    def _form_target(self, xin, row_weights):
        """Stage 5: target = A x0 - b by the engine's own K1 at iteration 0
        (unless the caller gave target), then the row weights installed."""
        if xin is not None:
            self.x.copy_(self.colv * xin if self.scaled else xin)
            if self.fixed_sums:
                self.set_x_bound(float(self.x.abs().max().item()))
            self.stage(_native.STAGE_K1, 0)        # r = A x0 + (-b), unweighted
            self.target.copy_(self.r)
        if row_weights is not None:
            self.set_row_weights(row_weights)

    @property
    def A(self):
        if self._A_dev is None:
            self._A_dev = DeviceCSR(self._A_host)
        return self._A_dev

    @property
    def AT(self):
        if self._AT_dev is None:
            self._AT_dev = DeviceCSR(self._AT_host)
        return self._AT_dev

    # -- raw device steps ------------------------------------------------------
    def set_z0(self, z0):
        torch = _torch()
        z0 = torch.as_tensor(z0, dtype=torch.float64).cuda().reshape(-1)
        if z0.numel() != self.nz:
            raise ValueError('z0 has %d entries, expected %d' % (z0.numel(), self.nz))
        self.z[0][:self.nz].copy_(z0)
        self.z0 = z0

    def set_x_bound(self, bound):
        """fixed_sums: the bound on |entries of x as K1 gathers them| for the
        calls enqueued next (bsls_bb_problem.x_bound; colv_max in iterations)."""
        self.P.x_bound = max(float(bound), 1e-300)

    def load_r(self, r):
        """Copy a residual into r as a K1 finish would leave it: under
        fixed_sums also max|r| in the workspace slots K2 scales from."""
        torch = _torch()
        self.r.copy_(torch.as_tensor(r, dtype=torch.float64).reshape(-1))
        if self.fixed_sums:
            n = _native.lib().bsls_bb_rmax_slots()
            slots = self.work[self._rmax_off:self._rmax_off + 8 * n].view(torch.float64)
            slots.zero_()
            slots[0] = self.r.abs().max()      # (the bit pattern the kernels' atomic max keeps)

    def set_row_weights(self, w):
        """Per-link weights for what runs next: m finite values >= 0 (host or
        device memory, copied to a device tensor the engine keeps), or None
        for the unweighted problem.  A pointer swap: the images, the workspace
        and target stay, and solve()'s prologue resets the scalars, so one
        engine serves every fold of a cross-validation.  The objective becomes
        f = 0.5 sum_i w_i r_i^2; rows with w_i == 0 are held out and their
        0.5 sum r_i^2 is held_out()."""
        w = row_weights_check(w, self.m)
        if w is None:
            self.row_weights = None
            self.P.roww = None
            return
        if self.fixed_sums:
            raise ValueError('row_weights are not covered by fixed_sums: build the engine '
                             'without one of them')
        if self.P.shard_role != 0 or self.P.r_fx > 0:
            raise ValueError('row_weights are not covered on a column shard')
        if self.P.k1_atomic == 2:
            raise ValueError('row_weights keep the ordered group sums: BSLS_K1_ATOMIC=1 '
                             'does not go with them')
        torch = _torch()
        self.row_weights = torch.from_numpy(w).cuda()
        self.P.roww = self.row_weights.data_ptr()

    def _reg_refusals(self, k1_atomic, shard_role=0, r_fx=0.0):
        """What a regulariser cannot be combined with (ValueError); host only."""
        if self.fixed_sums:
            raise ValueError('a regulariser is not covered by fixed_sums: build the engine '
                             'without one of them')
        if not self._reg_ok:
            raise ValueError('a regulariser needs the whole problem on the particular x0 '
                             '(1 at each block\'s last entry): not a column shard\'s target '
                             'or another x0')
        if shard_role != 0 or r_fx > 0:
            raise ValueError('a regulariser is not covered on a column shard')
        if k1_atomic == 2:
            raise ValueError('a regulariser keeps the ordered group sums: BSLS_K1_ATOMIC=1 '
                             'does not go with it')

    def set_regulariser(self, lam, d=None):
        """The weighted L2 regulariser for what runs next (the reference's
        reg = 'L2', python/CrossValidation.py:140-148): f gains 0.5 lam ||d o
        (N z + x0)||^2 and nabla_f gains N'(lam d^2 o (N z + x0)).  d: n finite
        values >= 0 (kept on the device; None keeps the last d, ones at
        first -- the reference's plain reg = 'L2'); lam finite and >= 0, 0 or
        None for no regulariser.  The engine forms reg_w = lam * d * d on the
        device; the images, the workspace and target stay, so one engine
        serves every lambda of a path."""
        lam = reg_lambda_check(lam)
        d = reg_weights_check(d, self.n)
        torch = _torch()
        if d is not None:
            self.reg_d = torch.from_numpy(d).cuda()
        if lam == 0.0:
            self.reg_lambda = 0.0
            self.P.reg_w = None
            return
        self._reg_refusals(self.P.k1_atomic, self.P.shard_role, self.P.r_fx)
        dev = dict(dtype=torch.float64, device='cuda')
        if self.reg_d is None:
            self.reg_d = torch.ones(self.n, **dev)
        if self.reg_w is None:
            self.reg_w = torch.empty(self.n, **dev)
            self.reg_g = torch.zeros(max(self.nz, 1), **dev)
            self.reg_work = torch.zeros(_native.lib().bsls_bb_reg_work_size(self.n),
                                        dtype=torch.uint8, device='cuda')
        torch.mul(self.reg_d * lam, self.reg_d, out=self.reg_w)     # (lam * d) * d
        self.reg_lambda = lam
        self.P.reg_w, self.P.reg_g, self.P.reg_work = (
            self.reg_w.data_ptr(), self.reg_g.data_ptr(), self.reg_work.data_ptr())

    def _unregularised_only(self, what):
        if self.reg_lambda:
            raise ValueError('%s is not covered by a regulariser (BB only): '
                             'set_regulariser(0) first' % what)

    def _reg_terms(self):
        """bsls_bb_reg at z[0], outside an iteration: between Z2X and K1."""
        if self.reg_lambda:
            check(_native.lib().bsls_bb_reg(self.P, 0, 0, stream_handle()), 'bsls_bb_reg')

    @contextlib.contextmanager
    def _plain(self):
        """The regulariser's pointer cleared for a call of the plain operators."""
        keep = self.P.reg_w
        self.P.reg_w = None
        try:
            yield
        finally:
            self.P.reg_w = keep

    def held_out(self):
        """0.5 sum of r_i^2 over the rows with weight 0 (r the plain residual)
        at the last solve() / f(z); 0.0 on an unweighted engine."""
        if self.row_weights is None:
            return 0.0
        return 0.5 * float(self.scal[_native.S_HELD].item())

    def link_metrics(self, z=None, nbins=6, edges=None):
        """The reference's link metrics of the fit (dev_metrics.metrics_from_cells:
        GEH, RMSE, pRMSE and error over the train and the held-out links, and
        per link class by flow) at z: None (the z of the last solve()), one z,
        or a list of z (logged states, device or host; the figures are then
        arrays over them).  x_hat = x0 + N z, A x_hat by apply_A_x (unweighted;
        the general CSR under fixed_sums), then one bsls_link_metrics launch
        over every state with row_weights as the mask (none: every link is
        train).  edges: the class edges, else link_classes(b, nbins).  The
        metrics are of the plain residual, with a regulariser too.  Overwrites
        the x / r scratch as apply_A_x does; scal, z, g, the weights and the
        regulariser stay."""
        import dev_metrics
        if self.b is None:
            raise ValueError('link metrics need b: this engine was built from a target '
                             'without one')
        if self.P.shard_role != 0 or self.P.r_fx > 0:
            raise ValueError('link metrics are not covered on a column shard')
        if not np.all(np.isfinite(self._b_host)):
            raise ValueError('b must be finite (no NaN or inf)')
        e = (dev_metrics.edges_check(edges) if edges is not None
             else dev_metrics.link_classes(self._b_host, nbins))
        torch = _torch()
        many = isinstance(z, (list, tuple))
        if z is None:
            if getattr(self, '_last_zbuf', None) is None:
                raise ValueError('link_metrics(z=None) reads the z of the last solve(): '
                                 'there was none')
            z = self.current_z(self._last_zbuf)
        zs = list(z) if many else [z]
        if not zs:
            raise ValueError('link_metrics needs at least one state')
        ax = torch.empty(len(zs), self.m, dtype=torch.float64, device='cuda')
        for s, zi in enumerate(zs):
            zi = torch.as_tensor(zi, dtype=torch.float64).cuda().reshape(-1)
            if zi.numel() != self.nz:
                raise ValueError('z has %d entries, expected %d' % (zi.numel(), self.nz))
            if self._x0_own is None:
                xh = self.n_apply(zi, with_x0=True)
            else:
                xh = self.n_apply(zi) + self._x0_own
            ax[s].copy_(self.apply_A_x(xh))
        cells = dev_metrics.launch(ax, self.m, self.b, self.row_weights, 0, e, self.m, len(zs))
        return dev_metrics.metrics_from_cells(cells if many else cells[0])

    def _unweighted_only(self, what):
        if self.row_weights is not None:
            raise ValueError('%s is not covered by row_weights (BB only): '
                             'set_row_weights(None) first' % what)

    def _fixed_only_bb(self, what):
        if self.fixed_sums:
            raise ValueError('%s is not covered by fixed_sums (BB only): build the engine '
                             'without it' % what)

    def prologue(self):
        if self.fixed_sums:
            # x = N (z0 + 1), then N z0: differences of two entries
            zmax = float(self.z[0][:self.nz].abs().max().item()) if self.nz else 0.0
            self.set_x_bound(2.0 * (zmax + 1.0) * self.colv_max)
        check(_native.lib().bsls_bb_prologue(self.P, stream_handle()), 'bsls_bb_prologue')

    def iterate(self, first, count):
        if self.fixed_sums:
            self.P.x_bound = self.colv_max        # |N z| <= 1 after K3's clip
        check(_native.lib().bsls_bb_iterate(self.P, int(first), int(count), stream_handle()),
              'bsls_bb_iterate')

    def stage(self, k, it):
        """One building block of an iteration (bsls_bb_stage, include/bsls_hip.h)."""
        check(_native.lib().bsls_bb_stage(self.P, int(k), int(it), stream_handle()),
              'bsls_bb_stage %d' % k)

    def set_rr_slice(self, lo, hi):
        """Rows [lo, hi) of r whose ||r||^2 stage 10 sums (the sliced sharded
        schedule: each rank its 1/world share)."""
        if not (0 <= lo <= hi <= self.m):
            raise ValueError('slice out of range')
        self.P.rr_lo, self.P.rr_hi = int(lo), int(hi)

    def fixed_r_ok(self):
        """Whether this column shard can keep r in 64-bit fixed point
        (bsls_bb_problem.r_fx): its K1 adds its column groups' sums by
        atomics with the init folded into K3 (a dealt K1 image of several
        groups on shard_role 1 / 2) and its K2 walks a dealt image."""
        P = self.P
        atomic = (P.k1_atomic == 2) if P.k1_atomic else P.shard_role != 0
        return bool(self.A_til is not None and self.A_til.img['ngroups'] > 1 and atomic
                    and self.AT_til is not None and self.tile_layouts[1] in (1, 2)
                    and P.shard_role != 0)

    def set_r_fixed(self, scale):
        """r in 64-bit fixed point at `scale` (a power of two; 0: doubles):
        the atomic K1's group sums then add as integers (order-free) and the
        r exchange sums int64 words (exact) -- the same r bits however the
        groups and ranks land.  Every |partial sum of r| must stay below
        2^62 / scale (distributed.ShardedBB sizes it)."""
        scale = float(scale)
        if scale > 0:
            self._fixed_only_bb('a fixed-point r')
        self._unweighted_only('a fixed-point r')
        if scale > 0:
            self._unregularised_only('a fixed-point r')
        if scale < 0 or (scale > 0 and not self.fixed_r_ok()):
            raise ValueError('fixed-point r needs an atomic sharded K1 (fixed_r_ok)')
        self.P.r_fx = scale

    @property
    def r_exchange(self):
        """r as the exchange sums it: int64 words under a fixed-point r."""
        torch = _torch()
        return self.r.view(torch.int64) if self.P.r_fx > 0 else self.r

    def residual_value(self):
        """r as doubles (a copy), whatever its representation."""
        torch = _torch()
        if self.P.r_fx > 0:
            return self.r.view(torch.int64).to(torch.float64) / self.P.r_fx
        return self.r.clone()

    def set_shard_role(self, role):
        """bsls_bb_problem.shard_role: 0 the whole problem here, 1 a column
        shard that adds target to its partial residual, 2 another column shard
        (distributed.ShardedBB)."""
        if role not in (0, 1, 2):
            raise ValueError('shard role must be 0, 1 or 2')
        if role != 0:
            self._fixed_only_bb('a column shard')
            self._unweighted_only('a column shard')
            self._unregularised_only('a column shard')
        self.P.shard_role = int(role)

    def row_blocks(self):
        """(K1 row blocks, rows per block): the granule of residual_rows."""
        R = ctypes.c_int64(0)
        nb = _native.lib().bsls_bb_row_blocks(self.P, ctypes.byref(R))
        if nb < 0:
            check(int(nb), 'bsls_bb_row_blocks')
        return int(nb), int(R.value)

    def k2_part(self, it, part, stream=None):
        """Stage 10 on K2 column group `part` (bsls_bb_k2_part; link-part engines)."""
        check(_native.lib().bsls_bb_k2_part(self.P, int(it), int(part), stream_handle(stream)),
              'bsls_bb_k2_part')

    def k1_rows(self, it, rb0, rb1, stream=None):
        """Stage 14 on K1 row blocks [rb0, rb1) (bsls_bb_k1_rows)."""
        check(_native.lib().bsls_bb_k1_rows(self.P, int(it), int(rb0), int(rb1),
                                            stream_handle(stream)), 'bsls_bb_k1_rows')

    def residual_rows(self, it, rb0, rb1, stream=None):
        """Stage 1 on K1 row blocks [rb0, rb1) (bsls_bb_residual_rows)."""
        check(_native.lib().bsls_bb_residual_rows(self.P, int(it), int(rb0), int(rb1),
                                                  stream_handle(stream)),
              'bsls_bb_residual_rows')

    # -- closures of main.solve_in_z (python/main.py:53-65), on the device ------
    def n_apply(self, z, with_x0=False, out=None):
        """N z (or x0 + N z) without materialising N."""
        torch = _torch()
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device='cuda')
        check(_native.lib().bsls_n_apply(ptr(out), ptr(z), ptr(self.layout.xstarts),
                                         self.layout.p, self.n, 1 if with_x0 else 0,
                                         stream_handle()), 'bsls_n_apply')
        return out

    def nt_apply(self, w, out=None):
        """N' w."""
        torch = _torch()
        if out is None:
            out = torch.empty(max(self.nz, 1), dtype=torch.float64, device='cuda')
        check(_native.lib().bsls_nt_apply(ptr(w), ptr(out), ptr(self.layout.xstarts),
                                          self.layout.p, self.n, stream_handle()),
              'bsls_nt_apply')
        return out[:self.nz]

    # The closures run on the fused kernels' images (K1 / K2 stages), not on
    # general CSR copies: z goes through z[0] (stage 6: x = colv * N z), K1
    # (stage 1: A x; stage 7: A x + target, ||r||^2, f) and K2 (stage 3 at
    # iteration 0: N'A'r).  They share the engine's buffers with the fused BB
    # loop, so they must not run while a solve() is in flight.
    def _x_of(self, z):
        torch = _torch()
        z = torch.as_tensor(z, dtype=torch.float64, device='cuda').reshape(-1)
        if z.numel() != self.nz:
            raise ValueError('z has %d entries, expected %d' % (z.numel(), self.nz))
        self.z[0][:self.nz].copy_(z)
        if self.fixed_sums:
            self.set_x_bound(2.0 * float(z.abs().max().item()) * self.colv_max if self.nz else 0.0)
        self.stage(_native.STAGE_Z2X, 0)

    def apply_A(self, z, alpha=1.0):
        """alpha A N z (DORE's linop with A scaled by alpha, gradient_descent.py:57-63).
        Unweighted, as apply_A_x and apply_AT: row_weights act on residual, f
        and nabla_f only."""
        self._fixed_only_bb('apply_A (DORE)')
        with self._plain():
            self._x_of(z)
            self.stage(_native.STAGE_K1_PARTIAL, 0)
        return self.r * alpha if alpha != 1.0 else self.r.clone()

    def apply_AT(self, r, alpha=1.0):
        """alpha N' A' r (DORE's linop_T)."""
        self.load_r(r)
        with self._plain():
            self.stage(_native.STAGE_K2, 0)
        g = self.g[0][:self.nz]
        return g * alpha if alpha != 1.0 else g.clone()

    def residual(self, z, alpha=1.0):
        """alpha (A N z + target) (DORE scales A and target by alpha); with
        row_weights w the weighted residual, alpha w * (A N z + target)."""
        self._x_of(z)
        self._reg_terms()
        self.stage(_native.STAGE_K1, 0)
        return self.r * alpha if alpha != 1.0 else self.r.clone()

    def f(self, z):
        """0.5 ||A N z + target||^2 (main.py:53), f as K1's finish forms it; with
        row_weights w, 0.5 sum w_i r_i^2 (and held_out() the zero-weight rows');
        with a regulariser + 0.5 lam ||d o (N z + x0)||^2."""
        self._x_of(z)
        self._reg_terms()
        self.stage(_native.STAGE_K1, 0)
        return float(self.scal[_native.S_FX].item())

    def nabla_f(self, z):
        """N' A' (A N z + target) (main.py:54); with row_weights w,
        N' A' (w * (A N z + target)); with a regulariser + N'(lam d^2 o (N z + x0))."""
        self._x_of(z)
        self._reg_terms()
        self.stage(_native.STAGE_K1, 0)
        self.stage(_native.STAGE_K2, 0)
        return self.g[0][:self.nz].clone()

    def line_search(self):
        """This engine's device weak Wolfe line search (LBFGS.solve)."""
        self._fixed_only_bb('the line search')
        self._unweighted_only('the line search')
        self._unregularised_only('the line search')
        ls = getattr(self, '_ls', None)
        if ls is None:
            ls = self._ls = LineSearch(self)
        return ls

    def apply_A_x(self, x):
        """A x for an x-space vector (LS_postprocess's A x_true)."""
        torch = _torch()
        x = torch.as_tensor(x, dtype=torch.float64, device='cuda').reshape(-1)
        if self.fixed_sums:
            # (the stage without target is not covered: the general CSR kernel)
            return self.A.matvec(x)
        self.x.copy_(self.colv * x if self.scaled else x)
        with self._plain():
            self.stage(_native.STAGE_K1_PARTIAL, 0)
        return self.r.clone()

    def proj(self, z):
        """isotonic_regression_multi_c on the z-blocks, then clip to [0, 1]
        (main.py:61-65); returns a new tensor like np.maximum(np.minimum(..)).
        The PAVA follows BSLS_ISO, read per call (IsoPlan.apply)."""
        torch = _torch()
        L = _native.lib()
        if self.layout.max_zblock < 1 or np.any(self.layout.sizes < 2):
            raise AssertionError   # the reference's strictly-increasing z-starts assert
        y = z.clone()
        self.layout.iso_plan().apply(y)
        return torch.clamp(y, 0.0, 1.0)

    def lsv_matvec(self, v):
        """N'A'A N v for ARPACK (bsls_utils.lsv_operator), on the fused images."""
        torch = _torch()
        vd = torch.from_numpy(np.ascontiguousarray(np.real(v), dtype=np.float64)).cuda()
        return self.apply_AT(self.apply_A(vd)).cpu().numpy()

    def scalars(self):
        return self.scal.cpu().numpy()

    def current_z(self, zbuf):
        return self.z[int(zbuf)][:self.nz]

    # -- BB.solve semantics ------------------------------------------------------
    def solve(self, z0=None, log=None, record_every=500, poll=50, to_host=True):
        """Run BB to its stopping rule; log(i, state, dt) exactly where
        python/BB.py:10,40-44 logs.  Returns the final z (device tensor)."""
        torch = _torch()
        if z0 is None:
            z0 = torch.zeros(self.nz, dtype=torch.float64)   # x2z(particular_x0) == 0
        self.set_z0(z0)
        keep = (lambda t: t.cpu().numpy().copy()) if to_host else (lambda t: t.clone())
        if log is None:
            log = lambda i, s, d: time.time()

        def stopped(j, reason, last):
            self.stop_reason, self.iterations = reason, last
        (zb, _), = poll_solve(self, 1, self.P.max_iter, record_every, poll,
                              lambda j, i, s, d: log(i, s, d), first=lambda j: keep(self.z0),
                              state=lambda j, zb: keep(self.current_z(zb)), stopped=stopped)
        self._last_zbuf = int(zb)
        return self.current_z(zb)

    def run_fixed(self, iters):
        """Enqueue exactly `iters` iterations (no host sync, no logging)."""
        self.iterate(1, iters)
