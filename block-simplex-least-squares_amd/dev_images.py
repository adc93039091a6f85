"""Matrix images of the fused kernels and their host planners: the general CSR
copy, the panel and tile images of A and A' (host builders, NumPy models of
the kernels' walks, the device copies with their ctypes structs) and the
launch plans that size them.  The planners and models need no GPU."""
import os

import numpy as np
import scipy.sparse as sps

import _native
from _native import check, ptr, stream_handle


def _torch():
    """torch, imported on first use: the planners run without it (the one
    place; the other dev_* modules import this)."""
    import torch
    return torch


class DeviceCSR:
    """A CSR matrix resident in HBM (int64 indptr, int32 indices, fp64 data) plus
    its CSR-stream row tiles (<= 2048 nonzeros, <= 1024 rows each; with
    `tile_ends` tiles end only at those rows)."""

    def __init__(self, A, tile_ends=None, group=None):
        torch = _torch()
        A = sps.csr_matrix(A)
        A.sort_indices()
        self.shape = A.shape
        self.m, self.n = A.shape
        self.nnz = int(A.nnz)
        if self.n >= 2 ** 31:
            raise ValueError('column count exceeds int32 indices; shard the columns')
        ip = A.indptr.astype(np.int64)
        self.indptr = torch.from_numpy(ip).cuda()
        self.indices = torch.from_numpy(A.indices.astype(np.int32)).cuda()
        self.data = torch.from_numpy(A.data.astype(np.float64)).cuda()
        tiles = _native.plan_tiles(ip, ends=tile_ends)
        self.ntiles = int(tiles.shape[0] - 1)
        self.tiles = torch.from_numpy(tiles).cuda()
        self.group = group or _native.group_for_rows(self.m / max(self.ntiles, 1))
        self._work = None

    def matvec(self, x, out=None, add=None, alpha=1.0, want_sq=False):
        """out = alpha * (A x) + add ; returns (out, sq) with sq = ||out||^2 (device
        scalar tensor) when want_sq."""
        torch = _torch()
        L = _native.lib()
        if out is None:
            out = torch.empty(self.m, dtype=torch.float64, device='cuda')
        sq = torch.zeros(1, dtype=torch.float64, device='cuda') if want_sq else None
        if self._work is None:
            self._work = torch.zeros(L.bsls_spmv_workspace_size(self.ntiles), dtype=torch.uint8,
                                     device='cuda')
        check(L.bsls_csr_spmv(self.m, ptr(self.indptr), ptr(self.indices), ptr(self.data),
                              ptr(self.tiles), self.ntiles, ptr(x), ptr(add), float(alpha),
                              ptr(out), ptr(sq), self.group, ptr(self._work), self._work.numel(),
                              stream_handle()), 'bsls_csr_spmv')
        return (out, sq) if want_sq else out


def even_bounds(lo, hi, parts):
    """parts + 1 increasing even column bounds from lo to hi (hi itself may be odd):
    chunk starts stay 16-B aligned for the LDS staging (panels.hpp)."""
    b = np.round(np.linspace(lo, hi, parts + 1) / 2.0).astype(np.int64) * 2
    b[0], b[-1] = lo, hi
    return np.unique(b)


def chunk_plan(ncols, ngroups, chunk=None):
    """Column chunks (<= chunk wide) nested in `ngroups` groups of near-equal
    width.  Returns (chunk_col, group_chunk)."""
    chunk = int(chunk or _native.PANEL_CHUNK)
    ngroups = max(1, min(int(ngroups), (ncols + 1) // 2))
    gb = even_bounds(0, ncols, ngroups)
    cols, gch = [0], [0]
    for g in range(gb.size - 1):
        w = int(gb[g + 1] - gb[g])
        k = max(1, -(-w // chunk))
        cb = even_bounds(int(gb[g]), int(gb[g + 1]), k)
        while np.any(np.diff(cb) > chunk):
            k += 1
            cb = even_bounds(int(gb[g]), int(gb[g + 1]), k)
        cols.extend(cb[1:].tolist())
        gch.append(len(cols) - 1)
    return np.array(cols, dtype=np.int64), np.array(gch, dtype=np.int64)


class PanelOverflow(ValueError):
    """A 64-row slice holds more entries in one chunk than the panel format's
    16-bit running counts address (dense rows): the caller falls back to
    another format (BBEngine: streamed tiles; DeviceLSQ users: the CSR kernels)."""


def build_panels(M, prow, halo=False, chunk_col=None, group_chunk=None, values=True):
    """Panel image of the CSR matrix M (include/bsls_hip.h struct bsls_panels,
    csrc/panels.hpp).  Host arrays in a dict; `values=False` drops the entry
    values (scaled incidence).  Vectorised: two sorts over the entries."""
    M = sps.csr_matrix(M)
    M.sort_indices()
    R, C = M.shape
    PW = _native.PANEL_WAVES
    prow = int(prow)
    if not 1 <= prow <= _native.PANEL_ROWS or prow + int(halo) > 256:
        raise ValueError('prow out of range')
    if chunk_col is None:
        chunk_col, group_chunk = chunk_plan(C, 1)
    chunk_col = np.asarray(chunk_col, dtype=np.int64)
    group_chunk = np.asarray(group_chunk, dtype=np.int64)
    widths = np.diff(chunk_col)
    if np.any(widths > _native.PANEL_CHUNK) or np.any(chunk_col[:-1] % 2):
        raise ValueError('bad chunk plan')
    nch = chunk_col.size - 1
    npan = max(1, -(-R // prow))
    nrb = -(-npan // PW)
    nsegs = nrb * nch * PW
    ip = M.indptr.astype(np.int64)
    rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(ip))
    cols = M.indices.astype(np.int64)
    vals = M.data
    pn = rows // prow
    lr = rows - pn * prow
    if halo:
        # row 0 of panel p > 0 is also local row prow of panel p - 1
        h = np.nonzero((lr == 0) & (pn > 0))[0]
        pn = np.concatenate([pn, pn[h] - 1])
        lr = np.concatenate([lr, np.full(h.size, prow, dtype=np.int64)])
        cols = np.concatenate([cols, cols[h]])
        vals = np.concatenate([vals, vals[h]])
    ch = np.searchsorted(chunk_col, cols, side='right') - 1
    seg = ((pn // PW) * nch + ch) * PW + pn % PW
    # storage order: segment, row (slice-major), then the row's entries by
    # column, each row's run padded to an even length (aligned pair loads)
    key = seg * 256 + lr
    order = np.argsort(key, kind='stable')
    key, cols, ch, vals = key[order], cols[order], ch[order], vals[order]
    E = key.size
    cnt_all = np.bincount(key, minlength=nsegs * 256).reshape(nsegs, 4, 64)
    D = cnt_all.max(axis=2)                       # nsegs x 4 (<= chunk width < 2^16)
    live = D > 0
    padc = cnt_all + (cnt_all & 1)
    incl = np.cumsum(padc, axis=2)                # per slice, inclusive over lanes
    if incl[:, :, 63].max(initial=0) > 0xFFFE:
        raise PanelOverflow('a 64-row slice has more than 65534 entries in one chunk')
    cnt = (incl | (cnt_all & 1))[live].astype(np.uint16).reshape(-1)
    cnt_off = np.concatenate(([0], np.cumsum(64 * live.sum(axis=1)))).astype(np.int64)
    ne = padc.sum(axis=(1, 2))
    ent_off = np.concatenate(([0], np.cumsum(ne))).astype(np.int64)
    seg_info = (D[:, 0] | (D[:, 1] << 16) | (D[:, 2] << 32) | (D[:, 3] << 48)).astype(np.int64)
    Ep = int(ent_off[-1])
    slack = 64
    ent = np.zeros(Ep + slack, dtype=np.uint16)
    val = np.zeros(Ep + slack, dtype=np.float64) if values else None
    if E:
        flat = padc.reshape(nsegs, 256)
        excl = (np.cumsum(flat, axis=1) - flat).reshape(-1)       # per (seg, row)
        newp = np.empty(E, dtype=bool)
        newp[0] = True
        np.not_equal(key[1:], key[:-1], out=newp[1:])
        pstart = np.nonzero(newp)[0]
        k = np.arange(E, dtype=np.int64) - np.repeat(pstart, np.diff(np.append(pstart, E)))
        dest = ent_off[key >> 8] + excl[key] + k
        ent[dest] = (cols - chunk_col[ch]).astype(np.uint16)
        if values:
            val[dest] = vals
    return dict(rows=R, cols=C, prow=prow, halo=int(bool(halo)), npanels=npan, nchunks=nch,
                ngroups=group_chunk.size - 1, tab_cap=max(64, int(widths.max(initial=2))),
                chunk_col=chunk_col, group_chunk=group_chunk, ent_off=ent_off, cnt_off=cnt_off,
                seg_info=seg_info, cnt=np.concatenate([cnt, np.zeros(64, np.uint16)]),
                ent=ent, val=val, nnz=E, stored=Ep)


def panels_matvec(img, x, colv=None):
    """Host restatement of the kernels' walk over a panel image (panel_segment
    in csrc/panels.hpp): per chunk group, row sums entry by entry in storage
    order; the group partials then added in group order (K1b).  Returns the
    kernels' bit pattern and, for the last group, the per-panel sums including
    halo rows.  Test helper (numpy, vectorised per diagonal)."""
    R, prow, halo = img['rows'], img['prow'], img['halo']
    nch = img['nchunks']
    PW = _native.PANEL_WAVES
    x = np.asarray(x, dtype=np.float64)
    parts = []
    for g in range(img['ngroups']):
        acc = np.zeros((img['npanels'], 256))
        for c in range(img['group_chunk'][g], img['group_chunk'][g + 1]):
            c0 = img['chunk_col'][c]
            for p in range(img['npanels']):
                sgi = ((p // PW) * nch + c) * PW + p % PW
                info = int(img['seg_info'][sgi])
                e = int(img['ent_off'][sgi])
                co = int(img['cnt_off'][sgi])
                for q in range(4):
                    Dq = (info >> (16 * q)) & 0xFFFF
                    if Dq == 0:
                        continue
                    st = img['cnt'][co:co + 64].astype(np.int64)
                    co += 64
                    inc = st & ~1
                    cnp = np.diff(np.concatenate(([0], inc)))          # padded counts
                    start = e + inc - cnp
                    cn = cnp - (st & 1)
                    rr = 64 * q + np.arange(64)
                    for k in range(Dq):
                        a = cn > k
                        t = x[c0 + img['ent'][start[a] + k].astype(np.int64)]
                        if img['val'] is not None:
                            acc[p, rr[a]] = acc[p, rr[a]] + img['val'][start[a] + k] * t
                        elif colv is not None:
                            acc[p, rr[a]] = acc[p, rr[a]] + colv[p * prow + rr[a]] * t
                        else:
                            acc[p, rr[a]] = acc[p, rr[a]] + t
                    e += int(cnp.sum())
        parts.append(acc)
    out = parts[0][:, :prow].reshape(-1)[:R].copy()
    for acc in parts[1:]:
        out = out + acc[:, :prow].reshape(-1)[:R]
    return out, parts[-1][:, :prow + halo]


def scaled_incidence_scale(A):
    """colv with A[i, j] == colv[j] for every stored entry, or None
    (bsls_utils.assert_scaled_incidence, bsls_utils.py:494-507, made exact)."""
    C = sps.csc_matrix(A)
    C.sort_indices()
    n = C.shape[1]
    lens = np.diff(C.indptr)
    colv = np.zeros(n)
    has = lens > 0
    colv[has] = C.data[C.indptr[:-1][has]]
    if C.nnz and not np.array_equal(C.data, np.repeat(colv, lens)):
        return None
    return colv


class DevicePanels:
    """A panel image on the device + the ctypes struct pointing at it."""

    def __init__(self, M, prow, halo=False, ngroups=1, values=True, img=None, chunk=None):
        torch = _torch()
        img = img or build_panels(M, prow, halo, *chunk_plan(M.shape[1], ngroups, chunk=chunk),
                                  values=values)
        self.img = img
        self.nnz = img['nnz']
        self.t = {}
        for k in ('chunk_col', 'group_chunk', 'ent_off', 'cnt_off', 'seg_info'):
            self.t[k] = torch.from_numpy(np.ascontiguousarray(img[k], dtype=np.int64)).cuda()
        self.t['cnt'] = torch.from_numpy(img['cnt'].view(np.int16)).cuda()
        self.t['ent'] = torch.from_numpy(img['ent'].view(np.int16)).cuda()
        if img['val'] is not None:
            self.t['val'] = torch.from_numpy(img['val']).cuda()
        S = _native.Panels()
        for k in ('rows', 'cols', 'prow', 'halo', 'npanels', 'nchunks', 'ngroups', 'tab_cap'):
            setattr(S, k, int(img[k]))
        for k, v in self.t.items():
            setattr(S, k, v.data_ptr())
        self.struct = S

    def bytes(self):
        return sum(v.numel() * v.element_size() for v in self.t.values())


def tile_plan(rows, cols, halo=0, colv_lds=False, cus=256, l2_slice=None, env=None, layout=0,
              nnz=None):
    """(H, ngroups, order) of a tile image (include/bsls_hip.h struct bsls_tiles,
    csrc/tiles.hpp): column groups (a power of two) until one group's slice of
    the gathered vector fits an XCD's L2 (order 1, XCD-sequential, past 8
    groups); row blocks as tall as the LDS holds (half of it when K2 keeps the
    column scales beside the sums: scaled incidence, one group), at least one
    workgroup per CU, the grid rounded up to whole rounds of `cus` workgroups.
    The environment variable `env` ("H,groups") overrides it."""
    plan = os.environ.get(env) if env else None
    if plan:
        v = [int(a) for a in plan.split(',')]
        H, G = v[0], v[1]
        return H, G, (v[2] if len(v) > 2 else (1 if G > 8 else 0))
    if layout in (1, 2):
        # dealt image: one round of workgroups (one per CU); K1 with as many
        # column groups, up to 8, as keep its row blocks within the LDS -- a
        # narrower group puts more of a tile's entries on each gathered line,
        # past 8 the last-arriving workgroups' group sums make a tail.
        # Measured (tools/stage_time.py): C3 K1 G x row blocks 8 x 32 34.0 us
        # (4 x 64: 36.5, 16 x 16: 51.8, 2 x 128: 46.9, 8 x 64: 46.6, 32 x 8:
        # 126); C5 K1 4 x 64 374 us (the most the LDS allows in one round;
        # 8 x 64: 400, 16: 526, 32: 812; 2 / 1 groups leave CUs idle: 698 /
        # 1303).  K2 (the routes' rows: partial sums of n rows are dear) one
        # group: C3 256 row blocks 36.9 us (128: 48.9, 500: 47.0), C5 512
        # row blocks 370 us (before the row-sum scaling: 2 groups 611, 4: 775
        # against 503).
        mult = 2 if colv_lds else 1
        hmax = _native.TILE_LDS_BYTES // (8 * mult) - 1 - halo
        G = 1
        if not halo:
            G = 8
            while G > 1 and (-(-rows * G // cus) > hmax or G > cols):
                G //= 2
        nmin = -(-rows // hmax)
        nrb = max(nmin, cus // G)
        nrb = -(-(nrb * G) // cus) * cus // G if nrb * G > cus else nrb
        H = max(64, -(-rows // nrb))
        # (K2 tiles as sparse as a C5 shard over 8 GPUs, 0.08 entries per
        # column, were given two groups of twice the rows until round 4: the
        # kernel alone 78.0 -> 72.5 us, but the rehearsed iteration is faster
        # with one group -- 160.7 against 149.6 us, 162.5 against 154.4 in an
        # earlier session -- the groups' partial row sums (2 x 10 MB through the
        # Infinity Cache) cost K1 and K3 more than K2 gains; tools/shard_ab_r04.sh)
        return int(H), int(G), 0
    if l2_slice is None:
        # measured on the C5 shard (tools/stage_time.py): K1 fastest with
        # 2.5-MB slices of x (4 groups: 112 us, 8: 148 us), K2 with the whole
        # 8-MB r in one group (117 us; 2: 122, 4: 150) -- one group also keeps
        # K2 bit-identical to SciPy
        l2_slice = (8 << 20) if halo else (3 << 20)
    G = 1
    while 8 * cols / G > l2_slice and G < 64:
        G *= 2
    G = max(1, min(G, cols))
    order = 1 if G > 8 else 0
    mult = 2 if (colv_lds and G == 1) else 1
    if layout == 1:
        hmax = _native.TILE_LDS_BYTES // (8 * mult) - 1 - halo      # rows + the dummy row
    else:
        per = _native.TILE_LDS_BYTES // (8 * _native.TILE_THREADS * mult) - 1
        hmax = per * _native.TILE_THREADS - halo
    nrb = max(-(-rows // hmax), -(-cus // G))
    nrb = -(-(nrb * G) // cus) * cus // G if nrb * G > cus else nrb
    H = max(64, -(-rows // nrb))
    return int(H), int(G), int(order)


def spmv_format(M, fmt=None, dealt=True):
    """'panels' or 'tiles' for the fused SpMV over matrix M (rows x cols).
    With the dealt tile layout available (`dealt`, i.e. not a deterministic
    engine) always tiles: measured on C3 (tools/stage_time.py --fmt) K1 34.0
    against the panels' 43.0 us, K2 36.9 against 41.4; on C5 the panels idle
    (0.3 entries per row per chunk).  Deterministic engines keep the panels
    while a panel chunk (BSLS_PANEL_CHUNK columns) holds at least one entry
    per row on average (C3: 3.2), the thread-stream tiles below that
    (csrc/tiles.hpp).  fmt / BSLS_SPMV_FORMAT force one."""
    fmt = fmt or os.environ.get('BSLS_SPMV_FORMAT') or 'auto'
    if fmt != 'auto':
        if fmt not in ('panels', 'tiles'):
            raise ValueError('unknown SpMV format %r' % fmt)
        return fmt
    if dealt:
        return 'tiles'
    R, C = M.shape
    lam = (M.nnz / max(R, 1)) * min(_native.PANEL_CHUNK, C) / max(C, 1)
    return 'tiles' if lam < 1.0 else 'panels'


def tiles_matvec(img, x, colv=None, group_sums=False):
    """Host restatement of the tile kernels' walk (csrc/tiles.hpp) over an image
    from _native.tiles_build: per (row block, group) each row summed entry by
    entry in stream order, the groups then added in group order.  Returns the
    row sums (halo rows dropped).  Test helper (NumPy, vectorised per quad)."""
    R, H, halo, G = img['rows'], img['H'], img['halo'], img['ngroups']
    T = _native.TILE_THREADS
    gc = img['group_col']
    x = np.asarray(x, dtype=np.float64)
    if img.get('layout', 0) in (1, 2):
        return _dealt_matvec(img, x, colv, group_sums)
    nslots = -(-(H + halo) // T)
    out = np.zeros(R)
    parts = []
    for g in range(G):
        acc = np.zeros(R)
        for rb in range(img['nrb']):
            rows = np.zeros((nslots + 1) * T)
            for w in range(16):
                s = (rb * G + g) * 16 + w
                q0, q1 = int(img['wave_off'][s]), int(img['wave_off'][s + 1])
                lanes = w * 64 + np.arange(64)
                for q in range(q0, q1, 64):
                    for j in range(4):
                        e = img['ent'][4 * (q + np.arange(64)) + j].astype(np.int64)
                        lr = (e >> 24) * T + lanes
                        xv = x[gc[g] + (e & 0xFFFFFF)]
                        if img['val'] is not None:
                            t = img['val'][4 * (q + np.arange(64)) + j] * xv
                        elif colv is not None:
                            rr = np.minimum(rb * H + lr, R - 1)
                            t = np.where(lr < H + halo, colv[rr], 0.0) * xv
                        else:
                            t = xv
                        rows[lr] = rows[lr] + t
            r0 = rb * H
            r1 = min(r0 + H, R)
            acc[r0:r1] = rows[:r1 - r0]
        parts.append(acc)
    out = parts[0].copy()
    for a in parts[1:]:
        out = out + a
    return (out, parts) if group_sums else out


def _dealt_matvec(img, x, colv=None, group_sums=False):
    """tiles_matvec for a layout-1 (dealt) image: every (quad-step, wave, slot,
    lane) entry added to its row (the device adds them with LDS atomics in no
    fixed order; the sums agree to rounding)."""
    R, H, halo, G = img['rows'], img['H'], img['halo'], img['ngroups']
    gc, wo = img['group_col'], img['wave_off']
    ent = img['ent'].astype(np.int64)
    cb = 16
    if img.get('layout', 1) == 2:
        # 3-byte entries: unpack every lane's 3 words into the 4-per-lane form
        cb = 24 - int(H + halo).bit_length()
        nl = int(wo[-1]) * 1024
        w = ent[:3 * nl].reshape(-1, 3)
        u = np.empty((nl, 4), dtype=np.int64)
        u[:, 0] = w[:, 0] & 0xFFFFFF
        u[:, 1] = (w[:, 0] >> 24) | ((w[:, 1] & 0xFFFF) << 8)
        u[:, 2] = (w[:, 1] >> 16) | ((w[:, 2] & 0xFF) << 16)
        u[:, 3] = w[:, 2] >> 8
        ent = u.reshape(-1)
    cmask = (1 << cb) - 1
    parts = []
    for g in range(G):
        acc = np.zeros(R)
        for rb in range(img['nrb']):
            t = rb * G + g
            q0, q1 = int(wo[t]), int(wo[t + 1])
            if q1 == q0:
                continue
            rows = np.zeros(H + halo + 1)
            lanes = np.arange(64)
            for q in range(q0, q1):
                for w in range(16):
                    u = ((q * 16 + w) * 64 + lanes) * 4
                    for j in range(4):
                        e = ent[u + j]
                        lr = e >> cb
                        col = gc[g] + int(img['base'][(q * 16 + w) * 4 + j]) + (e & cmask)
                        xv = x[np.minimum(col, x.size - 1)]
                        if img['val'] is not None:
                            term = img['val'][u + j] * xv
                        elif colv is not None:
                            rr = np.minimum(rb * H + lr, R - 1)
                            term = np.where(lr < H + halo, colv[rr], 0.0) * xv
                        else:
                            term = xv
                        np.add.at(rows, lr, term)
            r0 = rb * H
            r1 = min(r0 + H, R)
            acc[r0:r1] = rows[:r1 - r0]
        parts.append(acc)
    out = parts[0].copy()
    for a in parts[1:]:
        out = out + a
    return (out, parts) if group_sums else out


NT_BYTES = 256 << 20


def value_codec(val, layout):
    """(flag, array) for a dealt image's stored values: _Float16 or float when
    every value (padding zeros included) converts to that type exactly -- the
    kernels widen them back to the same doubles, so the products do not change
    (BSLS_TILE_VAL16 / VAL32, include/bsls_hip.h) -- else the doubles.
    BSLS_VAL_CODEC=f64|f32|f16 forces the choice down to the exact ones."""
    if val is None or layout not in (1, 2):
        return 0, val
    want = os.environ.get('BSLS_VAL_CODEC', 'auto')
    order = {'auto': ('f16', 'f32'), 'f16': ('f16', 'f32'), 'f32': ('f32',), 'f64': ()}[want]
    for c in order:
        dt = np.float16 if c == 'f16' else np.float32
        with np.errstate(over='ignore', invalid='ignore'):
            nv = val.astype(dt)
        if np.array_equal(nv.astype(np.float64), val):
            return (_native.TILE_VAL16 if c == 'f16' else _native.TILE_VAL32), nv
    return 0, val


def self_bytes(img):
    """Bytes of a tile image's entry stream (+ values)."""
    b = img['ent'].nbytes
    if img.get('val') is not None:
        b += img.get('val_dev', img['val']).nbytes
    return b


class DeviceTiles:
    """A tile image on the device + the ctypes struct pointing at it."""

    def __init__(self, M, halo=0, values=True, colv_lds=False, plan=None, layout=0,
                 group_col=None):
        torch = _torch()
        M = sps.csr_matrix(M)
        M.sort_indices()
        R, C = M.shape
        H, G, order = plan or tile_plan(R, C, halo, colv_lds,
                                        env='BSLS_TILE_PLAN_AT' if halo else 'BSLS_TILE_PLAN_A',
                                        layout=layout, nnz=M.nnz)
        if group_col is not None:
            # the caller's column groups (the sharded K2's link parts, aligned
            # with K1's row-block parts)
            gc = np.asarray(group_col, dtype=np.int64)
            G = gc.shape[0] - 1
            if gc[0] != 0 or gc[-1] != C:
                raise ValueError('column groups must cover [0, %d)' % C)
        else:
            gc = np.round(np.linspace(0, C, G + 1)).astype(np.int64)
        if np.any(np.diff(gc) < 1):
            raise ValueError('more column groups than columns')
        if layout in (1, 2):
            img = _native.tiles_build_dealt(M, H, halo, gc, values=values, packed=layout == 2)
        else:
            img = _native.tiles_build(M, H, halo, gc, values=values)
        img.update(rows=R, cols=C, H=H, halo=halo, ngroups=G, order=order, group_col=gc,
                   layout=layout)
        self.img = img
        self.nnz = int(M.nnz)
        self.t = {'group_col': torch.from_numpy(gc).cuda(),
                  'wave_off': torch.from_numpy(img['wave_off']).cuda(),
                  'ent': torch.from_numpy(img['ent'].view(np.int32)).cuda()}
        vflag, vdev = value_codec(img['val'], layout)
        self.val_codec = {0: 'f64', _native.TILE_VAL32: 'f32', _native.TILE_VAL16: 'f16'}[vflag]
        if img['val'] is not None:
            img['val_dev'] = vdev
            self.t['val'] = torch.from_numpy(vdev).cuda()
        if layout in (1, 2):
            self.t['base'] = torch.from_numpy(img['base']).cuda()
        S = _native.Tiles()
        # dealt images larger than the Infinity Cache stream their entries
        # non-temporally (csrc/tiles.hpp tq_load)
        nt = self_bytes(img) > NT_BYTES
        if os.environ.get('BSLS_TILE_NT'):          # A/B override of the policy
            nt = os.environ['BSLS_TILE_NT'] == '1'
        S.layout = layout | (_native.TILE_NT if layout in (1, 2) and nt else 0) | vflag
        S.base = self.t['base'].data_ptr() if layout in (1, 2) else None
        S.rows, S.cols, S.H, S.halo = R, C, H, halo
        S.nrb, S.ngroups, S.order, S.nquads = img['nrb'], G, order, img['nquads']
        S.group_col = self.t['group_col'].data_ptr()
        S.wave_off = self.t['wave_off'].data_ptr()
        S.ent = self.t['ent'].data_ptr()
        S.val = self.t['val'].data_ptr() if 'val' in self.t else None
        self.struct = S

    def bytes(self):
        return sum(v.numel() * v.element_size() for v in self.t.values())


def panel_rows(rows, workgroups_per_group, waves=16):
    """Rows per panel so one launch is about `workgroups_per_group` workgroups of
    16 panels per group (one per CU), within 64 .. BSLS_PANEL_ROWS."""
    want = -(-rows // (workgroups_per_group * waves))
    return int(min(_native.PANEL_ROWS, max(min(64, rows), want)))


def k1_plan(m, cus=256, max_groups=10):
    """(rows per panel, column groups) of the A image (K1, lsq_k1): as many
    column groups as keep the launch (groups x row blocks of 16 panels) within
    one workgroup per CU with panels as tall as they go (<= BSLS_PANEL_ROWS),
    i.e. full 64-row slices and fewer chunks per workgroup.  C3 (m = 100k):
    10 groups x 25 row blocks of 250-row panels, K1 42.8 us against 45.8 us
    for 8 x 32 of 196 rows (whose fourth slice held 4 rows).
    BSLS_K1_PLAN="groups,wg" overrides it (A/B timing of plans)."""
    plan = os.environ.get('BSLS_K1_PLAN')
    if plan:
        groups, wg = (int(v) for v in plan.split(','))
        return panel_rows(m, wg), groups
    rbs_min = -(-m // (16 * _native.PANEL_ROWS))
    groups = max(1, min(max_groups, cus // max(1, rbs_min)))
    rbs = max(rbs_min, cus // groups)
    return panel_rows(m, rbs), groups


def row_parts(nblocks, parts):
    """parts + 1 row-block bounds splitting K1's row blocks into `parts` runs."""
    parts = max(1, min(int(parts), int(nblocks)))
    return [int(v) for v in np.round(np.linspace(0, nblocks, parts + 1)).astype(np.int64)]


def set_images(S, A_pan, A_til, AT_pan, AT_til):
    """Point a problem or operator struct (bsls_bb_problem, bsls_lsq_op) at its
    image pair: A as panels (S.A) or tiles (S.At), A' as panels (S.AT) or
    tiles (S.ATt) -- of each pair the one that is not None."""
    if A_pan is not None:
        S.A = A_pan.struct
    else:
        S.At = A_til.struct
    if AT_pan is not None:
        S.AT = AT_pan.struct
    else:
        S.ATt = AT_til.struct
