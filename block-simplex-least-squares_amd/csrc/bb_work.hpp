// bb_work.hpp -- the BB engine's workspace: what bsls_bb_problem.work holds and
// where.  Part of bb.hip's translation unit.
#pragma once

namespace bsls {

struct BBWork {
    unsigned *tk1, *tk2, *tkf, *tkrb, *tk2rb;
    double *p1, *p2, *pf;
    int32_t *wsc;
    double *dz;   // z - z_prev, written by K3 (and the prologue) for the next K2
    uint64_t *hd; // K3's warm start: each pack's last run-head mask (<= n - nz packs),
                  //   two sets (slot 1: DORE's second projection, the line search's trials)
    int64_t hd_stride;
    unsigned long long *rmax;   // fx_sums: max|r| as bit patterns, RMAX_SLOTS words
    size_t bytes;
};

static size_t al16(size_t v) { return (v + 15) & ~(size_t)15; }

// fx_sums (bsls_bb_problem): max|r| for K2's fixed-point scale, kept on the
// device.  The bit patterns of non-negative doubles order as unsigned integers
// (a NaN's above inf's), so every workgroup that finishes rows of r folds its
// max into one of RMAX_SLOTS words with a 64-bit atomic max -- order-free,
// hence the same bits at the same r (as lsq.hip's lsq_xmax_kernel; an atomic
// per wave into 16 words took bb_k1_sum from 5.7 to 9.3 us at C3).  K2 reads
// the max over the slots; K3, between K2 and the next K1 finish, clears them.
constexpr int RMAX_SLOTS = 64;


static BBWork bb_layout(void *base, int64_t m, int64_t n, int64_t nz) {
    BBWork w{};
    char *p = (char *)base;
    size_t off = 0;
    w.tk1 = (unsigned *)(p + off);
    w.tk2 = (unsigned *)(p + off + TICKET_BYTES);
    w.tkf = (unsigned *)(p + off + 2 * TICKET_BYTES);
    off += al16(3 * TICKET_BYTES);
    w.tkrb = (unsigned *)(p + off);              // K1: one ticket per row block
    off += al16((size_t)(m / 16 + 2) * 4);
    w.tk2rb = (unsigned *)(p + off);             // K2 tiles: one ticket per row block (H >= 64)
    off += al16((size_t)(n / 64 + 2) * 4);
    // K1's per-row-block partials of ||r||^2: one per row block (two slots
    // reserved), and a row block holds >= 16 rows (16 panels of >= 1 row;
    // tiles of >= 64 rows)
    w.p1 = (double *)(p + off);
    off += al16((size_t)(m / 16 + 2) * 2 * 8);
    w.p2 = (double *)(p + off);
    off += al16((size_t)((n + PANEL_WAVES - 1) / PANEL_WAVES + 1) * 5 * 8);   // (5 sums fused)
    w.pf = (double *)(p + off);
    off += al16((size_t)((m + 255) / 256 + 1) * 2 * 8);
    w.wsc = (int32_t *)(p + off);
    off += al16((size_t)(nz > 0 ? nz : 1) * 4);
    w.dz = (double *)(p + off);
    off += al16((size_t)(nz > 0 ? nz : 1) * 8);
    w.hd = (uint64_t *)(p + off);
    w.hd_stride = n - nz > 0 ? n - nz : 1;
    off += al16((size_t)w.hd_stride * 2 * 8);
    w.rmax = (unsigned long long *)(p + off);
    off += al16((size_t)RMAX_SLOTS * 8);
    w.bytes = off;
    return w;
}

static BBWork bb_layout(const bsls_bb_problem &P) { return bb_layout(P.work, P.m, P.n, P.nz); }

}  // namespace bsls
