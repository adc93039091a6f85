// bb.hip -- fused z-space projected Barzilai-Borwein iteration on one GCD.
//
// Reference loop (python/BB.py:17-41) over main.solve_in_z's closures
// (python/main.py:53-65), stopping rule solvers.stopping (python/solvers.py:40-63):
//     g = N'A'(A N z + target);  dg = g - g_prev;  if sum(dg) == 0: break
//     t = (z - z_prev).dg / dg.dg;  z <- clip01(PAVA(z - t g));  fx = f(z); stop?
// One iteration here = three kernels, all HBM-bound, no host round trip:
//   K2  g = N'(A' r) with an explicit A' in panel format (panels.hpp): each
//       workgroup stages r chunk by chunk into LDS and sums its rows there in
//       CSR order (bit-identical to SciPy's csr_matvec); each panel carries the
//       next panel's first row, so the adjacent difference N'w = w_i - w_{i+1}
//       stays in the wave; fused: dg, the four BB sums, the store of g.
//   K3  t from the sums; per z-block PAVA (v1 pooling order, bit-identical to
//       isotonic_regression.h:13-58) + clip to [0,1] + the vector N z (per-block
//       differences, last entry -z_last), one wave per pack of whole blocks
//       (<= 64 entries, one lane per entry, pava_wave.hpp).  N is never
//       materialised.
//   K1  r = A (N z) + target, target = A x0 - b, exactly the reference's
//       A.dot(N.dot(z)) + target.  A in panel format with its column chunks
//       split into G groups (device.k1_plan: C3 10), group = blockIdx % G;
//       each workgroup stages its group's slice of x chunk by chunk into LDS
//       and publishes one partial per (row, group); the last of a row
//       block's G workgroups sums them in group order, adds target,
//       ||r||^2 (next gradient's residual AND f(z)); the last row block runs
//       the stopping test.
//   For a scaled incidence A (bsls_utils.py:494) the values are not stored:
//   K3 writes colv * (N z) (the same products SciPy forms), K2 multiplies by
//   the row's colv.
// Sparse row blocks (C5: 1M links, ~0.3 entries per row per panel chunk) take
// the streamed-tile format instead of the panels for K1 and/or K2 (tiles.hpp;
// bb_k1t / bb_k2t, chosen per matrix by the host: P.At / P.ATt).
// Every cross-workgroup sum of a reduction (the BB sums, ||r||^2) is reduced in
// a fixed order by the last-arriving workgroup (bsls_common.hpp last_block_sum).
// The SpMV row sums are fixed-order on the panels and the thread-stream tiles
// (BBEngine(deterministic=True): runs bit-reproducible); the dealt tiles, the
// default, add them with LDS atomics, so their rounding varies run to run at
// the 1e-16 level -- unless bsls_bb_problem.fx_sums (BBEngine(fixed_sums=True))
// has them summed as integers in fixed point, which is order-free.
// Scalars live in device memory (scal[]); the host only polls them.
#include "pava.hpp"
#include "pava_long.hpp"
#include "pava_wave.hpp"
#include "panels.hpp"
#include "tiles.hpp"

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

// column scale i (bsls_bb_problem.colv_codec: exact narrow copies read instead
// of the doubles)
__device__ __forceinline__ double colv_at(const bsls_bb_problem &P, int64_t i) {
    if (P.colv_codec == 2) return (double)reinterpret_cast<const _Float16 *>(P.colv_n)[i];
    if (P.colv_codec == 1) return (double)reinterpret_cast<const float *>(P.colv_n)[i];
    return P.colv[i];
}

// the same with the codec known at compile time (the hot kernels are
// instantiated per codec: a runtime switch among three loads inside K2's
// batched epilogue kept its loads from being in flight together)
template <int CV>
__device__ __forceinline__ double colv_t(const bsls_bb_problem &P, int64_t i) {
    if constexpr (CV == 2) return (double)reinterpret_cast<const _Float16 *>(P.colv_n)[i];
    else if constexpr (CV == 1) return (double)reinterpret_cast<const float *>(P.colv_n)[i];
    else return P.colv[i];
}

// The hand-offs between the iteration's kernels (the measurements:
// profiles/handoff_ab.txt): bb_k1_sum issues its first rows'
// loads before its stop test resolves (one memory round trip instead of two)
// and takes two adjacent rows per thread with 16-B loads and stores where m
// and the first row are even; the split K1's partials leave through
// write-through stores (as K3's z / dz / x): no dirty lines for the kernel's
// end to flush before bb_k1_sum starts (the same for K2's g and bb_k1_sum's r
// measured slower and is not in the source).  The forms these replaced, each
// behind an A/B switch of its own, last existed at commit 36c7740.
// BSLS_PHASE_STAMPS: a diagnostic build, never the product library -- wave 0
// of every workgroup of bb_k2t, bb_k3, bb_k1t and bb_k1_sum keeps
// s_memrealtime at its phase boundaries and leaves them in a buffer of this
// build's own (tools/phase_times.py reads it through bsls_phase_read).
#ifdef BSLS_PHASE_STAMPS
constexpr int PH_SLOTS = 8, PH_WGS = 4096;
enum { PH_K2 = 0, PH_K3 = 1, PH_K1 = 2, PH_SUM = 3 };
__device__ unsigned long long bsls_phase_buf[4][PH_WGS][PH_SLOTS];
#define PH_DECL unsigned long long ph_t[PH_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PH(s) (ph_t[s] = __builtin_amdgcn_s_memrealtime())
#define PH_FLUSH(k)                                                            \
    do {                                                                       \
        if (threadIdx.x == 0 && blockIdx.x < PH_WGS)                           \
            for (int ph_s = 0; ph_s < PH_SLOTS; ++ph_s)                        \
                bsls_phase_buf[k][blockIdx.x][ph_s] = ph_t[ph_s];              \
    } while (0)
#else
#define PH_DECL
#define PH(s) ((void)0)
#define PH_FLUSH(k) ((void)0)
#endif

// 8-B write-through (sc1) store through a buffer resource: the line
// leaves L2 at once instead of as a dirty line at the kernel's end (as
// proj.hip's store-out).  Lanes whose offset is past the resource's bytes are
// dropped by the hardware.
typedef double bb_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void wt_store_f64(const __amdgpu_buffer_rsrc_t &rs, int off,
                                             double v) {
    __builtin_amdgcn_raw_buffer_store_b64(
        __builtin_bit_cast(HIP_vector_type<unsigned, 2>::Native_vec_, v), rs, off, 0, 16);
}
// the resource over `count` doubles at p (count * 8 < 2^31 by the callers)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(double *p, int64_t count) {
    return __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)(count * 8), 0x00020000);
}

// solvers.py:40-63 on iteration iter's g.g and dg.dg (the all-reduced sums)
__device__ __forceinline__ int bb_stop_reason(const bsls_bb_problem &P, int64_t iter, double fx,
                                              double gg, double dgdg) {
    if (iter >= P.max_iter) return BSLS_STOP_MAXITER;
    if (P.early_exit) {
        const double gn = sqrt(gg);
        if (gn * gn <= P.opt_tol * (1 + fabs(fx))) return BSLS_STOP_GRAD;
        if (sqrt(dgdg) == 0) return BSLS_STOP_DG;
    }
    return 0;
}

__device__ __forceinline__ void bb_stop_check(const bsls_bb_problem &P, int64_t iter, double fx) {
    double *s = P.scal;
    const int reason = bb_stop_reason(P, iter, fx, s[BSLS_S_GG], s[BSLS_S_DGDG]);
    if (reason) s[BSLS_S_STOP] = (double)reason;
}

__device__ __forceinline__ void bb_record_f(const bsls_bb_problem &P, int64_t iter, double rr,
                                            bool iterating) {
    double *s = P.scal;
    const double nr = sqrt(rr);
    const double fx = 0.5 * (nr * nr);  // 0.5 * la.norm(r)**2, main.py:53
    s[BSLS_S_RR] = rr;
    s[BSLS_S_FX] = fx;
    if (iterating) {
        s[BSLS_S_ITER] = (double)iter;
        s[BSLS_S_ZBUF] = (double)(iter & 1);
        bb_stop_check(P, iter, fx);
    }
}

// A column shard's r in 64-bit fixed point (bsls_bb_problem.r_fx > 0): the
// stored word is the int64 llrint(r * r_fx).  r_fx_of(v): v as that word.
__device__ __forceinline__ double r_fx_of(const bsls_bb_problem &P, double v) {
    return __longlong_as_double(__double2ll_rn(v * P.r_fx));
}
__device__ __forceinline__ double r_load(const bsls_bb_problem &P, int64_t i) {
    if (P.r_fx > 0.0) return (double)__double_as_longlong(P.r[i]) * (1.0 / P.r_fx);
    return P.r[i];
}

__device__ __forceinline__ unsigned long long abs_bits(double v) {
    return (unsigned long long)__double_as_longlong(fabs(v));
}
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) {
    return a > b ? a : b;
}
// a thread's max (bit pattern) -> its wave's -> its workgroup's -> one slot
// (every thread of the workgroup calls it: one barrier)
__device__ __forceinline__ void rmax_fold(unsigned long long *slots, unsigned long long mb) {
    __shared__ unsigned long long wmax[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mb = umax64(mb, __shfl_xor(mb, o, WAVE));
    if (lane_id() == 0) wmax[threadIdx.x / WAVE] = mb;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x / WAVE); ++k) mb = umax64(mb, wmax[k]);
        if (mb) atomicMax(slots + blockIdx.x % RMAX_SLOTS, mb);
    }
}
__device__ __forceinline__ double rmax_of(const unsigned long long *slots) {
    unsigned long long b = 0ull;
#pragma unroll
    for (int k = 0; k < RMAX_SLOTS; ++k) b = umax64(b, slots[k]);
    return __longlong_as_double((long long)b);
}

// The fixed-point scale of a walk whose rows' sum |terms| stays within B:
// B < 2^e (frexp), fxs = 2^(50 - e) puts every row within +-2^50, inv undoes
// it.  e is kept >= -900 so the scale stays finite (a larger bound is still a
// bound).  Returns whether B is no finite bound (a NaN or inf in what it was
// made from): the rows are then NaN, as float sums would make them.
__device__ __forceinline__ bool fx_scale(double B, double &fxs, double &inv) {
    int ex = 0;
    if (B > 0.0 && B <= 1.7976931348623157e308) (void)frexp(B, &ex);
    if (ex < -900) ex = -900;
    fxs = ldexp(1.0, 50 - ex);
    inv = ldexp(1.0, ex - 50);
    return !(B <= 1.7976931348623157e308);
}
// row lr's two words back to a double (tiles.hpp fx_value).  Terms within
// the bound keep the high word inside +-2^51; one outside it holds a term
// beyond the bound, a NaN or an inf (their bit patterns add as huge integers):
// NaN, which the solvers' checks then see.
__device__ __forceinline__ double fx_row(const double *rows, int lr, int lo_off, double inv,
                                         double inv_lo, bool bad) {
    const long long hi = reinterpret_cast<const long long *>(rows)[lr];
    if (bad || hi > (1LL << 51) || hi < -(1LL << 51)) return __builtin_nan("");
    return fx_value(rows, lr, lo_off, inv, inv_lo);
}

// A column-sharded rank other than the one adding target (shard_role 2)
// writes r = 0 for its rows once the run has stopped: its K1 no longer forms a
// partial, and the all-reduce must leave the final residual (held by the
// shard_role 1 rank, whose r is not touched) as it was.
__device__ __forceinline__ void k1_stopped_rows(const bsls_bb_problem &P, int64_t r0, int64_t r1,
                                                int64_t t0, int64_t stride) {
    if (P.shard_role != 2) return;
    for (int64_t row = r0 + t0; row < r1; row += stride) P.r[row] = 0.0;
}

// bsls_bb_problem.roww, a row's value o under its weight w: what r stores (an
// exact +0.0 for a held-out row, w == 0, whatever o is -- selected out, not
// multiplied, so a NaN or inf there reaches `held` only), its share w o^2 of
// the objective into sq and, held out, o^2 into held.
__device__ __forceinline__ double k1_weigh(double o, double w, double &sq, double &held) {
    const bool out = (w == 0.0);
    const double wo = out ? 0.0 : w * o;
    sq += out ? 0.0 : o * wo;
    held += out ? o * o : 0.0;
    return wo;
}

// K1's finish for row block rb (rows [r0, r1)), run by one workgroup: r =
// the G partials of each row summed in group order (from rpart, or from LDS
// `local` when the block had one group) + target; its share of ||r||^2 goes
// to the last row block, which records f and runs the stopping test.
// FX (fx_sums): |r| of the rows folded into rmax for the next K2's scale.
// RW (bsls_bb_problem.roww): the weighted finish, k1_weigh.
template <bool ADD, bool REDUCE, bool FX = false, bool RW = false>
__device__ __forceinline__ void k1_finish(const bsls_bb_problem &P, int64_t iter, bool iterating,
                                          int64_t rb, unsigned nrb, int64_t r0, int64_t r1,
                                          int64_t G, const double *local, double *part,
                                          unsigned *ticket, double *red,
                                          unsigned long long *rmax = nullptr) {
    static_assert(!RW || (ADD && !FX), "weights: the finishes that add target, float sums");
    constexpr int NS = RW ? 2 : 1;   // (RW: [1] the held-out rows' o^2)
    double sq[NS] = {};
    unsigned long long mb = 0ull;
    if (local) {
        for (int64_t row = r0 + threadIdx.x; row < r1; row += blockDim.x) {
            double o = local[row - r0];
            if (ADD) o += P.target[row];
            if constexpr (RW) {
                P.r[row] = k1_weigh(o, P.roww[row], sq[0], sq[NS - 1]);
            } else {
                P.r[row] = o;
                sq[0] += o * o;
            }
            if constexpr (FX) mb = umax64(mb, abs_bits(o));
        }
    } else {
        // up to RPT rows per thread, every partial load of them in flight at once
        constexpr int RPT = 4;
        for (int64_t row0 = r0 + threadIdx.x; row0 < r1; row0 += RPT * blockDim.x) {
            double v[RPT][8];
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const int64_t row = row0 + (int64_t)u * blockDim.x;
                const int64_t rr = row < r1 ? row : r0;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    v[u][c] = (c < G) ? __hip_atomic_load(&P.rpart[c * P.m + rr], __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT)
                                      : 0.0;
            }
#pragma unroll
            for (int u = 0; u < RPT; ++u) {
                const int64_t row = row0 + (int64_t)u * blockDim.x;
                if (row >= r1) continue;
                double o = v[u][0];
#pragma unroll
                for (int c = 1; c < 8; ++c)
                    if (c < G) o += v[u][c];
                for (int64_t c = 8; c < G; ++c)
                    o += __hip_atomic_load(&P.rpart[c * P.m + row], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                if (ADD) o += P.target[row];
                if constexpr (RW) {
                    P.r[row] = k1_weigh(o, P.roww[row], sq[0], sq[NS - 1]);
                } else {
                    P.r[row] = o;
                    sq[0] += o * o;
                }
                if constexpr (FX) mb = umax64(mb, abs_bits(o));
            }
        }
    }
    if constexpr (FX) rmax_fold(rmax, mb);
    if (!REDUCE) return;
    block_sum<NS>(sq, red);
    double tot[NS];
    if (last_of_sum<NS>(sq, part, (unsigned)rb, nrb, ticket, tot, red) && threadIdx.x == 0) {
        if constexpr (RW) P.scal[BSLS_S_HELD] = tot[NS - 1];
        bb_record_f(P, iter, tot[0], iterating);
    }
}

// K1: workgroup (group g = blockIdx % ngroups, panels 16 rb .. 16 rb + 15)
// stages x chunk by chunk (the group's columns) and publishes, per row, the
// sum over the group's columns in rpart[g][row] (sc1: visible across XCDs).
// The last of the row block's ngroups workgroups to arrive sums the partials
// in group order (+ target), writes r, and (REDUCE) hands its share of
// ||r||^2 to the last row block, which records f and runs the stopping test.
template <int MODE, bool ITER, bool ADD, bool REDUCE, bool RW = false>
__global__ __launch_bounds__(1024) void bb_k1(bsls_bb_problem P, int64_t iter, unsigned *tkrb,
                                              double *part, unsigned *ticket, int64_t rb_base) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int row_last;
    const bsls_panels &M = P.A;
    const int64_t G = M.ngroups;
    const int64_t g = blockIdx.x % G, rb = rb_base + blockIdx.x / G;
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        if (g == 0) {
            const int64_t r0 = rb * PANEL_WAVES * M.prow;
            const int64_t r1 = (r0 + PANEL_WAVES * M.prow < P.m) ? r0 + PANEL_WAVES * M.prow : P.m;
            k1_stopped_rows(P, r0, r1, threadIdx.x, blockDim.x);
        }
        return;
    }
    const int wv = threadIdx.x / WAVE, lane = lane_id();
    const int64_t panel = rb * PANEL_WAVES + wv;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const double sc[4] = {0.0, 0.0, 0.0, 0.0};
    panel_chunks<MODE>(M, rb, wv, M.group_chunk[g], M.group_chunk[g + 1], P.x, lds, s, sc);
    if (panel < M.npanels) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = 64 * q + lane;
            const int64_t row = panel * M.prow + i;
            if (i < M.prow && row < P.m)
                __hip_atomic_store(&P.rpart[g * P.m + row], s[q], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (!rowblock_last(tkrb, rb, G, &row_last)) return;
    const int64_t r0 = rb * PANEL_WAVES * M.prow;
    const int64_t r1 = (r0 + PANEL_WAVES * M.prow < P.m) ? r0 + PANEL_WAVES * M.prow : P.m;
    const unsigned nrb = (unsigned)((M.npanels + PANEL_WAVES - 1) / PANEL_WAVES);
    k1_finish<ADD, REDUCE, false, RW>(P, iter, ITER, rb, nrb, r0, r1, G, nullptr, part, ticket,
                                      lds);
}

// A K1 tile launch with several column groups ends once its partials are
// stored, and bb_k1_sum finishes the rows in a launch of its own -- the kernel
// boundary replaces an in-kernel hand-off (partials drained, a ticket per row
// block, the last arriver's loads, a second ticket for ||r||^2: a chain of
// dependent round trips that took ~half of C3's K1; that finish inside bb_k1t
// last existed at commit 36c7740).
//
// K1's finish as its own launch (rows [r0, r1), one thread per row): r = the G
// partials in group order (+ target, ADD), ||r||^2 and f by the last block
// (REDUCE), as k1_finish.
// W = 2 (the launch: m and r0 even, r1 - r0 >= 2, 16-B aligned arrays): item
// idx of a thread is the row pair r0 + 2 idx, + 1, loaded and stored as 16
// bytes; the single last row of an odd r1 - r0 is the grid's last thread's,
// after its pairs.  W = 1: an item is a row.  A thread's first item is loaded
// at a clamped index before the stop test (the flag's round trip and the
// rows' run together; nothing is stored before the test).
template <int W>
struct K1SumVec {
    typedef double type;
};
template <>
struct K1SumVec<2> {
    typedef bb_d2 type;
};
__device__ __forceinline__ double k1_sq(double o) { return o * o; }
__device__ __forceinline__ double k1_sq(bb_d2 o) { return o.x * o.x + o.y * o.y; }
__device__ __forceinline__ unsigned long long k1_abs(double o) { return abs_bits(o); }
__device__ __forceinline__ unsigned long long k1_abs(bb_d2 o) {
    return umax64(abs_bits(o.x), abs_bits(o.y));
}

__device__ __forceinline__ bb_d2 k1_weigh(bb_d2 o, bb_d2 w, double &sq, double &held) {
    bb_d2 wo;
    wo.x = k1_weigh(o.x, w.x, sq, held);
    wo.y = k1_weigh(o.y, w.y, sq, held);
    return wo;
}

// FX (fx_sums): |r| of the rows folded into rmax, as k1_finish
// RW (roww): the weighted finish, as k1_finish (W = 2: the pair's weights as
// one 16-B load beside target's)
template <bool ITER, bool ADD, bool REDUCE, int W = 1, bool FX = false, bool RW = false>
__global__ __launch_bounds__(256) void bb_k1_sum(bsls_bb_problem P, int64_t iter, int64_t G,
                                                 int64_t r0, int64_t r1, double *part,
                                                 unsigned *ticket,
                                                 unsigned long long *rmax = nullptr) {
    static_assert(!RW || (ADD && !FX), "weights: the finishes that add target, float sums");
    constexpr int NS = RW ? 2 : 1;   // (RW: [1] the held-out rows' o^2)
    typedef typename K1SumVec<W>::type vec;
    __shared__ double red[8];   // (NS doubles per wave)
    PH_DECL;
    PH(0);
    const double stop = ITER ? P.scal[BSLS_S_STOP] : 0.0;
    // grid-stride items: with REDUCE the launch is capped at K1_SUM_GRID
    // workgroups (one per 256 rows made 3.9k arrivals at the ||r||^2 tickets
    // at m = 1M: 12.5 us against 4.6 without the reduction)
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t idx = t0;
    const int64_t ni = (r1 - r0) / W;   // whole items (>= 1)
    vec v[8], tg;
    [[maybe_unused]] vec wt;
    auto load = [&](int64_t i) {
        const int64_t row = r0 + W * (i < ni ? i : ni - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c)
            v[c] = (c < G) ? *reinterpret_cast<const vec *>(&P.rpart[c * P.m + row]) : vec{};
        tg = ADD ? *reinterpret_cast<const vec *>(&P.target[row]) : vec{};
        if constexpr (RW) wt = *reinterpret_cast<const vec *>(&P.roww[row]);
    };
    load(idx);
    if (ITER && stop != 0.0) {
        k1_stopped_rows(P, r0, r1, t0, gs);
        return;
    }
    PH(1);
    double sq[NS] = {};
    unsigned long long mb = 0ull;
    while (idx < ni) {
        const int64_t row = r0 + W * idx;
        vec o = v[0];
#pragma unroll
        for (int c = 1; c < 8; ++c)
            if (c < G) o += v[c];
        for (int64_t c = 8; c < G; ++c) o += *reinterpret_cast<const vec *>(&P.rpart[c * P.m + row]);
        if (ADD) o += tg;
        if constexpr (RW) {
            *reinterpret_cast<vec *>(&P.r[row]) = k1_weigh(o, wt, sq[0], sq[NS - 1]);
        } else {
            *reinterpret_cast<vec *>(&P.r[row]) = o;
            sq[0] += k1_sq(o);
        }
        if constexpr (FX) mb = umax64(mb, k1_abs(o));
        idx += gs;
        if (idx < ni) load(idx);
    }
    if (W == 2 && ((r1 - r0) & 1) && t0 == gs - 1) {
        const int64_t row = r1 - 1;
        double o = P.rpart[row];
        for (int64_t c = 1; c < G; ++c) o += P.rpart[c * P.m + row];
        if (ADD) o += P.target[row];
        if constexpr (RW) {
            P.r[row] = k1_weigh(o, P.roww[row], sq[0], sq[NS - 1]);
        } else {
            P.r[row] = o;
            sq[0] += o * o;
        }
        if constexpr (FX) mb = umax64(mb, abs_bits(o));
    }
    PH(2);
    if constexpr (FX) rmax_fold(rmax, mb);
    if (!REDUCE) {
        PH_FLUSH(PH_SUM);
        return;
    }
    block_sum<NS>(sq, red);
    double tot[NS];
    if (last_block_sum<NS>(sq, part, ticket, tot, red) && threadIdx.x == 0) {
        if constexpr (RW) P.scal[BSLS_S_HELD] = tot[NS - 1];
        bb_record_f(P, iter, tot[0], ITER);
    }
    PH(3);
    PH_FLUSH(PH_SUM);
}

// K1 with global atomics (BSLS_K1_ATOMIC): rows [r0, r1) of r start as
// target (ADD) or 0 for the groups to add into; once the run has stopped, the
// shard_role 1 rank keeps its r (the final residual) and the others write 0.
template <bool ITER, bool ADD>
__global__ __launch_bounds__(256) void bb_k1_init(bsls_bb_problem P, int64_t r0, int64_t r1) {
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        k1_stopped_rows(P, r0, r1, t0, gs);
        return;
    }
    for (int64_t row = r0 + t0; row < r1; row += gs) {
        const double v = ADD ? P.target[row] : 0.0;
        P.r[row] = (P.r_fx > 0.0) ? r_fx_of(P, v) : v;
    }
}

// K1 on a tile image (tiles.hpp): workgroup (rb, g) sums its rows over group
// g's columns of x in LDS; with one group it finishes the block itself,
// otherwise it leaves its partials in rpart for bb_k1_sum (or, ATOM, adds them
// into r).
// (__launch_bounds__' second argument: one workgroup of 1024 threads per CU,
// the whole register file for it.  Two per CU -- registers capped so two
// tiles share one -- measured slower, profiles/r05_k1_two_tiles_per_cu.log;
// that variant build last existed at commit 36c7740.)
// FX (bsls_bb_problem.fx_sums, dealt images, never ATOM): the walk keeps each
// row's sum in two integer words (tiles.hpp fx_add: order-free), scaled from
// the caller's bound fx_a1 * x_bound; each row is converted once after the
// walk, and what follows -- the finish, or the partials and bb_k1_sum -- is the
// float form's, already ordered.
// RW (roww, never ATOM or FX): the one-group finish weighted, as k1_finish;
// with several groups the kernel is RW = false's and bb_k1_sum weighs.
template <int MODE, bool ITER, bool ADD, bool REDUCE, bool ATOM = false, bool FX = false,
          bool RW = false>
__global__ __launch_bounds__(1024, 1) void bb_k1t(bsls_bb_problem P, int64_t iter, double *part,
                                                  unsigned *ticket, int64_t rb_base,
                                                  unsigned long long *rmax = nullptr) {
    static_assert(!(FX && ATOM), "the fixed-point sums finish through the ordered partials");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[32];   // (k1_finish: 2 doubles per wave)
    const bsls_tiles &T = P.At;
    PH_DECL;
    PH(0);
    int64_t rb, g;
    tile_map(T, blockIdx.x, gridDim.x / T.ngroups, rb, g);
    rb += rb_base;
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        // (several groups: bb_k1_sum zeroes the rows; ATOM: bb_k1_init did)
        if (!ATOM && g == 0 && T.ngroups == 1)
            k1_stopped_rows(P, rb * T.H, (rb * T.H + T.H < P.m) ? rb * T.H + T.H : P.m,
                            threadIdx.x, blockDim.x);
        return;
    }
    const int HR = (int)tile_lds_doubles(T, FX);   // (FX: two words per row)
    double fxs = 1.0, inv = 1.0;
    bool bad = false;
    if constexpr (FX) bad = fx_scale(P.fx_a1 * P.x_bound, fxs, inv);
    // (the clear and its barrier: under the dealt walk's first loads, tiles.hpp
    // tile_walk_dealt's `mid`)
    PH(1);
    auto clear = [&]() {
        PH(2);
        for (int i = threadIdx.x; i < HR; i += blockDim.x) lds[i] = 0.0;   // (integer 0 too)
        __syncthreads();
        PH(3);
    };
    tile_walk_any<MODE, FX>(T, rb, g, P.x, lds, nullptr, fxs, 1.0, clear);
    PH(4);
    __syncthreads();
    PH(5);
    const int64_t G = T.ngroups;
    const int64_t r0 = rb * T.H, r1 = (r0 + T.H < P.m) ? r0 + T.H : P.m;
    if constexpr (FX) {
        // each row's words to its double, in place (the low words sit past the rows)
        const int lo_off = (int)(T.H + T.halo + 1);
        const double inv_lo = ldexp(inv, -fx_lo_shift(T.cols));
        for (int i = threadIdx.x; i < (int)(r1 - r0); i += blockDim.x)
            lds[i] = fx_row(lds, i, lo_off, inv, inv_lo, bad);
        __syncthreads();
    }
    if (G == 1) {
        k1_finish<ADD, REDUCE, FX, RW>(P, iter, ITER, rb, (unsigned)T.nrb, r0, r1, 1, lds, part,
                                       ticket, red, rmax);
        PH(6);
        PH_FLUSH(PH_K1);
        return;
    }
    if (ATOM) {
        // r was set to target / 0 by bb_k1_init: every group adds its sums
        // (global f64 atomics; the order over groups varies run to run, as the
        // dealt walk's LDS sums do)
        // (r_fx: the sums as int64 words, added as integers -- order-free)
        if (P.r_fx > 0.0) {
            for (int64_t row = r0 + threadIdx.x; row < r1; row += blockDim.x)
                atomicAdd(reinterpret_cast<unsigned long long *>(&P.r[row]),
                          (unsigned long long)__double2ll_rn(lds[row - r0] * P.r_fx));
        } else {
            for (int64_t row = r0 + threadIdx.x; row < r1; row += blockDim.x)
                unsafeAtomicAdd(&P.r[row], lds[row - r0]);
        }
        return;
    }
    // the partials only, through write-through stores; bb_k1_sum (next in the
    // stream) finishes the rows
    // (a row block's sums fit LDS: the offsets stay far below 2^31)
    const __amdgpu_buffer_rsrc_t rp = wt_rsrc(P.rpart + g * P.m + r0, r1 - r0);
    for (int64_t row = r0 + threadIdx.x; row < r1; row += blockDim.x)
        wt_store_f64(rp, (int)(row - r0) * 8, lds[row - r0]);
    PH(6);
    PH_FLUSH(PH_K1);
}

// K2's epilogue rows per thread per batch (K2E; round 6: 4 -- C3's 3.8 rows
// per thread fit one batch, C5's 19 run five at the speed of three of 8, and
// the kernel drops from 124 to 86 VGPRs: C3 13.2k -> 13.4k it/s, C5 and the
// 8-way C5 rank the same, tools/gpu_r06k.sh; A/B builds: BSLS_K2E.  Loading
// the first batch's z indices and scales before the walk instead, to land
// under it, measured no gain: 13.2k)
#ifndef BSLS_K2E
#define BSLS_K2E 4
#endif

// K2 on a tile image: w = A'r for row block rb (+ its halo row) in LDS, summed
// over r's column groups (one group: in CSR order, bit-identical to SciPy;
// several: partials in wpart, summed in group order by the block's last
// workgroup); then g = N'w, dg and the four BB sums, as bb_k2.  MODE 1: stored
// values; MODE 2: scaled incidence, each term colv[row] * r_i (SciPy's
// product; the rows' scales sit in LDS beside the sums); MODE 3: scaled
// incidence with several groups (no bit pattern to keep): w_i = colv_i *
// sum r, one product per row after the group sums, and the whole LDS for rows.
// FUSE (stage 8, column-sharded): every workgroup first sums r_i^2 over its
// slice of r (already the all-reduced residual; slice blockIdx of nrb * G, so
// the linear read also warms the caches the walk gathers r from), the
// finishing workgroup of row block rb adds its groups' slices in group order
// (through wpart's tail, see bsls_bb_problem.wpart), and the last one records
// f and runs the stopping test of iteration iter - 1 before it stores this
// iteration's sums.  (At the end of the finishing workgroups only, the slice
// sums cost 13 us of tail in the 8-way rehearsal.)
// FUSE 2 (stage 10, the sliced schedule): the same r^2, but over this rank's
// rows [P.rr_lo, P.rr_hi) of r only (1/world of m: the other ranks sum the
// rest), stored with the sums as scal[RR] for the all-reduce; the last
// workgroup keeps iteration iter - 1's sums in scal[PSUMDG..PGG] for the
// stop test that follows the all-reduce (stage 12), instead of testing.
// K2 of a stopped sharded run: the driver still all-reduces scal[SUMDG..RR]
// after every K2 it enqueues, so the shard_role 2 ranks zero their copy and
// the sum leaves role 1's -- the stop iteration's sums -- instead of world
// times them, growing with every iteration enqueued past the stop
// (fuse 2 all-reduces scal[RR] with the four sums)
template <int FUSE>
__device__ __forceinline__ void k2_stopped_sums(const bsls_bb_problem &P) {
    if (P.shard_role == 2 && blockIdx.x == 0 && threadIdx.x == 0)
        for (int q = 0; q < (FUSE == 2 ? 5 : 4); ++q) P.scal[BSLS_S_SUMDG + q] = 0.0;
}

// K2's last workgroup, one thread: the reduced sums tot into scal (bb_k2t and
// bb_k2).  FUSE 1 first records f and runs the stopping test of iteration
// iter - 1 on tot[4] = ||r||^2; FUSE 2 keeps iteration iter - 1's sums in
// scal[PSUMDG..PGG] and stores tot[4] as scal[RR].
template <int FUSE>
__device__ __forceinline__ void k2_store_sums(const bsls_bb_problem &P, int64_t iter,
                                              const double (&tot)[FUSE ? 5 : 4]) {
    if constexpr (FUSE == 1) {
        bb_record_f(P, iter - 1, tot[4], iter - 1 > 0);
        // stopped at iter - 1: keep that iteration's sums (what the
        // unfused schedule leaves in scal); g[iter & 1], written by this
        // launch, is the other buffer -- the stopping iterate's g is untouched
        if (P.scal[BSLS_S_STOP] != 0.0) {
            // (the sums all-reduced after this launch: as k2_stopped_sums)
            if (P.shard_role == 2)
                for (int q = 0; q < 4; ++q) P.scal[BSLS_S_SUMDG + q] = 0.0;
            return;
        }
    }
    if constexpr (FUSE == 2) {
        double *sc = P.scal;
        for (int q = 0; q < 4; ++q) sc[BSLS_S_PSUMDG + q] = sc[BSLS_S_SUMDG + q];
        sc[BSLS_S_RR] = tot[4];
    }
    P.scal[BSLS_S_SUMDG] = tot[0];
    P.scal[BSLS_S_DZDG] = tot[1];
    P.scal[BSLS_S_DGDG] = tot[2];
    P.scal[BSLS_S_GG] = tot[3];
}

// gsel >= 0 (bsls_bb_k2_part): only column group gsel, one workgroup per row
// block -- the link-part pipeline of the sharded schedule launches the groups
// one by one, each as soon as its rows of r are all-reduced.  The launches
// are ordered on one stream, so the roles are fixed: groups < G - 1 leave
// their partial row sums (and r^2 slices) in wpart and return; the last group
// adds them in group order and runs the epilogue -- no tickets.  Its slice of
// ||r||^2 stays inside its own link range (rows of r the earlier parts'
// exchanges have not finished may not be read).
// FX (bsls_bb_problem.fx_sums: gsel < 0, FUSE 0, MODE 1 / 3, dealt images):
// the walk's row sums in two integer words (tiles.hpp fx_add: order-free),
// scaled from fx_a2 * max|r| (rmax: the slots K1's finish keeps); after the
// walk the rows -- the halo row too -- are converted in place to doubles (one
// group of a scaled incidence: to w_i = colv_i * sum, the epilogue's product),
// and the group hand-off and the N' epilogue run as in the float form.
template <int MODE, bool ITER, int FUSE = 0, int CV = 0, bool FX = false>
__global__ __launch_bounds__(1024) void bb_k2t(bsls_bb_problem P, const double *__restrict__ dzv,
                                               const double *__restrict__ gp,
                                               double *__restrict__ gout, double *part,
                                               unsigned *ticket, unsigned *tk2rb, int64_t iter,
                                               int gsel, const unsigned long long *rmax = nullptr) {
    static_assert(!FX || (FUSE == 0 && (MODE == 1 || MODE == 3)), "FX: the single-GCD dealt K2");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[5 * 16];
    __shared__ int row_last;
    PH_DECL;
    PH(0);
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        if (gsel < 0 || gsel == P.ATt.ngroups - 1) k2_stopped_sums<FUSE>(P);
        return;
    }
    PH(1);
    const bsls_tiles &T = P.ATt;
    int64_t rb, g;
    if (gsel >= 0) {
        rb = blockIdx.x;
        g = gsel;
    } else {
        tile_map(T, blockIdx.x, T.nrb, rb, g);
    }
    const int HR = (int)tile_lds_doubles(T, false);
    double *rows = lds;
    double *rc = lds + HR;
    const int64_t i0 = rb * T.H;
    const int64_t nloc = (i0 + T.H + 1 <= P.n) ? T.H + 1 : P.n - i0;   // rows incl. the halo
    const int64_t G = T.ngroups;
    double rr[1] = {0.0};
    if constexpr (FUSE) {
        if (ITER) {
            // the slice's loads RR at a time, all in flight (a load-then-add
            // loop waited out one memory latency per element, at the start of
            // every workgroup); same left-to-right order, padding adds +0
            constexpr int RR = 4;
            const int64_t ns = T.nrb * G, sl = rb * G + g;
            const bool cut = FUSE == 2 && P.rr_hi > P.rr_lo;
            int64_t lo = cut ? P.rr_lo : 0, span = (cut ? P.rr_hi : P.m) - lo;
            int64_t q0 = lo + sl * span / ns, q1 = lo + (sl + 1) * span / ns;
            if (gsel >= 0) {
                // this part's link range, cut to the rank's slice, over the row blocks
                const int64_t a = T.group_col[g] > lo ? T.group_col[g] : lo;
                const int64_t b = T.group_col[g + 1] < lo + span ? T.group_col[g + 1] : lo + span;
                const int64_t w = b > a ? b - a : 0;
                q0 = a + rb * w / T.nrb;
                q1 = a + (rb + 1) * w / T.nrb;
            }
            for (int64_t i0 = q0 + threadIdx.x; i0 < q1; i0 += RR * (int64_t)blockDim.x) {
                double v[RR];
#pragma unroll
                for (int q = 0; q < RR; ++q) {
                    const int64_t i = i0 + (int64_t)q * blockDim.x;
                    v[q] = (i < q1) ? r_load(P, i) : 0.0;
                }
#pragma unroll
                for (int q = 0; q < RR; ++q) rr[0] += v[q] * v[q];
            }
        }
    }
    // (the clear and its barrier: under the dealt walk's first loads, tiles.hpp
    // tile_walk_dealt's `mid`)
    auto clear = [&]() {
        PH(2);
        for (int i = threadIdx.x; i < HR; i += blockDim.x) {
            rows[i] = 0.0;
            if (MODE == 2) rc[i] = (i < nloc) ? colv_t<CV>(P, i0 + i) : 0.0;
            if (FX) rc[i] = 0.0;   // (the low words: integer 0)
        }
        __syncthreads();
        PH(3);
    };
    if constexpr (FX) {
        double fxs, inv;
        const bool bad = fx_scale(P.fx_a2 * rmax_of(rmax), fxs, inv);
        tile_walk_any<(MODE == 3 ? 0 : MODE), true>(T, rb, g, P.r, rows, rc, fxs, 1.0, clear);
        PH(4);
        __syncthreads();
        const double inv_lo = ldexp(inv, -fx_lo_shift(T.cols));
        for (int i = threadIdx.x; i < (int)nloc; i += blockDim.x) {
            const double v = fx_row(rows, i, HR, inv, inv_lo, bad);
            rows[i] = (MODE == 3 && G == 1) ? colv_t<CV>(P, i0 + i) * v : v;
        }
    } else if (P.r_fx > 0.0) {
        tile_walk_any<(MODE == 3 ? 0 : MODE), false, true>(T, rb, g, P.r, rows, rc, 1.0,
                                                            1.0 / P.r_fx, clear);
    } else {
        tile_walk_any<(MODE == 3 ? 0 : MODE)>(T, rb, g, P.r, rows, rc, 1.0, 1.0, clear);
    }
    PH(4);
    __syncthreads();
    PH(5);
    // wpart's tail: one slot per (group, row block) for the slices' r^2 sums
    double *rrp = P.wpart + G * T.nrb * (T.H + 1);
    if (FUSE && ITER && G > 1) {
        block_sum<1>(rr, red);
        if (threadIdx.x == 0)
            __hip_atomic_store(&rrp[g * T.nrb + rb], rr[0], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    bool fin = true;
    // dealt image, one group (MODE 3): w_i = colv_i * (sum of r over row i),
    // one product per row (the sums' order is not fixed anyway), formed in the
    // epilogue below; several groups: by the finishing workgroup
    // (FX: the conversion above formed the products already)
    const bool scale_epi = !FX && MODE == 3 && G == 1;
    if (G > 1 && gsel >= 0) {
        // the part pipeline: fixed roles (see above)
        if (gsel < G - 1) {
            double *wp = P.wpart + (g * T.nrb + rb) * (T.H + 1);
            for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x) wp[i] = rows[i];
            return;
        }
        for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x) {
            double o = 0.0;
            for (int64_t c = 0; c < G - 1; ++c)
                o += __hip_atomic_load(&P.wpart[(c * T.nrb + rb) * (T.H + 1) + i], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            o += rows[i];
            rows[i] = (MODE == 3) ? colv_t<CV>(P, i0 + i) * o : o;
        }
        __syncthreads();
    } else if (G > 1) {
        double *wp = P.wpart + (g * T.nrb + rb) * (T.H + 1);
        for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x)
            __hip_atomic_store(&wp[i], rows[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        fin = rowblock_last(tk2rb, rb, G, &row_last);
        if (fin) {
            for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x) {
                double o = 0.0;
                for (int64_t c = 0; c < G; ++c)
                    o += __hip_atomic_load(&P.wpart[(c * T.nrb + rb) * (T.H + 1) + i],
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                rows[i] = (MODE == 3) ? colv_t<CV>(P, i0 + i) * o : o;
            }
            __syncthreads();
        }
    }
    constexpr int NS = FUSE ? 5 : 4;
    double sums[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sums[q] = 0.0;
    if (fin && BSLS_TILE_KO != 4) {   // (KO 4: no epilogue -- timing builds only)
        // K2E rows per thread per batch: every z index, then every operand of
        // the batch in flight at once (two round trips per batch instead of
        // two per row: C5's 19 rows per thread made the epilogue ~90 us)
        const int64_t iend = (nloc < T.H) ? nloc : T.H;
        constexpr int K2E = BSLS_K2E;
        for (int64_t ib = threadIdx.x; ib < iend; ib += K2E * blockDim.x) {
            int32_t jq[K2E];
            double ca[K2E], cb[K2E], gq[K2E], dq[K2E];
#pragma unroll
            for (int q = 0; q < K2E; ++q) {
                const int64_t i = ib + (int64_t)q * blockDim.x;
                // (j < 0: a block's last x entry, also the matrix's last row)
                jq[q] = (i < iend) ? P.xz[i0 + i] : -1;
                ca[q] = cb[q] = 1.0;
                if (scale_epi && i < iend) {
                    ca[q] = colv_t<CV>(P, i0 + i);
                    cb[q] = (i + 1 < nloc) ? colv_t<CV>(P, i0 + i + 1) : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q < K2E; ++q) {
                gq[q] = dq[q] = 0.0;
                if (ITER && jq[q] >= 0) {
                    gq[q] = gp[jq[q]];
                    if (dzv) dq[q] = dzv[jq[q]];
                }
            }
#pragma unroll
            for (int q = 0; q < K2E; ++q) {
                const int64_t i = ib + (int64_t)q * blockDim.x;
                const int32_t j = jq[q];
                if (j < 0) continue;
                const double wa = scale_epi ? ca[q] * rows[i] : rows[i];
                const double wb = scale_epi ? cb[q] * rows[i + 1] : rows[i + 1];
                const double gv = wa - wb;
                gout[j] = gv;
                if (ITER) {
                    const double dg = gv - gq[q];
                    const double dz = dq[q];
                    sums[0] += dg;
                    sums[1] += dz * dg;
                    sums[2] += dg * dg;
                    sums[3] += gv * gv;
                }
            }
        }
    }
    PH(6);
    if (!ITER || !fin) {
        PH_FLUSH(PH_K2);
        return;
    }
    if constexpr (FUSE) {
        if (G == 1) {
            sums[4] = rr[0];
        } else if (threadIdx.x == 0) {
            // (the group partials' hand-off above orders these slots too)
            double o = 0.0;
            for (int64_t c = 0; c < G; ++c)
                o += __hip_atomic_load(&rrp[c * T.nrb + rb], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            sums[4] = o;
        }
    }
    block_sum<NS>(sums, red);
    double tot[NS];
    // one slot per row block, summed in row-block order: with several groups
    // the finishing workgroup of a block varies from run to run, so its
    // blockIdx must not decide where the block's sums enter the reduction
    const bool last = (G == 1) ? last_block_sum<NS>(sums, part, ticket, tot, red)
                               : last_of_sum<NS>(sums, part, (unsigned)rb, (unsigned)T.nrb, ticket,
                                                 tot, red);
    if (last && threadIdx.x == 0) k2_store_sums<FUSE>(P, iter, tot);
    PH(7);
    PH_FLUSH(PH_K2);
}

// Stage 12 (the sliced schedule, after the all-reduce of scal[SUMDG..RR]):
// f(iter - 1) from the summed ||r||^2 and the stopping test of iter - 1 on
// its own g.g and dg.dg (kept by stage 10 in scal[PSUMDG..PGG]); on a stop the
// scal sums go back to that iteration's, as the unfused schedule leaves them.
__global__ void bb_shard_record(bsls_bb_problem P, int64_t iter) {
    if (threadIdx.x != 0) return;
    double *s = P.scal;
    const int64_t it = iter - 1;
    if (it > 0 && s[BSLS_S_STOP] != 0.0) return;
    const double rr = s[BSLS_S_RR];
    const double nr = sqrt(rr);
    const double fx = 0.5 * (nr * nr);      // 0.5 * la.norm(r)**2, main.py:53
    s[BSLS_S_FX] = fx;
    if (it <= 0) return;
    s[BSLS_S_ITER] = (double)it;
    s[BSLS_S_ZBUF] = (double)(it & 1);
    const int reason = bb_stop_reason(P, it, fx, s[BSLS_S_PGG], s[BSLS_S_PDGDG]);
    if (reason) {
        s[BSLS_S_STOP] = (double)reason;
        for (int q = 0; q < 4; ++q) s[BSLS_S_SUMDG + q] = s[BSLS_S_PSUMDG + q];
    }
}

// Multi-GPU stage 2: r (already all-reduced) += target, ||r||^2, stop test.
__global__ __launch_bounds__(256) void bb_r_finish(bsls_bb_problem P, int64_t iter, double *part,
                                                   unsigned *ticket, int add_target) {
    __shared__ double red[4];
    if (iter > 0 && P.scal[BSLS_S_STOP] != 0.0) return;
    // grid-stride over at most R_FINISH_GRID workgroups (the launch below):
    // one workgroup per 256 rows made 3.9k ticket arrivals at m = 1M, ~20 us
    // for 24 MB in the 8-way rehearsal
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    double sq[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < P.m; i += gs) {
        double o = r_load(P, i);
        if (add_target) {
            o += P.target[i];
            P.r[i] = (P.r_fx > 0.0) ? r_fx_of(P, o) : o;
        }
        sq[0] += o * o;
    }
    block_sum<1>(sq, red);
    double tot[1];
    if (last_block_sum<1>(sq, part, ticket, tot, red) && threadIdx.x == 0)
        bb_record_f(P, iter, tot[0], iter > 0);
}
constexpr int R_FINISH_GRID = 512;

// K2: g = N'(A' r); with ITER also dg = g - g_prev and the BB sums.  The
// workgroup's 16 panels (x-rows) are summed over every chunk of r; then lane
// position p of a panel has w_i in acc[p] and w_{i+1} in acc[p + 1] (the halo
// row), so N'w = w_i - w_{i+1} needs no exchange.  The column scales are
// loaded before the chunk loop; the epilogue's z indices and operands after
// it (the walk holds 122 of the 128 VGPRs; loading the indices early measured
// no faster).  The ITER epilogue reads g_prev and dz = z - z_prev (K3 wrote
// dz from the z's it holds, bit-identical to the subtraction here): 15.2 MB
// that no walk overlaps, where z and z_prev were 22.8 MB.
template <int MODE, bool ITER, int FUSE = 0>
__global__ __launch_bounds__(1024) void bb_k2(bsls_bb_problem P, const double *__restrict__ dzv,
                                              const double *__restrict__ gp,
                                              double *__restrict__ gout, double *part,
                                              unsigned *ticket, int64_t iter) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        k2_stopped_sums<FUSE>(P);
        return;
    }
    const bsls_panels &M = P.AT;
    const int wv = threadIdx.x / WAVE, lane = lane_id();
    const int64_t panel = (int64_t)blockIdx.x * PANEL_WAVES + wv;
    const int64_t i0 = panel * M.prow;
    const bool live = panel < M.npanels;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    if (MODE == 2) {
        // unconditional loads at clamped rows (all in flight together)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 64 * q + lane;        // halo row included
            const bool ok = live && 64 * q + lane <= M.prow && i < P.n;
            const double v = colv_at(P, ok ? i : 0);
            sc[q] = ok ? v : 0.0;
        }
    }
    panel_chunks<MODE>(M, blockIdx.x, wv, 0, M.nchunks, P.r, lds, s, sc);
    // w_{i+1}: the next lane, or lane 0 of the next slice (the halo row is
    // row prow of the panel)
    double nx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double dn = __shfl_down(s[q], 1, WAVE);
        const double wrap = (q < 3) ? __shfl(s[q < 3 ? q + 1 : q], 0, WAVE) : 0.0;
        nx[q] = (lane < 63) ? dn : wrap;
    }
    __syncthreads();   // the chunk table becomes the reduction scratch below
    constexpr int NS = FUSE ? 5 : 4;
    double sums[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sums[q] = 0.0;
    // epilogue operands: unconditional loads at clamped indices, all in flight
    int32_t j[4];
    double gpj[4], dzj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int pos = 64 * q + lane;
        const int64_t i = i0 + pos;
        const bool ok = live && pos < M.prow && i < P.n;
        const int32_t jj = P.xz[ok ? i : 0];
        j[q] = ok ? jj : -1;
    }
    if (ITER) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int32_t jc = j[q] >= 0 ? j[q] : 0;
            gpj[q] = gp[jc];
            dzj[q] = dzv ? dzv[jc] : 0.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (j[q] >= 0) {
            const double g = s[q] - nx[q];
            gout[j[q]] = g;
            if (ITER) {
                const double dg = g - gpj[q];
                const double dz = dzj[q];
                sums[0] += dg;
                sums[1] += dz * dg;
                sums[2] += dg * dg;
                sums[3] += g * g;
            }
        }
    }
    if (!ITER) return;
    if constexpr (FUSE) {   // stage 8 / 10: this workgroup's slice of ||r||^2 (see bb_k2t)
        const bool cut = FUSE == 2 && P.rr_hi > P.rr_lo;
        const int64_t lo = cut ? P.rr_lo : 0, span = (cut ? P.rr_hi : P.m) - lo;
        const int64_t q0 = lo + (int64_t)blockIdx.x * span / gridDim.x;
        const int64_t q1 = lo + ((int64_t)blockIdx.x + 1) * span / gridDim.x;
        for (int64_t i = q0 + threadIdx.x; i < q1; i += blockDim.x) {
            const double v = P.r[i];
            sums[4] += v * v;
        }
    }
    block_sum<NS>(sums, lds);
    double tot[NS];
    if (last_block_sum<NS>(sums, part, ticket, tot, lds) && threadIdx.x == 0)
        k2_store_sums<FUSE>(P, iter, tot);
}

// x entry i of N z; for a scaled incidence K1 gathers colv[i] * x_i instead,
// the product SciPy's csr_matvec forms for every entry of column i.
__device__ __forceinline__ void x_put(const bsls_bb_problem &P, int64_t i, double v) {
    P.x[i] = P.colv ? colv_at(P, i) * v : v;
}

__device__ __forceinline__ int64_t zend(const bsls_bb_problem &P, int64_t b) {
    return (b + 1 < P.nblocks) ? P.zstarts[b + 1] : P.nz;
}
__device__ __forceinline__ int64_t xend(const bsls_bb_problem &P, int64_t b) {
    return (b + 1 < P.nblocks) ? P.xstarts[b + 1] : P.n;
}

// K3: t, z_new = clip01(PAVA(z - t g)) per block, x = N z_new.  One wave per
// pack of whole z-blocks (<= 64 entries, one lane each): the PAVA passes run
// wave-parallel (pava_wave.hpp, bit-identical to the serial reference); a
// block longer than 64 entries gets a pack of its own and the serial PAVA.
// sc = scal[STOP], scal[SUMDG], scal[DZDG], scal[DGDG], loaded by the caller
// together with its other first loads (one round trip, not three)
__device__ __forceinline__ bool bb_step_t(const bsls_bb_problem &P, int64_t iter,
                                          const double (&sc)[4], double &t) {
    double *s = P.scal;
    if (sc[0] != 0.0) return false;
    if (P.early_exit && sc[1] == 0.0) {  // BB.py:22
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            s[BSLS_S_STOP] = (double)BSLS_STOP_NOCHANGE;
            s[BSLS_S_ITER] = (double)iter;
            s[BSLS_S_ZBUF] = (double)((iter - 1) & 1);
        }
        return false;
    }
    t = sc[2] / sc[3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        s[BSLS_S_T] = t;
        if (fabs(t) <= 1e-10 || fabs(t) > 1e10) s[BSLS_S_WARN] += 1.0;
    }
    return true;
}

#ifndef BSLS_K3_SGPRS
#define BSLS_K3_SGPRS 80
#endif

// Each wave takes K3_PPW packs (w, w + W, ...; W = waves in the grid) and
// issues every load of all of them -- metadata, then z, g and the column
// scales -- before the first PAVA.  MERGE (K3_PPW = 2): the two packs' PAVA
// share the wave after their first passes (pava_v1_wave_pair).
// (at most 80 SGPRs: 256-thread blocks are admitted 8 per CU only up to 80,
// MI355X_MICROARCH.md "Residency"; the merged form otherwise takes 83 and 7)
template <int K3_PPW, bool MERGE, int CV = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(BSLS_K3_SGPRS)))
void bb_k3(bsls_bb_problem P, int64_t iter,
                                             const double *__restrict__ zc,
                                             const double *__restrict__ g,
                                             double *__restrict__ zn,
                                             double *__restrict__ dzo,
                                             int32_t *__restrict__ wsc, int rec,
                                             uint64_t *__restrict__ hd, int kinit,
                                             unsigned long long *rmax_clear = nullptr) {
    PH_DECL;
    PH(0);
    const double sc[4] = {P.scal[BSLS_S_STOP], P.scal[BSLS_S_SUMDG], P.scal[BSLS_S_DZDG],
                          P.scal[BSLS_S_DGDG]};
    // fx_sums: K2, which read max|r|, has finished and the next K1 finish has
    // not begun: the slots back to 0 for it
    if (rmax_clear && blockIdx.x == 0 && threadIdx.x < RMAX_SLOTS) rmax_clear[threadIdx.x] = 0ull;
    // kinit (stage 15): the next K1's r initialisation folded in (its atomic
    // group sums add into r): r = target on the shard_role 1 rank, 0 on the
    // others; once stopped, role 1 keeps its r and the others write 0 -- as
    // bb_k1_init, one launch fewer
    auto init_r = [&](bool stopped) {
        const int64_t gs = (int64_t)gridDim.x * blockDim.x;
        const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (stopped) {
            k1_stopped_rows(P, 0, P.m, t0, gs);
            return;
        }
        const bool add = P.shard_role == 1;
        for (int64_t row = t0; row < P.m; row += gs) {
            const double v = add ? P.target[row] : 0.0;
            P.r[row] = (P.r_fx > 0.0) ? r_fx_of(P, v) : v;
        }
    };
    // rec (stage 13, the sliced sharded schedule): stage 12 folded in -- f and
    // the stopping test of iter - 1 from the all-reduced scal[RR] and the kept
    // scal[PGG] / scal[PDGDG], decided alike by every workgroup (the same
    // inputs), recorded by workgroup 0; on a stop every workgroup returns
    if (rec && !(iter - 1 > 0 && sc[0] != 0.0)) {
        double *s = P.scal;
        const int64_t it = iter - 1;
        const double nr = sqrt(s[BSLS_S_RR]);
        const double fx = 0.5 * (nr * nr);
        const int reason = it > 0 ? bb_stop_reason(P, it, fx, s[BSLS_S_PGG], s[BSLS_S_PDGDG]) : 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            s[BSLS_S_FX] = fx;
            if (it > 0) {
                s[BSLS_S_ITER] = (double)it;
                s[BSLS_S_ZBUF] = (double)(it & 1);
            }
            if (reason) {
                s[BSLS_S_STOP] = (double)reason;
                for (int q = 0; q < 4; ++q) s[BSLS_S_SUMDG + q] = s[BSLS_S_PSUMDG + q];
            }
        }
        if (reason) {
            if (kinit) init_r(true);
            return;
        }
    }
    const int l = lane_id();
    const int wv = threadIdx.x / WAVE;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int64_t w0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wv);   // wave-uniform
    __shared__ double pv_y[4][64];
    __shared__ int pv_p[4][128];
    __shared__ int pv_c[4][65];
    int64_t z0[K3_PPW], b0[K3_PPW];
    int L[K3_PPW];
    uint64_t B[K3_PPW], H[K3_PPW];
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q) {
        // unconditional loads at a clamped index (straight-line, one round trip)
        const int64_t pk = w0 + q * nw;
        const int64_t pc = pk < P.npacks ? pk : P.npacks - 1;
        z0[q] = P.pk_z0[pc];
        b0[q] = P.pk_b0[pc];
        L[q] = pk < P.npacks ? P.pk_len[pc] : 0;
        B[q] = (uint64_t)P.pk_mask[pc];
        H[q] = hd ? hd[pc] : 0ull;
    }
    double zv[K3_PPW], gv[K3_PPW], cv[K3_PPW], cv2[K3_PPW];
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q) {
        const bool act = l < L[q] && L[q] <= WAVE;
        const bool bend = (l == L[q] - 1) || (l < 63 && ((B[q] >> (l + 1)) & 1ull));
        const int64_t xi = z0[q] + l + b0[q] + __popcll(B[q] & mask_le(l)) - 1;
        cv[q] = cv2[q] = 1.0;
        if (P.colv) {
            // the column scales of this lane's x entries, loaded before the
            // PAVA so their round trip overlaps it (x_put's products)
            cv[q] = act ? colv_t<CV>(P, xi) : 1.0;
            cv2[q] = (act && bend) ? colv_t<CV>(P, xi + 1) : 1.0;
        }
        zv[q] = act ? zc[z0[q] + l] : 0.0;
        gv[q] = act ? g[z0[q] + l] : 0.0;
    }
    double t;
    const bool go = bb_step_t(P, iter, sc, t);
    if (kinit) init_r(!go);
    if (!go) return;
    PH(1);
    double yv[K3_PPW];
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q)   // x_next = x - t g (BB.py:29)
        yv[q] = (l < L[q] && L[q] <= WAVE) ? zv[q] - t * gv[q] : 0.0;
#ifdef BSLS_PHASE_STAMPS
    // (the stamp after z and g have landed: it waits for them through yv)
    asm volatile("" ::"v"(yv[0]));
    PH(2);
#endif
    if (BSLS_K3_KO != 1) {
        // warm start: the last run partition of each pack, tested first; a
        // pack that passes needs no reference pass, and a partition that
        // fails is repaired -- its unsplittable runs kept pooled -- and the
        // reference passes continue from it (pava_warm_repair)
        bool need[K3_PPW], store[K3_PPW];
        uint64_t Hn[K3_PPW];
#pragma unroll
        for (int q = 0; q < K3_PPW; ++q) {
            need[q] = L[q] > 0 && L[q] <= WAVE;
            store[q] = need[q];
            if (hd && need[q] && (H[q] & B[q]) == B[q] && (H[q] & ~mask_lt(L[q])) == 0ull) {
                store[q] = pava_warm_repair(yv[q], L[q], B[q], H[q], pv_y[wv], pv_p[wv],
                                            pv_c[wv], &Hn[q]);
                need[q] = false;
            }
        }
        if (MERGE && K3_PPW == 2 && need[0] && need[K3_PPW - 1]) {
            pava_v1_wave_pair(yv[0], L[0], B[0], yv[K3_PPW - 1], L[K3_PPW - 1], B[K3_PPW - 1],
                              pv_y[wv], pv_p[wv], pv_c[wv], &Hn[0], &Hn[K3_PPW - 1]);
        } else {
#pragma unroll
            for (int q = 0; q < K3_PPW; ++q)
                if (need[q])
                    pava_v1_wave_c(yv[q], L[q], B[q], pv_y[wv], pv_p[wv], pv_c[wv], &Hn[q]);
        }
        if (hd) {
#pragma unroll
            for (int q = 0; q < K3_PPW; ++q)   // the new partition for the next call
                if (store[q] && l == 0) hd[w0 + q * nw] = Hn[q];
        }
    }
    PH(3);
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q) {
        if (L[q] == 0) break;
        if (L[q] <= WAVE) {
            const bool act = l < L[q];
            const bool bstart = (B[q] >> l) & 1ull;
            const int bl = __popcll(B[q] & mask_le(l)) - 1;   // block within the pack
            const bool bend = (l == L[q] - 1) || (l < 63 && ((B[q] >> (l + 1)) & 1ull));
            const double v = clip01(yv[q]);
            const double vprev = shfl_d(v, l > 0 ? l - 1 : 0);
            const int nb = __popcll(B[q]);
            const __amdgpu_buffer_rsrc_t rz =
                __builtin_amdgcn_make_buffer_rsrc(zn + z0[q], 0, L[q] * 8, 0x00020000);
            const __amdgpu_buffer_rsrc_t rd =
                __builtin_amdgcn_make_buffer_rsrc(dzo + z0[q], 0, L[q] * 8, 0x00020000);
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
                P.x + z0[q] + b0[q], 0, (L[q] + nb) * 8, 0x00020000);
            if (act) {
                wt_store_f64(rz, l * 8, v);
                wt_store_f64(rd, l * 8, v - zv[q]);   // next K2's z - z_prev
                const double d = v - (bstart ? 0.0 : vprev);
                const int xo = (l + bl) * 8;
                wt_store_f64(rx, xo, P.colv ? cv[q] * d : d);
                if (bend) wt_store_f64(rx, xo + 8, P.colv ? cv2[q] * (0.0 - v) : (0.0 - v));
            }
        } else if (!P.long_packs && l == 0) {
            // one block longer than a wave: serial PAVA in global memory
            // (with P.long_packs bb_k3_long takes it, a workgroup per block)
            const int64_t xs = P.xstarts[b0[q]];
            for (int64_t j = z0[q]; j < z0[q] + L[q]; ++j) {
                zn[j] = zc[j] - t * g[j];
                wsc[j] = 1;
            }
            pava_v1(zn, wsc, z0[q], z0[q] + L[q], 1);
            double prev = 0.0;
            int64_t xo = xs;
            for (int64_t j = z0[q]; j < z0[q] + L[q]; ++j) {
                const double v = clip01(zn[j]);
                zn[j] = v;
                dzo[j] = v - zc[j];
                x_put(P, xo++, v - prev);
                prev = v;
            }
            x_put(P, xo, 0.0 - prev);
        }
    }
    PH(4);
    PH_FLUSH(PH_K3);
}

// K3 for one z-block longer than a wave, one 1024-thread workgroup per block
// (after bb_k3 in the same stream): z - t g, PAVA v1 by the whole workgroup
// (pava_long.hpp, bit-identical), clip, dz and x as bb_k3's serial path.
// t as bb_step_t, without its writes (bb_k3 made them).
__global__ __launch_bounds__(LONG_T) void bb_k3_long(bsls_bb_problem P, int64_t iter,
                                                     const double *__restrict__ zc,
                                                     const double *__restrict__ g,
                                                     double *__restrict__ zn,
                                                     double *__restrict__ dzo) {
    __shared__ int64_t sh[LONG_T / 64 + 1];
    __shared__ int flag;
    const double *s = P.scal;
    if (s[BSLS_S_STOP] != 0.0) return;
    if (P.early_exit && s[BSLS_S_SUMDG] == 0.0) return;
    const double t = s[BSLS_S_DZDG] / s[BSLS_S_DGDG];
    const int64_t q = P.long_packs[blockIdx.x];
    const int64_t z0 = P.pk_z0[q], b0 = P.pk_b0[q], L = P.pk_len[q];
    const int64_t off = P.long_off[blockIdx.x], tot = P.long_off[P.nlong];
    double *Y0 = (double *)P.long_scratch + off;
    double *Y1 = (double *)P.long_scratch + tot + off;
    int32_t *W = (int32_t *)((double *)P.long_scratch + 2 * tot);
    int32_t *W0 = W + off, *W1 = W + tot + off, *CH = W + 2 * tot + blockIdx.x + off;
    for (int64_t j = threadIdx.x; j < L; j += LONG_T) zn[z0 + j] = zc[z0 + j] - t * g[z0 + j];
    __syncthreads();
    pava_v1_long(zn + z0, L, Y0, Y1, W0, W1, CH, sh, &flag);
    for (int64_t j = threadIdx.x; j < L; j += LONG_T) {
        const double v = clip01(zn[z0 + j]);
        zn[z0 + j] = v;
        dzo[z0 + j] = v - zc[z0 + j];
    }
    __syncthreads();
    const int64_t xs = P.xstarts[b0];
    for (int64_t j = threadIdx.x; j <= L; j += LONG_T) {
        const double v = (j < L) ? zn[z0 + j] : 0.0;
        const double prev = (j > 0) ? zn[z0 + j - 1] : 0.0;
        x_put(P, xs + j, v - prev);
    }
}

// Prologue helpers (BB.py:14-15: x_prev = x + 1); bb_z2x writes N z.
__global__ __launch_bounds__(256) void bb_plus_one(const double *__restrict__ a,
                                                   double *__restrict__ o,
                                                   double *__restrict__ dz, int64_t nz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nz) {
        const double v = a[i], w = v + 1;
        o[i] = w;
        dz[i] = v - w;   // iteration 1's z - z_prev
    }
}

// one thread per x entry (coalesced; C5 418 -> ~20 us against a thread per
// block): xz[i] is entry i's z index, -1 for a block's last entry (blocks
// have >= 2 routes); the same differences K3 forms (v - prev, prev = 0.0 at a
// block's first entry, 0.0 - z_last at its last)
__global__ __launch_bounds__(256) void bb_z2x(bsls_bb_problem P, const double *__restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const int32_t j = P.xz[i];
    const int32_t jp = (i > 0) ? P.xz[i - 1] : -1;
    double v;
    if (j >= 0) v = z[j] - (jp >= 0 ? z[jp] : 0.0);
    else v = 0.0 - z[jp];
    x_put(P, i, v);
}

// Up to ~160 KB of dynamic LDS (panel_lds_bytes): opt in once per kernel instance.
constexpr int PANEL_LDS_MAX = 163840 - 512;
template <typename K>
static void allow_lds(K kernel) {
    static bool done = false;
    if (!done) {
        // A refusal must not stay behind as the thread's last error: the launch
        // check after the kernel would report it as the launch's.  (PANEL_LDS_MAX
        // on top of a kernel's static LDS can pass the CU's 160 KB -- bb_k2t's
        // iterating forms hold 656 B -- and `done` is per kernel signature, so
        // it is a process's first K2 on tiles that asks: stage 3 of an iteration
        // with no prologue before it returned hipErrorInvalidValue.)
        if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                PANEL_LDS_MAX) != hipSuccess)
            (void)hipGetLastError();
        done = true;
    }
}

// K1's row blocks: panels 16 panels each, tiles H rows each
static int64_t k1_row_blocks(const bsls_bb_problem &P) {
    return P.At.ent ? P.At.nrb : (P.A.npanels + PANEL_WAVES - 1) / PANEL_WAVES;
}

// row blocks [rb0, rb1) of K1 (the whole matrix unless a multi-GPU driver
// all-reduces r part by part behind it); REDUCE needs the whole matrix
template <int MODE, bool ADD, bool REDUCE, bool ITER>
static void launch_k1_mode(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                           hipStream_t st, int64_t rb0, int64_t rb1) {
    if constexpr (ADD && (REDUCE || !ITER)) {
        // roww: the weighted finish (the same launches as fx_sums covers on the tiles)
        if (P.roww) {
            allow_lds(bb_k1<MODE, ITER, true, REDUCE, true>);
            bb_k1<MODE, ITER, true, REDUCE, true><<<(int)(P.A.ngroups * (rb1 - rb0)), 1024,
                                                    panel_lds_bytes(P.A), st>>>(P, iter, w.tkrb,
                                                                                w.p1, w.tk1, rb0);
            return;
        }
    }
    allow_lds(bb_k1<MODE, ITER, ADD, REDUCE>);
    bb_k1<MODE, ITER, ADD, REDUCE><<<(int)(P.A.ngroups * (rb1 - rb0)), 1024, panel_lds_bytes(P.A),
                                     st>>>(P, iter, w.tkrb, w.p1, w.tk1, rb0);
}

// Several-group K1 without the partials: r initialised (bb_k1_init), every
// group's sums added by global f64 atomics, ||r||^2 and the stop test
// (REDUCE) by bb_r_finish.  The default on a column shard's partial residual
// (stage 1): the rehearsed 8-way C5 rank-0 iteration 162.6 -> 148.4 us -- no
// bb_k1_sum, and no 4 x 8 MB of partials through the Infinity Cache ahead of
// K2.  On one GPU it measured no faster (C3 83.0 / 85.7 us, C5 800 / 801: the
// ||r||^2 pass reads r again), and the atomics' varying order moves the exact
// zero sum(dg) exit of BB.py:22 (a tests/fast problem stopped at 967 instead
// of ~770), so one GPU keeps the group sums.  bsls_bb_problem.k1_atomic
// (the engine's BSLS_K1_ATOMIC, read once): 1 = never, 2 = wherever K1 has
// several groups, 0 = the default above.
static bool k1_atomic(const bsls_bb_problem &P, bool reduce) {
    if (P.k1_atomic) return P.k1_atomic == 2;
    return P.shard_role != 0 && !reduce;
}

// stage 15 / 14: the atomic K1's r initialisation done by the K3 before it
// (bb_k3 kinit) -- whole matrix only
static bool k1_init_folded(const bsls_bb_problem &P) {
    return P.At.ent && P.At.ngroups > 1 && k1_atomic(P, false);
}

// bb_k1_sum behind a several-group bb_k1t over row blocks [rb0, rb1): rows in
// 16-B pairs (W = 2) where every pair is aligned in rpart, target, r and (RW)
// roww
template <bool ITER, bool ADD, bool REDUCE, bool FX, bool RW = false>
static void launch_k1_sum(const bsls_bb_problem &P, int64_t iter, const BBWork &w, hipStream_t st,
                          int64_t rb0, int64_t rb1) {
    const int64_t r0 = rb0 * P.At.H, r1 = (rb1 * P.At.H < P.m) ? rb1 * P.At.H : P.m;
    constexpr int K1_SUM_GRID = 1024;
    const bool pairs = !(P.m & 1) && !(r0 & 1) && r1 - r0 >= 2 &&
                       !(((uintptr_t)P.rpart | (uintptr_t)P.target | (uintptr_t)P.r |
                          (RW ? (uintptr_t)P.roww : (uintptr_t)0)) & 15);
    const int gk = grid_for(pairs ? (r1 - r0) / 2 : r1 - r0, 256);
    const int grid = (REDUCE && gk > K1_SUM_GRID) ? K1_SUM_GRID : gk;
    unsigned long long *rmax = FX ? w.rmax : nullptr;
    if (pairs)
        bb_k1_sum<ITER, ADD, REDUCE, 2, FX, RW><<<grid, 256, 0, st>>>(P, iter, P.At.ngroups, r0,
                                                                      r1, w.pf, w.tkf, rmax);
    else
        bb_k1_sum<ITER, ADD, REDUCE, 1, FX, RW><<<grid, 256, 0, st>>>(P, iter, P.At.ngroups, r0,
                                                                      r1, w.pf, w.tkf, rmax);
}

// K1 with fixed-point row sums (bsls_bb_problem.fx_sums): bb_k1t's FX form and,
// with several groups, bb_k1_sum's -- the launches of the float form
template <int MODE, bool REDUCE, bool ITER>
static void launch_k1t_fx(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                          hipStream_t st, int64_t rb0, int64_t rb1) {
    allow_lds(bb_k1t<MODE, ITER, true, REDUCE, false, true>);
    bb_k1t<MODE, ITER, true, REDUCE, false, true><<<(int)((rb1 - rb0) * P.At.ngroups),
                                                    BSLS_TILE_THREADS,
                                                    tile_lds_doubles(P.At, true) * 8, st>>>(
        P, iter, w.p1, w.tk1, rb0, w.rmax);
    if (P.At.ngroups > 1) launch_k1_sum<ITER, true, REDUCE, true>(P, iter, w, st, rb0, rb1);
}

template <int MODE, bool ADD, bool REDUCE, bool ITER>
static void launch_k1t_mode(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                            hipStream_t st, int64_t rb0, int64_t rb1, bool skip_init) {
    if (P.At.ngroups > 1 && k1_atomic(P, REDUCE)) {
        const int64_t r0 = rb0 * P.At.H, r1 = (rb1 * P.At.H < P.m) ? rb1 * P.At.H : P.m;
        const int gi = grid_for(r1 - r0, 256);
        // one row per thread (the grid-stride form at 1024 workgroups gave each
        // thread 4 rows at m = 1M; the rehearsed iteration measured the same
        // either way, 149.3-149.8 us)
        if (!skip_init)
            bb_k1_init<ITER, ADD><<<gi < 16384 ? gi : 16384, 256, 0, st>>>(P, r0, r1);
        allow_lds(bb_k1t<MODE, ITER, ADD, false, true>);
        bb_k1t<MODE, ITER, ADD, false, true><<<(int)((rb1 - rb0) * P.At.ngroups),
                                               BSLS_TILE_THREADS, tile_lds_doubles(P.At, false) * 8,
                                               st>>>(P, iter, w.p1, w.tk1, rb0);
        if (REDUCE)
            bb_r_finish<<<(grid_for(P.m, 256) < R_FINISH_GRID ? grid_for(P.m, 256) : R_FINISH_GRID),
                          256, 0, st>>>(P, iter, w.pf, w.tkf, 0);
        return;
    }
    if constexpr (ADD && (REDUCE || !ITER)) {
        // fx_sums (check_problem: dealt images, never the atomic K1; the entry
        // points that take the other forms -- no target, or an iteration's K1
        // without the reduction -- reject such a problem): the fixed-point
        // walk, and the finish that keeps max|r|
        if (P.fx_sums) {
            launch_k1t_fx<MODE, REDUCE, ITER>(P, iter, w, st, rb0, rb1);
            return;
        }
        // roww (check_problem: never with fx_sums or the atomic K1): one group
        // finishes weighted in the walk's kernel; several leave the float
        // form's partials, and bb_k1_sum weighs
        if (P.roww) {
            const int grid = (int)((rb1 - rb0) * P.At.ngroups);
            const size_t lds = tile_lds_doubles(P.At, false) * 8;
            if (P.At.ngroups > 1) {
                allow_lds(bb_k1t<MODE, ITER, true, REDUCE>);
                bb_k1t<MODE, ITER, true, REDUCE><<<grid, BSLS_TILE_THREADS, lds, st>>>(
                    P, iter, w.p1, w.tk1, rb0);
                launch_k1_sum<ITER, true, REDUCE, false, true>(P, iter, w, st, rb0, rb1);
            } else {
                allow_lds(bb_k1t<MODE, ITER, true, REDUCE, false, false, true>);
                bb_k1t<MODE, ITER, true, REDUCE, false, false, true>
                    <<<grid, BSLS_TILE_THREADS, lds, st>>>(P, iter, w.p1, w.tk1, rb0);
            }
            return;
        }
    }
    allow_lds(bb_k1t<MODE, ITER, ADD, REDUCE>);
    bb_k1t<MODE, ITER, ADD, REDUCE><<<(int)((rb1 - rb0) * P.At.ngroups), BSLS_TILE_THREADS,
                                      tile_lds_doubles(P.At, false) * 8, st>>>(P, iter, w.p1,
                                                                                w.tk1, rb0);
    if (P.At.ngroups > 1) launch_k1_sum<ITER, ADD, REDUCE, false>(P, iter, w, st, rb0, rb1);
}

template <bool ADD, bool REDUCE, bool ITER>
static void launch_k1(const bsls_bb_problem &P, int64_t iter, const BBWork &w, hipStream_t st,
                      int64_t rb0 = 0, int64_t rb1 = -1, bool skip_init = false) {
    if (rb1 < 0) rb1 = k1_row_blocks(P);
    if (P.At.ent) {
        if (P.colv) launch_k1t_mode<0, ADD, REDUCE, ITER>(P, iter, w, st, rb0, rb1, skip_init);
        else launch_k1t_mode<1, ADD, REDUCE, ITER>(P, iter, w, st, rb0, rb1, skip_init);
    } else if (P.colv) {
        launch_k1_mode<0, ADD, REDUCE, ITER>(P, iter, w, st, rb0, rb1);
    } else {
        launch_k1_mode<1, ADD, REDUCE, ITER>(P, iter, w, st, rb0, rb1);
    }
}

// A column shard's partial residual (stages 1 / 14, bsls_bb_residual_rows,
// bsls_bb_k1_rows): the shard_role 1 rank adds target, the stop test runs
// inside an iteration only, and ||r||^2 waits for the all-reduce of r
static void launch_k1_partial(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                              hipStream_t st, int64_t rb0 = 0, int64_t rb1 = -1,
                              bool skip_init = false) {
    const bool add = P.shard_role == 1;
    if (add && iter > 0) launch_k1<true, false, true>(P, iter, w, st, rb0, rb1, skip_init);
    else if (add) launch_k1<true, false, false>(P, iter, w, st, rb0, rb1, skip_init);
    else if (iter > 0) launch_k1<false, false, true>(P, iter, w, st, rb0, rb1, skip_init);
    else launch_k1<false, false, false>(P, iter, w, st, rb0, rb1, skip_init);
}

// fx_sums: max|r| back to 0 ahead of a K1 finish that no K3 has cleared it for
static hipError_t clear_rmax(const bsls_bb_problem &P, const BBWork &w, hipStream_t st) {
    return P.fx_sums ? hipMemsetAsync(w.rmax, 0, RMAX_SLOTS * 8, st) : hipSuccess;
}

// (dz: the vector the ITER sums dot with delta_g -- the workspace's z - z_prev
// unless given: the line search passes its direction d, with g_prev = 0)
template <int MODE, bool ITER, int FUSE>
static void launch_k2_mode(const bsls_bb_problem &P, const double *gp, double *gout,
                           const BBWork &w, hipStream_t st, int64_t iter, const double *dz) {
    allow_lds(bb_k2<MODE, ITER, FUSE>);
    bb_k2<MODE, ITER, FUSE><<<grid_for(P.AT.npanels, PANEL_WAVES), 1024, panel_lds_bytes(P.AT),
                              st>>>(P, dz, gp, gout, w.p2, w.tk2, iter);
}

template <int MODE, bool ITER, int FUSE, int CV>
static void launch_k2t_cv(const bsls_bb_problem &P, const double *gp, double *gout,
                          const BBWork &w, hipStream_t st, int64_t iter, const double *dz,
                          int gsel) {
    if constexpr (FUSE == 0 && (MODE == 1 || MODE == 3)) {
        // fx_sums (check_problem: a dealt image; bsls_bb_k2_part rejects it)
        if (P.fx_sums && gsel < 0) {
            allow_lds(bb_k2t<MODE, ITER, 0, CV, true>);
            bb_k2t<MODE, ITER, 0, CV, true><<<(int)(P.ATt.nrb * P.ATt.ngroups), BSLS_TILE_THREADS,
                                              tile_lds_doubles(P.ATt, true) * 8, st>>>(
                P, dz, gp, gout, w.p2, w.tk2, w.tk2rb, iter, gsel, w.rmax);
            return;
        }
    }
    allow_lds(bb_k2t<MODE, ITER, FUSE, CV>);
    bb_k2t<MODE, ITER, FUSE, CV><<<(int)(gsel >= 0 ? P.ATt.nrb : P.ATt.nrb * P.ATt.ngroups),
                                   BSLS_TILE_THREADS, tile_lds_doubles(P.ATt, MODE == 2) * 8, st>>>(
        P, dz, gp, gout, w.p2, w.tk2, w.tk2rb, iter, gsel);
}

template <int MODE, bool ITER, int FUSE>
static void launch_k2t_mode(const bsls_bb_problem &P, const double *gp, double *gout,
                            const BBWork &w, hipStream_t st, int64_t iter, const double *dz,
                            int gsel) {
    if (MODE != 1 && P.colv_codec == 2)
        launch_k2t_cv<MODE, ITER, FUSE, 2>(P, gp, gout, w, st, iter, dz, gsel);
    else if (MODE != 1 && P.colv_codec == 1)
        launch_k2t_cv<MODE, ITER, FUSE, 1>(P, gp, gout, w, st, iter, dz, gsel);
    else launch_k2t_cv<MODE, ITER, FUSE, 0>(P, gp, gout, w, st, iter, dz, gsel);
}

template <bool ITER, int FUSE = 0>
static void launch_k2(const bsls_bb_problem &P, const double *gp, double *gout,
                      const BBWork &w, hipStream_t st, int64_t iter = 0,
                      const double *dz = nullptr, int gsel = -1) {
    if (!dz) dz = w.dz;
    if (P.ATt.ent) {
        if (!P.colv) launch_k2t_mode<1, ITER, FUSE>(P, gp, gout, w, st, iter, dz, gsel);
        else if (P.ATt.ngroups == 1 && P.ATt.layout == 0)
            launch_k2t_mode<2, ITER, FUSE>(P, gp, gout, w, st, iter, dz, gsel);
        else launch_k2t_mode<3, ITER, FUSE>(P, gp, gout, w, st, iter, dz, gsel);
    } else if (P.colv) {
        launch_k2_mode<2, ITER, FUSE>(P, gp, gout, w, st, iter, dz);
    } else {
        launch_k2_mode<1, ITER, FUSE>(P, gp, gout, w, st, iter, dz);
    }
}

// Two packs per wave sharing their passes after the first
// (pava_v1_wave_pair) pay where the grid runs many rounds of resident waves:
// C5 (172k packs) K3 153 -> 141 us; C3 (16.7k packs, two rounds of 8 waves
// per SIMD) 18.8 -> 20.6 us, the longer wave outlasting its rounds.  So from
// 64k packs (8 rounds); bsls_bb_problem.k3_merge (the engine's
// BSLS_K3_MERGE, read once) forces one (1) or two (2).
static bool k3_merge(const bsls_bb_problem &P) {
    return P.k3_merge ? P.k3_merge == 2 : P.npacks >= 65536;
}

template <int CV>
static void launch_k3_cv(const bsls_bb_problem &P, int64_t iter, const double *zc,
                         const double *g, double *zn, const BBWork &w, hipStream_t st, int rec,
                         int slot, int kinit) {
    // (bsls_bb_problem.pava_warm; a second set of masks for a second
    // projection whose inputs alternate with the first's)
    uint64_t *hd = P.pava_warm ? w.hd + (slot ? w.hd_stride : 0) : nullptr;
    unsigned long long *rmc = P.fx_sums ? w.rmax : nullptr;
    if (k3_merge(P))
        bb_k3<2, true, CV><<<grid_for(P.npacks, 8), 256, 0, st>>>(P, iter, zc, g, zn, w.dz, w.wsc,
                                                                   rec, hd, kinit, rmc);
    else
        bb_k3<1, false, CV><<<grid_for(P.npacks, 4), 256, 0, st>>>(P, iter, zc, g, zn, w.dz,
                                                                    w.wsc, rec, hd, kinit, rmc);
}

static void launch_k3(const bsls_bb_problem &P, int64_t iter, const double *zc, const double *g,
                      double *zn, const BBWork &w, hipStream_t st, int rec = 0, int slot = 0,
                      int kinit = 0) {
    if (P.colv && P.colv_codec == 2) launch_k3_cv<2>(P, iter, zc, g, zn, w, st, rec, slot, kinit);
    else if (P.colv && P.colv_codec == 1)
        launch_k3_cv<1>(P, iter, zc, g, zn, w, st, rec, slot, kinit);
    else launch_k3_cv<0>(P, iter, zc, g, zn, w, st, rec, slot, kinit);
    if (P.long_packs && P.nlong > 0)
        bb_k3_long<<<(int)P.nlong, LONG_T, 0, st>>>(P, iter, zc, g, zn, w.dz);
}

static bool panels_ok(const bsls_panels &M, int64_t rows, int64_t cols, int64_t halo,
                      bool need_val) {
    if (M.rows != rows || M.cols != cols || M.halo != halo) return false;
    if (M.prow < 1 || M.prow + halo > 256 || M.npanels != (rows + M.prow - 1) / M.prow)
        return false;
    if (M.nchunks < 1 || M.ngroups < 1 || M.ngroups > M.nchunks) return false;
    if (M.tab_cap < 64 || M.tab_cap > BSLS_PANEL_CHUNK || panel_lds_bytes(M) > (size_t)PANEL_LDS_MAX)
        return false;
    if (!M.chunk_col || !M.group_chunk || !M.ent_off || !M.cnt_off || !M.seg_info || !M.cnt ||
        !M.ent)
        return false;
    return need_val ? M.val != nullptr : true;
}

static int check_problem(const bsls_bb_problem *p) {
    if (!p || p->m <= 0 || p->n <= 0 || p->nblocks <= 0 || p->nz != p->n - p->nblocks) return BSLS_E_ARG;
    if (p->shard_role < 0 || p->shard_role > 2) return BSLS_E_ARG;
    if (p->k1_atomic < 0 || p->k1_atomic > 2 || p->k3_merge < 0 || p->k3_merge > 2)
        return BSLS_E_ARG;
    // the fixed-point r: every writer of r is the atomic K1 (+ its init) and
    // every K2 reader the dealt walk
    if (!(p->r_fx >= 0.0) || p->r_fx > 1e300) return BSLS_E_ARG;
    if (p->r_fx > 0.0 && !(k1_init_folded(*p) && p->ATt.ent && (p->ATt.layout & 3) != 0))
        return BSLS_E_ARG;
    if (p->colv_codec < 0 || p->colv_codec > 2 || (p->colv_codec && (!p->colv_n || !p->colv)))
        return BSLS_E_ARG;
    // (sy_dr, dz . dg as ||r - r_prev||^2, retired in round 6: it moved where
    // the reference's exact-zero sum(delta_g) exit fires, BB.py:22)
    if (p->sy_dr != 0) return BSLS_E_ARG;
    const bool general = p->colv == nullptr;
    if (p->fx_sums) {
        // fixed-point row sums: dealt images of both matrices with room for two
        // words per row, the whole problem on this GCD, ordered group sums, and
        // bounds a scale can be made from
        const auto bound = [](double v) { return v > 0.0 && v <= 1e300; };
        if (p->fx_sums != 1 || p->shard_role != 0 || p->r_fx != 0.0 || p->k1_atomic == 2)
            return BSLS_E_ARG;
        if (!p->At.ent || (p->At.layout & 3) == 0 || !p->ATt.ent || (p->ATt.layout & 3) == 0)
            return BSLS_E_ARG;
        if (!tiles_valid(p->At, p->m, p->n, 0, general, true, PANEL_LDS_MAX) ||
            !tiles_valid(p->ATt, p->n, p->m, 1, general, true, PANEL_LDS_MAX))
            return BSLS_E_ARG;
        if (!bound(p->fx_a1) || !bound(p->fx_a2) || !bound(p->x_bound)) return BSLS_E_ARG;
    }
    // row weights: the whole problem on this GCD, float row sums, ordered group sums
    if (p->roww && (p->shard_role != 0 || p->r_fx != 0.0 || p->fx_sums != 0 || p->k1_atomic == 2))
        return BSLS_E_ARG;
    if (p->At.ent) {
        if (!tiles_valid(p->At, p->m, p->n, 0, general, false, PANEL_LDS_MAX)) return BSLS_E_ARG;
        if (p->At.ngroups > 1 && !p->rpart) return BSLS_E_ARG;
    } else if (!panels_ok(p->A, p->m, p->n, 0, general) || !p->rpart) {
        return BSLS_E_ARG;
    }
    if (p->ATt.ent) {
        if (!tiles_valid(p->ATt, p->n, p->m, 1, general,
                         !general && p->ATt.ngroups == 1 && p->ATt.layout == 0, PANEL_LDS_MAX))
            return BSLS_E_ARG;
        if (p->ATt.ngroups > 1 && !p->wpart) return BSLS_E_ARG;
    } else if (!panels_ok(p->AT, p->n, p->m, 1, general) || p->AT.ngroups != 1) {
        return BSLS_E_ARG;
    }
    if (p->work_bytes < bb_layout(nullptr, p->m, p->n, p->nz).bytes) return BSLS_E_WORKSPACE;
    if (!p->target || !p->xstarts || !p->zstarts || !p->xz) return BSLS_E_ARG;
    if (!p->pk_z0 || !p->pk_b0 || !p->pk_mask || !p->pk_len || p->npacks < 1) return BSLS_E_ARG;
    if (!p->z[0] || !p->z[1] || !p->g[0] || !p->g[1] || !p->x || !p->r || !p->scal || !p->work)
        return BSLS_E_ARG;
    if (p->long_packs && (p->nlong < 0 || (p->nlong > 0 && (!p->long_off || !p->long_scratch))))
        return BSLS_E_ARG;
    return BSLS_OK;
}

// the entry points that fx_sums and roww do not cover (include/bsls_hip.h)
static int check_problem_float(const bsls_bb_problem *p) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    return (p->fx_sums || p->roww) ? BSLS_E_ARG : BSLS_OK;
}

}  // namespace bsls

using namespace bsls;

// the engine's tenants, on the launchers above: LBFGS.solve's line search and DORE
#include "bb_ls.hpp"
#include "bb_dore.hpp"

#ifdef BSLS_PHASE_STAMPS
// the stamps of the last launches: [kernel][workgroup][slot] -> host (after a sync)
extern "C" int bsls_phase_read(unsigned long long *host, size_t count) {
    const size_t all = sizeof(bsls_phase_buf) / sizeof(unsigned long long);
    BSLS_CHECK(hipMemcpyFromSymbol(host, HIP_SYMBOL(bsls_phase_buf),
                                   (count < all ? count : all) * sizeof(unsigned long long)));
    return BSLS_OK;
}
extern "C" void bsls_phase_shape(int *shape) {
    shape[0] = 4;
    shape[1] = PH_WGS;
    shape[2] = PH_SLOTS;
}
#endif

extern "C" size_t bsls_ticket_bytes(void) { return (size_t)TICKET_BYTES; }

extern "C" size_t bsls_bb_workspace_size(int64_t m, int64_t n, int64_t nz) {
    return bb_layout(nullptr, m, n, nz).bytes;
}

extern "C" size_t bsls_bb_long_scratch_size(int64_t total) {
    // Y0, Y1 (doubles), W0, W1, CH (int32; CH one more per block, <= total)
    return (size_t)(total > 0 ? total : 0) * 32 + 64;
}

extern "C" size_t bsls_bb_dz_offset(int64_t m, int64_t n, int64_t nz) {
    return (size_t)((char *)bb_layout(nullptr, m, n, nz).dz - (char *)nullptr);
}

extern "C" size_t bsls_bb_rmax_offset(int64_t m, int64_t n, int64_t nz) {
    return (size_t)((char *)bb_layout(nullptr, m, n, nz).rmax - (char *)nullptr);
}

extern "C" int bsls_bb_rmax_slots(void) { return RMAX_SLOTS; }

extern "C" int bsls_bb_stage(const bsls_bb_problem *p, int stage, int64_t iter, void *stream) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    const bsls_bb_problem &P = *p;
    hipStream_t st = (hipStream_t)stream;
    const BBWork w = bb_layout(P);
    const int zc = (int)((iter - 1) & 1), zn = (int)(iter & 1);
    // fx_sums: the single-GCD stages only (0, 3-7, 9)
    if (P.fx_sums && (stage == 1 || stage == 2 || stage == 8 || (stage >= 10 && stage <= 15)))
        return BSLS_E_ARG;
    // roww: 0, 1 and 3-7 (stage 1, without target, stays the unweighted A x)
    if (P.roww && (stage == 2 || (stage >= 8 && stage <= 15))) return BSLS_E_ARG;
    switch (stage) {
        case 0:  // reset scalars and tickets
            BSLS_CHECK(hipMemsetAsync(P.scal, 0, BSLS_S_COUNT * sizeof(double), st));
            BSLS_CHECK(hipMemsetAsync(P.work, 0, (size_t)((char *)w.p1 - (char *)P.work), st));
            BSLS_CHECK(clear_rmax(P, w, st));
            return BSLS_OK;
        case 1:  // r_partial = A_g x_g (+ target on the shard_role 1 rank)
            launch_k1_partial(P, iter, w, st);
            break;
        case 2:  // r += target, ||r||^2, stop test
        case 9:  // ||r||^2, stop test (r already the residual)
            bb_r_finish<<<(grid_for(P.m, 256) < R_FINISH_GRID ? grid_for(P.m, 256) : R_FINISH_GRID),
                          256, 0, st>>>(P, iter, w.pf, w.tkf, stage == 2 ? 1 : 0);
            break;
        case 8:  // stage 3 with stage 9 of iteration iter - 1 folded in
            if (iter <= 0) return BSLS_E_ARG;
            launch_k2<true, 1>(P, P.g[zc], P.g[zn], w, st, iter);
            break;
        case 10:  // stage 3 with this rank's slice of ||r||^2 (sliced schedule)
            if (iter <= 0) return BSLS_E_ARG;
            if (P.rr_lo < 0 || P.rr_hi > P.m || P.rr_lo > P.rr_hi) return BSLS_E_ARG;
            launch_k2<true, 2>(P, P.g[zc], P.g[zn], w, st, iter);
            break;
        case 13:  // stage 12 folded into stage 4's K3 (one launch fewer)
            if (iter <= 0) return BSLS_E_ARG;
            launch_k3(P, iter, P.z[zc], P.g[zn], P.z[zn], w, st, 1);
            break;
        case 15:  // stage 13 with the next stage 14's r initialisation folded in
            if (iter <= 0) return BSLS_E_ARG;
            launch_k3(P, iter, P.z[zc], P.g[zn], P.z[zn], w, st, 1, 0,
                      k1_init_folded(P) ? 1 : 0);
            break;
        case 14:  // stage 1 after stage 15 (r already initialised when it folds)
            if (iter <= 0) return BSLS_E_ARG;
            launch_k1_partial(P, iter, w, st, 0, -1, k1_init_folded(P));
            break;
        case 12:  // f / stopping test of iteration iter - 1 (after the sums' all-reduce)
            if (iter <= 0) return BSLS_E_ARG;
            bb_shard_record<<<1, 64, 0, st>>>(P, iter);
            break;
        case 3:  // g = N'A'r (+ sums)
            if (iter > 0) launch_k2<true>(P, P.g[zc], P.g[zn], w, st);
            else launch_k2<false>(P, nullptr, P.g[0], w, st);
            break;
        case 4:  // t, projection, x
            if (iter <= 0) return BSLS_E_ARG;
            launch_k3(P, iter, P.z[zc], P.g[zn], P.z[zn], w, st);
            break;
        case 5:  // z[1] = z[0] + 1; x = N z[1]
            bb_plus_one<<<grid_for(P.nz > 0 ? P.nz : 1, 256), 256, 0, st>>>(P.z[0], P.z[1], w.dz, P.nz);
            BSLS_LAUNCH_CHECK();
            bb_z2x<<<grid_for(P.n, 256), 256, 0, st>>>(P, P.z[1]);
            break;
        case 6:  // x = N z[0]
            bb_z2x<<<grid_for(P.n, 256), 256, 0, st>>>(P, P.z[0]);
            break;
        case 7:  // single GCD K1: r = A x + target, ||r||^2, stop test (iter > 0)
            // (fx_sums: outside an iteration no K3 has cleared max|r| for this finish)
            if (iter <= 0) BSLS_CHECK(clear_rmax(P, w, st));
            if (iter > 0) launch_k1<true, true, true>(P, iter, w, st);
            else launch_k1<true, true, false>(P, iter, w, st);
            break;
        default:
            return BSLS_E_ARG;
    }
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}

extern "C" int64_t bsls_bb_row_blocks(const bsls_bb_problem *p, int64_t *rows_per_block) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    if (rows_per_block)
        *rows_per_block = p->At.ent ? p->At.H : (int64_t)PANEL_WAVES * p->A.prow;
    return k1_row_blocks(*p);
}

extern "C" int bsls_bb_residual_rows(const bsls_bb_problem *p, int64_t iter, int64_t rb0,
                                     int64_t rb1, void *stream) {
    const int rc = check_problem_float(p);
    if (rc != BSLS_OK) return rc;
    const bsls_bb_problem &P = *p;
    if (rb0 < 0 || rb1 <= rb0 || rb1 > k1_row_blocks(P)) return BSLS_E_ARG;
    const BBWork w = bb_layout(P);
    launch_k1_partial(P, iter, w, (hipStream_t)stream, rb0, rb1);
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}

extern "C" int bsls_bb_prologue(const bsls_bb_problem *p, void *stream) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    const bsls_bb_problem &P = *p;
    hipStream_t st = (hipStream_t)stream;
    const BBWork w = bb_layout(P);
    int e;
    if ((e = bsls_bb_stage(p, 0, 0, stream)) != BSLS_OK) return e;
    if ((e = bsls_bb_stage(p, 5, 0, stream)) != BSLS_OK) return e;
    launch_k1<true, false, false>(P, 0, w, st);  // r(z0 + 1)
    BSLS_LAUNCH_CHECK();
    if ((e = bsls_bb_stage(p, 3, 0, stream)) != BSLS_OK) return e;  // g_prev -> g[0]
    if ((e = bsls_bb_stage(p, 6, 0, stream)) != BSLS_OK) return e;
    // (fx_sums: max|r| of r(z0 + 1) was K2's; r(z0)'s alone is iteration 1's)
    BSLS_CHECK(clear_rmax(P, w, st));
    launch_k1<true, true, false>(P, 0, w, st);  // r(z0), f(z0)
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}

extern "C" int bsls_bb_iterate(const bsls_bb_problem *p, int64_t first_iter, int64_t count,
                               void *stream) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    if (first_iter < 1 || count < 0) return BSLS_E_ARG;
    const bsls_bb_problem &P = *p;
    hipStream_t st = (hipStream_t)stream;
    const BBWork w = bb_layout(P);
    for (int64_t i = first_iter; i < first_iter + count; ++i) {
        const int zc = (int)((i - 1) & 1), zn = (int)(i & 1);
        launch_k2<true>(P, P.g[zc], P.g[zn], w, st);
        launch_k3(P, i, P.z[zc], P.g[zn], P.z[zn], w, st);
        launch_k1<true, true, true>(P, i, w, st);
        BSLS_LAUNCH_CHECK();
    }
    return BSLS_OK;
}

// ---- the link-part pipeline of the column-sharded schedule -------------------
// (include/bsls_hip.h bsls_bb_k2_part / bsls_bb_k1_rows; csrc/shard.hip
// bsls_bb_shard_iterate_parts drives them with the exchange of each part's
// rows of r on a second stream)
extern "C" int bsls_bb_k2_part(const bsls_bb_problem *p, int64_t iter, int part, void *stream) {
    const int rc = check_problem_float(p);
    if (rc != BSLS_OK) return rc;
    const bsls_bb_problem &P = *p;
    if (iter <= 0 || !P.ATt.ent || (P.ATt.layout & 3) == 0 || P.ATt.ngroups < 2 || part < 0 ||
        part >= P.ATt.ngroups || !P.wpart)
        return BSLS_E_ARG;
    if (P.rr_lo < 0 || P.rr_hi > P.m || P.rr_lo > P.rr_hi) return BSLS_E_ARG;
    const BBWork w = bb_layout(P);
    const int zc = (int)((iter - 1) & 1), zn = (int)(iter & 1);
    launch_k2<true, 2>(P, P.g[zc], P.g[zn], w, (hipStream_t)stream, iter, nullptr, part);
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}

extern "C" int bsls_bb_k1_rows(const bsls_bb_problem *p, int64_t iter, int64_t rb0, int64_t rb1,
                               void *stream) {
    const int rc = check_problem_float(p);
    if (rc != BSLS_OK) return rc;
    const bsls_bb_problem &P = *p;
    if (iter <= 0 || rb0 < 0 || rb1 <= rb0 || rb1 > k1_row_blocks(P)) return BSLS_E_ARG;
    launch_k1_partial(P, iter, bb_layout(P), (hipStream_t)stream, rb0, rb1, k1_init_folded(P));
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}
