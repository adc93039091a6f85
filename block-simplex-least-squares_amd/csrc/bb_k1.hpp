// bb_k1.hpp -- K1 of the BB engine, r = A (N z) + target: the panel kernel, the
// tile kernel with its group sum and atomic forms, and the multi-GPU finish.
// Part of bb.hip's translation unit (the launches: bb_launch.hpp).
#pragma once

namespace bsls {

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

}  // namespace bsls
