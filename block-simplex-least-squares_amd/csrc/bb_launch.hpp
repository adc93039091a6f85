// bb_launch.hpp -- the host side of the BB engine's kernels: one launcher per
// kernel (its grid, block, LDS bytes and allow_lds written once), the form a
// K1 launch takes (k1_form), the launchers the entry points and the tenants
// call (launch_k1 / launch_k1_partial / launch_k2 / launch_k3), and the
// argument checks.  Part of bb.hip's translation unit.
#pragma once

namespace bsls {

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

// ---- K1 ----------------------------------------------------------------------

// K1's row blocks: panels 16 panels each, tiles H rows each
static int64_t k1_row_blocks(const bsls_bb_problem &P) {
    return P.At.ent ? P.At.nrb : (P.A.npanels + PANEL_WAVES - 1) / PANEL_WAVES;
}

// the rows [r0, r1) of the tile image's row blocks [rb0, rb1)
static void k1_tile_rows(const bsls_bb_problem &P, int64_t rb0, int64_t rb1, int64_t &r0,
                         int64_t &r1) {
    r0 = rb0 * P.At.H;
    r1 = (rb1 * P.At.H < P.m) ? rb1 * P.At.H : P.m;
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

// fx_sums and roww change how K1 finishes the residual, so they apply to the
// launches that finish one: target added, and either reduced to f or outside
// an iteration (the iteration's K1, stage 7, the prologue's two).  The other
// launches -- no target (stage 1 on one GCD, DORE, the line search's), or a
// column shard's iteration K1 without the reduction -- come from entry points
// that refuse such a problem (check_problem_float, bsls_bb_stage's table) or,
// stage 1 under roww, stay the unweighted A x; their FX / RW kernels are not
// instantiated.
constexpr bool k1_finishes_residual(bool add, bool reduce, bool iter) {
    return add && (reduce || !iter);
}

// The form a K1 launch takes: its kernels, in order.  As a template argument
// of a launcher it also names the kernel's variant (ATOM, FX, RW).
enum K1Form {
    K1_PANELS,           // bb_k1
    K1_PANELS_WEIGHTED,  // bb_k1<RW>
    K1_TILES,            // bb_k1t; several groups: + bb_k1_sum
    K1_TILES_ATOMIC,     // bb_k1_init (unless folded), bb_k1t<ATOM>; REDUCE: + bb_r_finish
    K1_TILES_FIXED,      // bb_k1t<FX>; several groups: + bb_k1_sum<FX>
    K1_TILES_WEIGHTED,   // one group: bb_k1t<RW>; several: bb_k1t, bb_k1_sum<RW>
};

// (check_problem: fx_sums needs dealt tiles and never the atomic K1; roww never
// fx_sums or the atomic K1)
static K1Form k1_form(const bsls_bb_problem &P, bool add, bool reduce, bool iter) {
    const bool finish = k1_finishes_residual(add, reduce, iter);
    if (!P.At.ent) return (finish && P.roww) ? K1_PANELS_WEIGHTED : K1_PANELS;
    if (P.At.ngroups > 1 && k1_atomic(P, reduce)) return K1_TILES_ATOMIC;
    if (finish && P.fx_sums) return K1_TILES_FIXED;
    if (finish && P.roww) return K1_TILES_WEIGHTED;
    return K1_TILES;
}

// row blocks [rb0, rb1) of K1 (the whole matrix unless a multi-GPU driver
// all-reduces r part by part behind it); REDUCE needs the whole matrix
template <int MODE, bool ITER, bool ADD, bool REDUCE, K1Form FORM>
static void launch_bb_k1(const bsls_bb_problem &P, int64_t iter, const BBWork &w, hipStream_t st,
                         int64_t rb0, int64_t rb1) {
    constexpr bool RW = FORM == K1_PANELS_WEIGHTED;
    allow_lds(bb_k1<MODE, ITER, ADD, REDUCE, RW>);
    bb_k1<MODE, ITER, ADD, REDUCE, RW><<<(int)(P.A.ngroups * (rb1 - rb0)), 1024,
                                         panel_lds_bytes(P.A), st>>>(P, iter, w.tkrb, w.p1, w.tk1,
                                                                     rb0);
}

// (FX: two words per row in LDS, and max|r| for the one-group finish)
template <int MODE, bool ITER, bool ADD, bool REDUCE, K1Form FORM>
static void launch_bb_k1t(const bsls_bb_problem &P, int64_t iter, const BBWork &w, hipStream_t st,
                          int64_t rb0, int64_t rb1) {
    constexpr bool ATOM = FORM == K1_TILES_ATOMIC, FX = FORM == K1_TILES_FIXED,
                   RW = FORM == K1_TILES_WEIGHTED;
    allow_lds(bb_k1t<MODE, ITER, ADD, REDUCE, ATOM, FX, RW>);
    bb_k1t<MODE, ITER, ADD, REDUCE, ATOM, FX, RW><<<(int)((rb1 - rb0) * P.At.ngroups),
                                                    BSLS_TILE_THREADS,
                                                    tile_lds_doubles(P.At, FX) * 8, st>>>(
        P, iter, w.p1, w.tk1, rb0, FX ? w.rmax : nullptr);
}

// bb_k1_sum behind a several-group bb_k1t over row blocks [rb0, rb1): rows in
// 16-B pairs (W = 2) where every pair is aligned in rpart, target, r and (RW)
// roww
template <bool ITER, bool ADD, bool REDUCE, K1Form FORM>
static void launch_bb_k1_sum(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                             hipStream_t st, int64_t rb0, int64_t rb1) {
    constexpr bool FX = FORM == K1_TILES_FIXED, RW = FORM == K1_TILES_WEIGHTED;
    int64_t r0, r1;
    k1_tile_rows(P, rb0, rb1, r0, r1);
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

template <bool ITER, bool ADD>
static void launch_bb_k1_init(const bsls_bb_problem &P, hipStream_t st, int64_t rb0, int64_t rb1) {
    int64_t r0, r1;
    k1_tile_rows(P, rb0, rb1, r0, r1);
    const int gi = grid_for(r1 - r0, 256);
    // one row per thread (the grid-stride form at 1024 workgroups gave each
    // thread 4 rows at m = 1M; the rehearsed iteration measured the same
    // either way, 149.3-149.8 us)
    bb_k1_init<ITER, ADD><<<gi < 16384 ? gi : 16384, 256, 0, st>>>(P, r0, r1);
}

// ||r||^2, f and the stop test over all of r (add_target: r += target first):
// the atomic K1's reduction, stages 2 and 9
static void launch_bb_r_finish(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                               hipStream_t st, int add_target) {
    const int g = grid_for(P.m, 256);
    bb_r_finish<<<g < R_FINISH_GRID ? g : R_FINISH_GRID, 256, 0, st>>>(P, iter, w.pf, w.tkf,
                                                                      add_target);
}

template <int MODE, bool ADD, bool REDUCE, bool ITER>
static void launch_k1_mode(const bsls_bb_problem &P, int64_t iter, const BBWork &w,
                           hipStream_t st, int64_t rb0, int64_t rb1, bool skip_init) {
    const K1Form form = k1_form(P, ADD, REDUCE, ITER);
    const bool several = P.At.ngroups > 1;
    if (form == K1_TILES_ATOMIC) {
        if (!skip_init) launch_bb_k1_init<ITER, ADD>(P, st, rb0, rb1);
        launch_bb_k1t<MODE, ITER, ADD, false, K1_TILES_ATOMIC>(P, iter, w, st, rb0, rb1);
        if (REDUCE) launch_bb_r_finish(P, iter, w, st, 0);
        return;
    }
    if constexpr (k1_finishes_residual(ADD, REDUCE, ITER)) {
        if (form == K1_TILES_FIXED) {
            // the fixed-point walk, and the finish that keeps max|r|
            launch_bb_k1t<MODE, ITER, ADD, REDUCE, K1_TILES_FIXED>(P, iter, w, st, rb0, rb1);
            if (several)
                launch_bb_k1_sum<ITER, ADD, REDUCE, K1_TILES_FIXED>(P, iter, w, st, rb0, rb1);
            return;
        }
        if (form == K1_TILES_WEIGHTED) {
            // one group finishes weighted in the walk's kernel; several leave the
            // float form's partials, and bb_k1_sum weighs
            if (several) {
                launch_bb_k1t<MODE, ITER, ADD, REDUCE, K1_TILES>(P, iter, w, st, rb0, rb1);
                launch_bb_k1_sum<ITER, ADD, REDUCE, K1_TILES_WEIGHTED>(P, iter, w, st, rb0, rb1);
            } else {
                launch_bb_k1t<MODE, ITER, ADD, REDUCE, K1_TILES_WEIGHTED>(P, iter, w, st, rb0,
                                                                          rb1);
            }
            return;
        }
        if (form == K1_PANELS_WEIGHTED) {
            launch_bb_k1<MODE, ITER, ADD, REDUCE, K1_PANELS_WEIGHTED>(P, iter, w, st, rb0, rb1);
            return;
        }
    }
    if (form == K1_PANELS) {
        launch_bb_k1<MODE, ITER, ADD, REDUCE, K1_PANELS>(P, iter, w, st, rb0, rb1);
        return;
    }
    launch_bb_k1t<MODE, ITER, ADD, REDUCE, K1_TILES>(P, iter, w, st, rb0, rb1);
    if (several) launch_bb_k1_sum<ITER, ADD, REDUCE, K1_TILES>(P, iter, w, st, rb0, rb1);
}

// (MODE 0: a scaled incidence, K3 wrote colv * N z; 1: stored values)
template <bool ADD, bool REDUCE, bool ITER>
static void launch_k1(const bsls_bb_problem &P, int64_t iter, const BBWork &w, hipStream_t st,
                      int64_t rb0 = 0, int64_t rb1 = -1, bool skip_init = false) {
    if (rb1 < 0) rb1 = k1_row_blocks(P);
    if (P.colv) launch_k1_mode<0, ADD, REDUCE, ITER>(P, iter, w, st, rb0, rb1, skip_init);
    else launch_k1_mode<1, ADD, REDUCE, ITER>(P, iter, w, st, rb0, rb1, skip_init);
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

// ---- K2 ----------------------------------------------------------------------

// (dz: the vector the ITER sums dot with delta_g -- the workspace's z - z_prev
// unless given: the line search passes its direction d, with g_prev = 0)
// (REG: bsls_bb_problem.reg_w -- the launches that refuse it never get here
// with it set: check_problem_float, bsls_bb_stage's table)
template <int MODE, bool ITER, int FUSE, bool REG = false>
static void launch_bb_k2(const bsls_bb_problem &P, const double *gp, double *gout,
                         const BBWork &w, hipStream_t st, int64_t iter, const double *dz) {
    if constexpr (FUSE == 0 && !REG) {
        if (P.reg_w) {
            launch_bb_k2<MODE, ITER, 0, true>(P, gp, gout, w, st, iter, dz);
            return;
        }
    }
    allow_lds(bb_k2<MODE, ITER, FUSE, REG>);
    bb_k2<MODE, ITER, FUSE, REG><<<grid_for(P.AT.npanels, PANEL_WAVES), 1024,
                                   panel_lds_bytes(P.AT), st>>>(P, dz, gp, gout, w.p2, w.tk2,
                                                                iter);
}

// (gsel >= 0: one column group, a workgroup per row block; two words per row in
// LDS for FX's integer sums and MODE 2's scales beside the sums)
template <int MODE, bool ITER, int FUSE, int CV, bool FX, bool REG = false>
static void launch_bb_k2t(const bsls_bb_problem &P, const double *gp, double *gout,
                          const BBWork &w, hipStream_t st, int64_t iter, const double *dz,
                          int gsel) {
    allow_lds(bb_k2t<MODE, ITER, FUSE, CV, FX, REG>);
    bb_k2t<MODE, ITER, FUSE, CV, FX, REG><<<(int)(gsel >= 0 ? P.ATt.nrb
                                                            : P.ATt.nrb * P.ATt.ngroups),
                                            BSLS_TILE_THREADS,
                                            tile_lds_doubles(P.ATt, FX || MODE == 2) * 8, st>>>(
        P, dz, gp, gout, w.p2, w.tk2, w.tk2rb, iter, gsel, FX ? w.rmax : nullptr);
}

template <int MODE, bool ITER, int FUSE, int CV>
static void launch_k2t_cv(const bsls_bb_problem &P, const double *gp, double *gout,
                          const BBWork &w, hipStream_t st, int64_t iter, const double *dz,
                          int gsel) {
    if constexpr (FUSE == 0 && (MODE == 1 || MODE == 3)) {
        // fx_sums (check_problem: a dealt image; bsls_bb_k2_part rejects it)
        if (P.fx_sums && gsel < 0) {
            launch_bb_k2t<MODE, ITER, 0, CV, true>(P, gp, gout, w, st, iter, dz, gsel);
            return;
        }
    }
    if constexpr (FUSE == 0) {
        // reg_w (check_problem: never with fx_sums; bsls_bb_k2_part rejects it)
        if (P.reg_w && gsel < 0) {
            launch_bb_k2t<MODE, ITER, 0, CV, false, true>(P, gp, gout, w, st, iter, dz, gsel);
            return;
        }
    }
    launch_bb_k2t<MODE, ITER, FUSE, CV, false>(P, gp, gout, w, st, iter, dz, gsel);
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
        launch_bb_k2<2, ITER, FUSE>(P, gp, gout, w, st, iter, dz);
    } else {
        launch_bb_k2<1, ITER, FUSE>(P, gp, gout, w, st, iter, dz);
    }
}

// stage 12: f and the stopping test of iteration iter - 1, one thread
static void launch_bb_shard_record(const bsls_bb_problem &P, int64_t iter, hipStream_t st) {
    bb_shard_record<<<1, 64, 0, st>>>(P, iter);
}

// ---- K3 ----------------------------------------------------------------------

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
static void launch_bb_k3(const bsls_bb_problem &P, int64_t iter, const double *zc,
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
    if (P.colv && P.colv_codec == 2) launch_bb_k3<2>(P, iter, zc, g, zn, w, st, rec, slot, kinit);
    else if (P.colv && P.colv_codec == 1)
        launch_bb_k3<1>(P, iter, zc, g, zn, w, st, rec, slot, kinit);
    else launch_bb_k3<0>(P, iter, zc, g, zn, w, st, rec, slot, kinit);
    if (P.long_packs && P.nlong > 0)
        bb_k3_long<<<(int)P.nlong, LONG_T, 0, st>>>(P, iter, zc, g, zn, w.dz);
}

// zn = z + 1 (and dz = 1) over the nz entries: the prologue's second point
static void launch_bb_plus_one(const bsls_bb_problem &P, const double *z, double *zn,
                               const BBWork &w, hipStream_t st) {
    bb_plus_one<<<grid_for(P.nz > 0 ? P.nz : 1, 256), 256, 0, st>>>(z, zn, w.dz, P.nz);
}

// x = N z (colv * N z for a scaled incidence)
static void launch_bb_z2x(const bsls_bb_problem &P, const double *z, hipStream_t st) {
    bb_z2x<<<grid_for(P.n, 256), 256, 0, st>>>(P, z);
}

// ---- argument checks ---------------------------------------------------------

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
    // the regulariser: the whole problem on this GCD, float row sums, ordered
    // group sums (composes with roww), and its two buffers
    if (p->reg_w && (p->shard_role != 0 || p->r_fx != 0.0 || p->fx_sums != 0 ||
                     p->k1_atomic == 2 || !p->reg_g || !p->reg_work))
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

// the entry points that fx_sums, roww and reg_w do not cover (include/bsls_hip.h)
static int check_problem_float(const bsls_bb_problem *p) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    return (p->fx_sums || p->roww || p->reg_w) ? BSLS_E_ARG : BSLS_OK;
}

}  // namespace bsls
