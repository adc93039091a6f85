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
// bsls_bb_problem.reg_w adds the reference's weighted L2 regulariser
// (CrossValidation.py:140-148): a fourth kernel between K3 and K1 (bb_reg.hpp)
// leaves N'(w o (N z + x0)) for the next K2's epilogue and sum w (N z + x0)^2
// for the f that K1's finish records.
#include "pava.hpp"
#include "pava_long.hpp"
#include "pava_wave.hpp"
#include "panels.hpp"
#include "tiles.hpp"

// This file: the C entry points.  The engine itself, in the order its parts
// build on one another -- the workspace layout, the kernels' shared device
// helpers, the three kernel families, then the launchers and argument checks:
#include "bb_work.hpp"
#include "bb_device.hpp"
#include "bb_k1.hpp"
#include "bb_k2.hpp"
#include "bb_k3.hpp"
#include "bb_reg.hpp"
#include "bb_launch.hpp"

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

// What a stage asks of its call and which problems it takes, one row per
// stage id (include/bsls_hip.h bsls_stage); an id outside the table, or the
// unassigned 11, is BSLS_E_ARG.  fx_sums: the single-GCD stages only.  roww:
// the same without R_FINISH (||r||^2 of the stored w o is not the objective)
// and with K1_PARTIAL, which without target stays the unweighted A x.  reg
// (reg_w): the single-GCD stages, K1_PARTIAL included (no f, no gradient: the
// plain A x), without the stages that finish r apart from K1's walk.  A new stage gets a row: it
// inherits nothing.
struct StageRule {
    bool known, needs_iter, fx_sums, roww, reg;   // needs_iter: iter >= 1
};
static const StageRule STAGE_RULES[] = {
    /* BSLS_STAGE_RESET             0 */ {true, false, true, true, true},
    /* BSLS_STAGE_K1_PARTIAL        1 */ {true, false, false, true, true},
    /* BSLS_STAGE_R_FINISH_TARGET   2 */ {true, false, false, false, false},
    /* BSLS_STAGE_K2                3 */ {true, false, true, true, true},
    /* BSLS_STAGE_K3                4 */ {true, true, true, true, true},
    /* BSLS_STAGE_Z_PLUS_ONE        5 */ {true, false, true, true, true},
    /* BSLS_STAGE_Z2X               6 */ {true, false, true, true, true},
    /* BSLS_STAGE_K1                7 */ {true, false, true, true, true},
    /* BSLS_STAGE_K2_R_FINISH       8 */ {true, true, false, false, false},
    /* BSLS_STAGE_R_FINISH          9 */ {true, false, true, false, false},
    /* BSLS_STAGE_K2_RR_SLICE      10 */ {true, true, false, false, false},
    /* unassigned                  11 */ {false, false, false, false, false},
    /* BSLS_STAGE_RECORD           12 */ {true, true, false, false, false},
    /* BSLS_STAGE_K3_RECORD        13 */ {true, true, false, false, false},
    /* BSLS_STAGE_K1_PARTIAL_INITED 14 */ {true, true, false, false, false},
    /* BSLS_STAGE_K3_RECORD_INIT   15 */ {true, true, false, false, false},
};
static_assert(sizeof(STAGE_RULES) / sizeof(STAGE_RULES[0]) == BSLS_STAGE_K3_RECORD_INIT + 1,
              "one row per stage id");

extern "C" int bsls_bb_stage(const bsls_bb_problem *p, int stage, int64_t iter, void *stream) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    const bsls_bb_problem &P = *p;
    hipStream_t st = (hipStream_t)stream;
    const BBWork w = bb_layout(P);
    const int zc = (int)((iter - 1) & 1), zn = (int)(iter & 1);
    if (stage < 0 || stage > BSLS_STAGE_K3_RECORD_INIT) return BSLS_E_ARG;
    const StageRule &rule = STAGE_RULES[stage];
    if (!rule.known || (rule.needs_iter && iter <= 0) || (P.fx_sums && !rule.fx_sums) ||
        (P.roww && !rule.roww) || (P.reg_w && !rule.reg))
        return BSLS_E_ARG;
    switch (stage) {
        case BSLS_STAGE_RESET:  // reset scalars and tickets
            BSLS_CHECK(hipMemsetAsync(P.scal, 0, BSLS_S_COUNT * sizeof(double), st));
            BSLS_CHECK(hipMemsetAsync(P.work, 0, (size_t)((char *)w.p1 - (char *)P.work), st));
            BSLS_CHECK(clear_rmax(P, w, st));
            return BSLS_OK;
        case BSLS_STAGE_K1_PARTIAL:  // r_partial = A_g x_g (+ target on the shard_role 1 rank)
            launch_k1_partial(P, iter, w, st);
            break;
        case BSLS_STAGE_R_FINISH_TARGET:  // r += target, ||r||^2, stop test
        case BSLS_STAGE_R_FINISH:         // ||r||^2, stop test (r already the residual)
            launch_bb_r_finish(P, iter, w, st, stage == BSLS_STAGE_R_FINISH_TARGET ? 1 : 0);
            break;
        case BSLS_STAGE_K2_R_FINISH:  // K2 with R_FINISH of iteration iter - 1 folded in
            launch_k2<true, 1>(P, P.g[zc], P.g[zn], w, st, iter);
            break;
        case BSLS_STAGE_K2_RR_SLICE:  // K2 with this rank's slice of ||r||^2 (sliced schedule)
            if (P.rr_lo < 0 || P.rr_hi > P.m || P.rr_lo > P.rr_hi) return BSLS_E_ARG;
            launch_k2<true, 2>(P, P.g[zc], P.g[zn], w, st, iter);
            break;
        case BSLS_STAGE_K3_RECORD:  // RECORD folded into K3 (one launch fewer)
            launch_k3(P, iter, P.z[zc], P.g[zn], P.z[zn], w, st, 1);
            break;
        case BSLS_STAGE_K3_RECORD_INIT:  // + the next K1_PARTIAL_INITED's r initialisation
            launch_k3(P, iter, P.z[zc], P.g[zn], P.z[zn], w, st, 1, 0,
                      k1_init_folded(P) ? 1 : 0);
            break;
        case BSLS_STAGE_K1_PARTIAL_INITED:  // (r already initialised when it folds)
            launch_k1_partial(P, iter, w, st, 0, -1, k1_init_folded(P));
            break;
        case BSLS_STAGE_RECORD:  // f / stopping test of iteration iter - 1 (after the
                                 // sums' all-reduce)
            launch_bb_shard_record(P, iter, st);
            break;
        case BSLS_STAGE_K2:  // g = N'A'r (+ sums)
            if (iter > 0) launch_k2<true>(P, P.g[zc], P.g[zn], w, st);
            else launch_k2<false>(P, nullptr, P.g[0], w, st);
            break;
        case BSLS_STAGE_K3:  // t, projection, x
            launch_k3(P, iter, P.z[zc], P.g[zn], P.z[zn], w, st);
            break;
        case BSLS_STAGE_Z_PLUS_ONE:  // z[1] = z[0] + 1; x = N z[1]
            launch_bb_plus_one(P, P.z[0], P.z[1], w, st);
            BSLS_LAUNCH_CHECK();
            launch_bb_z2x(P, P.z[1], st);
            break;
        case BSLS_STAGE_Z2X:  // x = N z[0]
            launch_bb_z2x(P, P.z[0], st);
            break;
        case BSLS_STAGE_K1:  // single GCD K1: r = A x + target, ||r||^2, stop test (iter > 0)
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
    if ((e = bsls_bb_stage(p, BSLS_STAGE_RESET, 0, stream)) != BSLS_OK) return e;
    if ((e = bsls_bb_stage(p, BSLS_STAGE_Z_PLUS_ONE, 0, stream)) != BSLS_OK) return e;
    if (P.reg_w) launch_bb_reg(P, P.z[1], 0, st);  // reg_g(z0 + 1) for g_prev
    launch_k1<true, false, false>(P, 0, w, st);  // r(z0 + 1)
    BSLS_LAUNCH_CHECK();
    if ((e = bsls_bb_stage(p, BSLS_STAGE_K2, 0, stream)) != BSLS_OK) return e;  // g_prev -> g[0]
    if ((e = bsls_bb_stage(p, BSLS_STAGE_Z2X, 0, stream)) != BSLS_OK) return e;
    // (fx_sums: max|r| of r(z0 + 1) was K2's; r(z0)'s alone is iteration 1's)
    BSLS_CHECK(clear_rmax(P, w, st));
    if (P.reg_w) launch_bb_reg(P, P.z[0], 0, st);  // reg_g(z0), and f(z0)'s second term
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
        if (P.reg_w) launch_bb_reg(P, P.z[zn], i, st);
        launch_k1<true, true, true>(P, i, w, st);
        BSLS_LAUNCH_CHECK();
    }
    return BSLS_OK;
}

extern "C" size_t bsls_bb_reg_work_size(int64_t n) { return reg_work_bytes(n > 0 ? n : 1); }

extern "C" int bsls_bb_reg(const bsls_bb_problem *p, int zbuf, int64_t iter, void *stream) {
    const int rc = check_problem(p);
    if (rc != BSLS_OK) return rc;
    if (!p->reg_w || zbuf < 0 || zbuf > 1) return BSLS_E_ARG;
    launch_bb_reg(*p, p->z[zbuf], iter, (hipStream_t)stream);
    BSLS_LAUNCH_CHECK();
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
