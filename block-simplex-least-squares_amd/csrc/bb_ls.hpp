// bb_ls.hpp -- LBFGS.solve's weak Wolfe line search on the device, a tenant of
// the BB engine's kernels.  Part of bb.hip's translation unit: included there
// after the launchers (it needs launch_k1 / k2 / k3, and a translation unit of
// its own would instantiate every kernel twice), under its `using namespace
// bsls`.
//
// (python/LBFGS.py:9-53; include/bsls_hip.h bsls_lbfgs_ls_*).  One trial =
//   K3 on S1:  pt = clip01(PAVA(x - (-t) d)) = proj(x + t d) (the reference's
//              roundings: (-t) d = -(t d)), x_engine = colv N pt
//   K1 on S1:  r = A x + target, S1[FX] = f(pt)
//   armijo:    f(pt) >= fx + c1 t slope -> beta = t, t = (alpha + beta) / 2;
//              else open S2 for the curvature test
//   K2 on S2:  g(pt) = N'A'r -> gpt; the sums with g_prev = 0 and dz = d give
//              S2[DZDG] = d . g(pt)
//   curvature: d . g(pt) < c2 slope -> alpha = t, t = 2 alpha or (alpha +
//              beta) / 2; else accepted
// then the reference's two exits (|alpha - beta| <= 1e-14, ||t d|| <= 1e-8,
// the norm as |t| ||d||).  Every kernel of a trial is gated by the state, so
// the host enqueues trials in chunks and reads the state once per chunk.
// st[]: BSLS_LS_* slots.
#pragma once

namespace bsls {

__device__ __forceinline__ void ls_stop(double *st, double *S1, double *S2, double why) {
    st[BSLS_LS_STOP] = why;
    S1[BSLS_S_STOP] = 1.0;
    S2[BSLS_S_STOP] = 1.0;
}

// the exits after a new t (LBFGS.py:45-49), else the next trial's K3 step
__device__ __forceinline__ void ls_next(double *st, double *S1, double *S2, double tn) {
    st[BSLS_LS_T] = tn;
    if (fabs(st[BSLS_LS_LO] - st[BSLS_LS_HI]) <= 1e-14) ls_stop(st, S1, S2, BSLS_LS_BRACKET);
    else if (fabs(tn) * st[BSLS_LS_DNORM] <= 1e-8) ls_stop(st, S1, S2, BSLS_LS_SMALL);
    else S1[BSLS_S_DZDG] = -tn;
}

__global__ __launch_bounds__(256) void ls_begin_kernel(const double *__restrict__ d,
                                                       const double *__restrict__ gx, int64_t nz,
                                                       const double *fx, double *st,
                                                       double *S1, double *S2, double *part,
                                                       unsigned *tickets) {
    __shared__ double red[2 * 4];
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nz; i += gs) {
        const double di = d[i];
        v[0] += di * gx[i];
        v[1] += di * di;
    }
    block_sum<2>(v, red);
    double tot[2];
    if (last_block_sum<2>(v, part, tickets, tot, red) && threadIdx.x == 0) {
        const double f0 = *fx;    // (fx may point into st: the last search's st[FT])
        for (int k = 0; k < BSLS_LS_COUNT; ++k) st[k] = 0.0;
        for (int k = 0; k < BSLS_S_COUNT; ++k) S1[k] = S2[k] = 0.0;
        st[BSLS_LS_T] = 1.0;
        st[BSLS_LS_HI] = INFINITY;
        st[BSLS_LS_SLOPE] = tot[0];
        st[BSLS_LS_DNORM] = sqrt(tot[1]);
        st[BSLS_LS_FX] = f0;
        S1[BSLS_S_SUMDG] = 1.0;      // K3's t = S1[DZDG] / S1[DGDG] = -t
        S1[BSLS_S_DZDG] = -1.0;
        S1[BSLS_S_DGDG] = 1.0;
        S2[BSLS_S_STOP] = 1.0;
    }
}

__global__ void ls_armijo_kernel(double *st, double *S1, double *S2, double c1) {
    if (threadIdx.x != 0 || st[BSLS_LS_STOP] != 0.0) return;
    const double t = st[BSLS_LS_T], ft = S1[BSLS_S_FX];
    st[BSLS_LS_NTRIAL] += 1.0;
    st[BSLS_LS_TLAST] = t;
    st[BSLS_LS_FT] = ft;
    if (ft >= st[BSLS_LS_FX] + c1 * t * st[BSLS_LS_SLOPE]) {   // Armijo violated (LBFGS.py:26)
        st[BSLS_LS_HI] = t;
        S2[BSLS_S_STOP] = 1.0;
        ls_next(st, S1, S2, 0.5 * (st[BSLS_LS_LO] + t));
    } else {
        S2[BSLS_S_STOP] = 0.0;     // the curvature test needs g(pt)
    }
}

__global__ void ls_curv_kernel(double *st, double *S1, double *S2, double c2) {
    if (threadIdx.x != 0 || st[BSLS_LS_STOP] != 0.0 || S2[BSLS_S_STOP] != 0.0) return;
    const double t = st[BSLS_LS_T];
    S2[BSLS_S_STOP] = 1.0;
    st[BSLS_LS_DGT] = S2[BSLS_S_DZDG];
    if (S2[BSLS_S_DZDG] < c2 * st[BSLS_LS_SLOPE]) {            // curvature violated (:33)
        st[BSLS_LS_LO] = t;
        const double hi = st[BSLS_LS_HI];
        ls_next(st, S1, S2, (hi == INFINITY) ? 2 * t : 0.5 * (t + hi));
    } else {
        ls_stop(st, S1, S2, BSLS_LS_ACCEPTED);                  // both conditions pass (:39)
    }
}

// after an accepted search: y = g(pt) - gx, s = t d (LBFGS.py:100-106, the
// same elementwise roundings), y.s and g(pt).g(pt); gated on the state
__global__ __launch_bounds__(256) void ls_finish_kernel(const double *__restrict__ d,
                                                        const double *__restrict__ gx,
                                                        const double *__restrict__ gpt, int64_t nz,
                                                        double *st, double *y_out, double *s_out,
                                                        double *part, unsigned *tickets) {
    __shared__ double red[2 * 4];
    if (st[BSLS_LS_STOP] != (double)BSLS_LS_ACCEPTED || st[BSLS_LS_DONE] != 0.0) return;
    const double t = st[BSLS_LS_T];
    const int64_t gs = (int64_t)gridDim.x * blockDim.x;
    double v[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nz; i += gs) {
        const double gi = gpt[i];
        const double y = gi - gx[i], s = t * d[i];
        if (y_out) y_out[i] = y;
        if (s_out) s_out[i] = s;
        v[0] += y * s;
        v[1] += gi * gi;
    }
    block_sum<2>(v, red);
    double tot[2];
    if (last_block_sum<2>(v, part, tickets, tot, red) && threadIdx.x == 0) {
        st[BSLS_LS_YS] = tot[0];
        st[BSLS_LS_GG] = tot[1];
        st[BSLS_LS_DONE] = 1.0;
    }
}

}  // namespace bsls

extern "C" size_t bsls_lbfgs_ls_work_size(int64_t nz) {
    return (size_t)(((nz > 0 ? nz : 1) + 255) / 256 + 1) * 2 * sizeof(double);
}

static int check_ls(const bsls_ls_state *s) {
    if (!s || !s->x || !s->d || !s->gx || !s->pt || !s->gpt || !s->zero || !s->fx || !s->st ||
        !s->S1 || !s->S2 || !s->part || !s->tickets)
        return BSLS_E_ARG;
    return BSLS_OK;
}

extern "C" int bsls_lbfgs_ls_begin(const bsls_bb_problem *p, const bsls_ls_state *s, void *stream) {
    int rc = check_problem_float(p);
    if (rc != BSLS_OK || (rc = check_ls(s)) != BSLS_OK) return rc;
    constexpr int LS_GRID = 512;
    const int g = grid_for(p->nz, 256);
    ls_begin_kernel<<<g < LS_GRID ? g : LS_GRID, 256, 0, (hipStream_t)stream>>>(
        s->d, s->gx, p->nz, s->fx, s->st, s->S1, s->S2, s->part, s->tickets);
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}

extern "C" int bsls_lbfgs_ls_trials(const bsls_bb_problem *p, const bsls_ls_state *s,
                                    int64_t count, void *stream) {
    int rc = check_problem_float(p);
    if (rc != BSLS_OK || (rc = check_ls(s)) != BSLS_OK) return rc;
    if (count < 0) return BSLS_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const BBWork w = bb_layout(*p);
    // the trial's problems: S1 gates K3 / K1 (and takes f), S2 gates K2; no
    // stopping rule of their own (max_iter unreachable, no early exits)
    bsls_bb_problem P1 = *p, P2 = *p;
    P1.scal = s->S1;
    P2.scal = s->S2;
    P1.max_iter = P2.max_iter = INT64_MAX;
    P1.early_exit = P2.early_exit = 0;
    for (int64_t k = 0; k < count; ++k) {
        launch_k3(P1, 1, s->x, s->d, s->pt, w, st, 0, 1);
        BSLS_LAUNCH_CHECK();
        launch_k1<true, true, true>(P1, 1, w, st);
        BSLS_LAUNCH_CHECK();
        ls_armijo_kernel<<<1, 64, 0, st>>>(s->st, s->S1, s->S2, s->c1);
        launch_k2<true>(P2, s->zero, s->gpt, w, st, 1, s->d);
        BSLS_LAUNCH_CHECK();
        ls_curv_kernel<<<1, 64, 0, st>>>(s->st, s->S1, s->S2, s->c2);
        BSLS_LAUNCH_CHECK();
    }
    return BSLS_OK;
}

extern "C" int bsls_lbfgs_ls_finish(const bsls_bb_problem *p, const bsls_ls_state *s,
                                    double *y_out, double *s_out, void *stream) {
    int rc = check_problem_float(p);
    if (rc != BSLS_OK || (rc = check_ls(s)) != BSLS_OK) return rc;
    constexpr int LS_GRID = 512;
    const int g = grid_for(p->nz, 256);
    ls_finish_kernel<<<g < LS_GRID ? g : LS_GRID, 256, 0, (hipStream_t)stream>>>(
        s->d, s->gx, s->gpt, p->nz, s->st, y_out, s_out, s->part, s->tickets);
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}
