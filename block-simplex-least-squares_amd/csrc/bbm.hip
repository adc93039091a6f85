// bbm.hip -- batched z-space BB: R <= 8 problems in lockstep over one CSR
// image of A and of A' (struct bsls_bbm_problem, include/bsls_hip.h).
//
// Per iteration i (python/BB.py:21-40 for every running problem j):
//   bbm_spmm   w = A' r                    interleaved n x RP
//   bbm_grad   g = N' w -> stacked, dg, the four BB sums, t_j, BB.py:25's exit
//   bbm_step   y = z - t_j g               stacked
//   bsls_isotonic_packs(y)                 the planned bit-exact PAVA, unchanged
//   bbm_x      z = clip01(y), dz, x = N z  interleaved n x RP
//   bbm_spmm   r = w (A x + target), f_j, solvers.stopping per problem
//
// The SpMM: a lane owns one (entry, problem) pair.  A row takes G lanes (a
// power of two, RP <= G <= 64, from the mean row length), i.e. G / RP entry
// slots of RP lanes; slot e walks entries e, e + G/RP, ... of the row and each
// entry's gather is the RP contiguous doubles in[idx * RP ..] -- one request
// of 8 RP bytes where the single-problem walk makes one of 8.  The slots are
// then added across lanes in a fixed xor tree.  The index and value of an
// entry are read once for all RP problems.
//
// Freezing: every store into a problem's z, g, dz, x, r or scalars is gated on
// its scal[j][STOP], read at the kernel's start (the only writers of STOP are
// the last workgroups of bbm_grad and of the finish, after every workgroup of
// their launch has read it).  y is scratch: the PAVA runs over all of it, and
// a stopped column's y is simply not read back.
#include "bbm.hpp"

using namespace bsls;

namespace {

__device__ __forceinline__ double *col_scal(const bsls_bbm_problem &P, int j) {
    return P.scal + (size_t)j * BSLS_S_COUNT;
}

// solvers.py:40-63 for one problem (bb.hip bb_stop_reason)
__device__ __forceinline__ int bbm_stop_reason(const bsls_bbm_problem &P, int64_t iter, double fx,
                                               double gg, double dgdg) {
    if (iter >= P.max_iter) return BSLS_STOP_MAXITER;
    if (P.early_exit) {
        const double gn = sqrt(gg);
        if (gn * gn <= P.opt_tol * (1 + fabs(fx))) return BSLS_STOP_GRAD;
        if (sqrt(dgdg) == 0) return BSLS_STOP_DG;
    }
    return 0;
}

// FIN 0: out = sum.  FIN 1: the A-side row finish, o = sum + target, r = o,
// rr_j = sum o^2.  FIN 2: the weighted finish (bb.hip k1_weigh): r = w o, an
// exact 0.0 where w == 0 whatever o is, rr_j = sum w o^2, held_j = sum of o^2
// over the w == 0 rows.  With iter > 0 stopped columns are not written and
// the last workgroup records iteration iter and runs the stop test.
template <int RP, int FIN>
__global__ __launch_bounds__(BBM_T) void bbm_spmm(bsls_bbm_problem P,
                                                  const int64_t *__restrict__ indptr,
                                                  const int32_t *__restrict__ idx,
                                                  const double *__restrict__ val,
                                                  const double *__restrict__ in,
                                                  double *__restrict__ out, int64_t rows, int G,
                                                  int64_t iter, double *part, unsigned *tickets) {
    const int t = threadIdx.x;
    const int lg = t & (G - 1);           // lane within the row's group
    const int j = lg & (RP - 1);          // == t % RP: the thread's problem
    const int e = lg / RP;                // entry slot
    const int E = G / RP;
    const int gpb = BBM_T / G;            // rows per workgroup and pass
    const bool iterating = iter > 0;
    const bool live = !iterating || col_scal(P, j)[BSLS_S_STOP] == 0.0;
    double mine[2] = {0.0, 0.0};
    for (int64_t row = (int64_t)blockIdx.x * gpb + t / G; row < rows;
         row += (int64_t)gridDim.x * gpb) {
        const int64_t k0 = indptr[row], k1 = indptr[row + 1];
        double acc = 0.0;
        for (int64_t k = k0 + e; k < k1; k += E)
            acc += val[k] * in[(int64_t)idx[k] * RP + j];
        for (int o = G >> 1; o >= RP; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
        if (lg < RP) {
            const int64_t at = row * RP + j;
            if constexpr (FIN == 0) {
                out[at] = acc;
            } else {
                const double o = acc + P.target[at];
                double wo = o;
                if constexpr (FIN == 2) {
                    const double w = P.roww[at];
                    const bool held = (w == 0.0);
                    wo = held ? 0.0 : w * o;
                    mine[0] += held ? 0.0 : o * wo;
                    mine[1] += held ? o * o : 0.0;
                } else {
                    mine[0] += o * o;
                }
                if (live) out[at] = wo;
            }
        }
    }
    if constexpr (FIN != 0) {
        constexpr int NV = 2 * RP;
        __shared__ double red[NV * (BBM_T / WAVE)];
        double v[NV], tot[NV];
        bbm_spread<RP, 2>(mine, j, v);
        block_sum<NV>(v, red);
        if (last_block_sum<NV>(v, part, tickets, tot, red) && t == 0) {
            // (the totals through LDS: indexed by a runtime column below)
#pragma unroll
            for (int k = 0; k < NV; ++k) red[k] = tot[k];
            for (int c = 0; c < (int)P.R; ++c) {
                double *s = col_scal(P, c);
                if (iterating && s[BSLS_S_STOP] != 0.0) continue;
                const double rr = red[2 * c];
                const double nr = sqrt(rr);
                const double fx = 0.5 * (nr * nr);   // 0.5 * la.norm(r)**2, main.py:53
                s[BSLS_S_RR] = rr;
                s[BSLS_S_FX] = fx;
                if constexpr (FIN == 2) s[BSLS_S_HELD] = red[2 * c + 1];
                if (iterating) {
                    s[BSLS_S_ITER] = (double)iter;
                    s[BSLS_S_ZBUF] = (double)(iter & 1);
                    const int reason =
                        bbm_stop_reason(P, iter, fx, s[BSLS_S_GG], s[BSLS_S_DGDG]);
                    if (reason) s[BSLS_S_STOP] = (double)reason;
                }
            }
        }
    }
}

// g = N' w, (N' w)_i = w[x_i] - w[x_i + 1] (bsls_nt_apply), from the
// interleaved w to the stacked g.  iter > 0: dg = g - g_prev, dz, the four
// sums per problem (block tree, then the last workgroup in index order), t_j,
// BB.py:25's exact-zero exit and BB.py:30's warning count.
template <int RP>
__global__ __launch_bounds__(BBM_T) void bbm_grad(bsls_bbm_problem P, int64_t iter,
                                                  const double *__restrict__ gprev,
                                                  double *__restrict__ gout, double *part,
                                                  unsigned *tickets) {
    const int t = threadIdx.x;
    const int j = t & (RP - 1);
    const bool iterating = iter > 0;
    const bool live = !iterating || col_scal(P, j)[BSLS_S_STOP] == 0.0;
    double mine[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t total = P.nz * RP;
    for (int64_t q = (int64_t)blockIdx.x * BBM_T + t; q < total; q += (int64_t)gridDim.x * BBM_T) {
        const int64_t i = q / RP;
        if (!live) continue;
        const int64_t xi = P.zx[i];
        const double gv = P.w[xi * RP + j] - P.w[(xi + 1) * RP + j];
        const int64_t at = (int64_t)j * P.nz + i;
        if (iterating) {
            const double dg = gv - gprev[at];
            const double dzv = P.dz[at];
            mine[0] += dg;
            mine[1] += dzv * dg;
            mine[2] += dg * dg;
            mine[3] += gv * gv;
        }
        gout[at] = gv;
    }
    if (!iterating) return;
    constexpr int NV = 4 * RP;
    __shared__ double red[NV * (BBM_T / WAVE)];
    double v[NV], tot[NV];
    bbm_spread<RP, 4>(mine, j, v);
    block_sum<NV>(v, red);
    if (last_block_sum<NV>(v, part, tickets, tot, red) && t == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[k] = tot[k];
        for (int c = 0; c < (int)P.R; ++c) {
            double *s = col_scal(P, c);
            if (s[BSLS_S_STOP] != 0.0) continue;
            const double *tc = red + 4 * c;
            s[BSLS_S_SUMDG] = tc[0];
            s[BSLS_S_DZDG] = tc[1];
            s[BSLS_S_DGDG] = tc[2];
            s[BSLS_S_GG] = tc[3];
            if (P.early_exit && tc[0] == 0.0) {   // BB.py:25
                s[BSLS_S_STOP] = (double)BSLS_STOP_NOCHANGE;
                s[BSLS_S_ITER] = (double)iter;
                s[BSLS_S_ZBUF] = (double)((iter - 1) & 1);
                continue;
            }
            const double tj = tc[1] / tc[2];
            s[BSLS_S_T] = tj;
            if (fabs(tj) <= 1e-10 || fabs(tj) > 1e10) s[BSLS_S_WARN] += 1.0;
        }
    }
}

// y = z - t_j g (BB.py:32), problem blockIdx.y
__global__ __launch_bounds__(BBM_T) void bbm_step(bsls_bbm_problem P,
                                                  const double *__restrict__ zc,
                                                  const double *__restrict__ g) {
    const int j = blockIdx.y;
    const double *s = col_scal(P, j);
    if (s[BSLS_S_STOP] != 0.0) return;
    const double tj = s[BSLS_S_T];
    const int64_t i = (int64_t)blockIdx.x * BBM_T + threadIdx.x;
    if (i >= P.nz) return;
    const int64_t at = (int64_t)j * P.nz + i;
    P.y[at] = zc[at] - tj * g[at];
}

// x = N z per block: v - prev, prev = 0.0 at a block's first entry, 0.0 -
// z_last at its last (bb.hip bb_z2x).  CLIP (the iteration): z = clip01(y)
// (main.py:65) into zn with dz = z - zc, live problems only; else x = N src
// for every column.
template <int RP, bool CLIP>
__global__ __launch_bounds__(BBM_T) void bbm_x(bsls_bbm_problem P, const double *__restrict__ src,
                                               const double *__restrict__ zc,
                                               double *__restrict__ zn) {
    const int64_t q = (int64_t)blockIdx.x * BBM_T + threadIdx.x;
    const int j = threadIdx.x & (RP - 1);
    const int64_t i = q / RP;
    if (i >= P.n) return;
    if (CLIP && col_scal(P, j)[BSLS_S_STOP] != 0.0) return;
    const int32_t jz = P.xz[i];
    const int32_t jp = (i > 0) ? P.xz[i - 1] : -1;
    const int64_t base = (int64_t)j * P.nz;
    double v = 0.0, prev = 0.0;
    if (jz >= 0) v = CLIP ? clip01(src[base + jz]) : src[base + jz];
    if (jp >= 0) prev = CLIP ? clip01(src[base + jp]) : src[base + jp];
    P.x[i * RP + j] = v - prev;
    if (CLIP && jz >= 0) {
        zn[base + jz] = v;
        P.dz[base + jz] = v - zc[base + jz];   // the next bbm_grad's z - z_prev
    }
}

// BB.py:19: x_prev = x + 1 -> z[1], and iteration 1's z - z_prev
__global__ __launch_bounds__(BBM_T) void bbm_plus_one(const double *__restrict__ a,
                                                      double *__restrict__ o,
                                                      double *__restrict__ dz, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * BBM_T + threadIdx.x;
    if (i < count) {
        const double v = a[i], w = v + 1;
        o[i] = w;
        dz[i] = v - w;
    }
}

// scal = 0; the padding columns start stopped
__global__ void bbm_reset(bsls_bbm_problem P) {
    const int q = threadIdx.x;
    if (q >= (int)P.RP * BSLS_S_COUNT) return;
    const int j = q / BSLS_S_COUNT, s = q % BSLS_S_COUNT;
    P.scal[q] = (s == BSLS_S_STOP && j >= (int)P.R) ? (double)BSLS_STOP_MAXITER : 0.0;
}

int check_bbm(const bsls_bbm_problem *p) {
    if (!p) return BSLS_E_ARG;
    const bsls_bbm_problem &P = *p;
    if (P.R < 1 || P.R > BBM_MAXRP || P.RP != bbm_width(P.R)) return BSLS_E_ARG;
    if (P.m < 1 || P.n < 2 || P.nblocks < 1 || P.nz < 1 || P.nz != P.n - P.nblocks)
        return BSLS_E_ARG;
    if (P.n * P.RP >= ((int64_t)1 << 40) || P.m * P.RP >= ((int64_t)1 << 40)) return BSLS_E_ARG;
    if (!P.a_indptr || !P.a_indices || !P.a_val || !P.at_indptr || !P.at_indices || !P.at_val ||
        P.a_nnz < 0 || P.at_nnz < 0)
        return BSLS_E_ARG;
    if (!P.target || !P.xz || !P.zx || !P.pk_start || !P.pk_mask || !P.pk_len || P.npacks < 1 ||
        P.nlong < 0)
        return BSLS_E_ARG;
    if (!P.z[0] || !P.z[1] || !P.g[0] || !P.g[1] || !P.dz || !P.y || !P.x || !P.w || !P.r ||
        !P.scal || !P.work)
        return BSLS_E_ARG;
    if (P.work_bytes < bbm_layout(nullptr, P.RP).bytes) return BSLS_E_WORKSPACE;
    if (P.nlong > 0 && (!P.long_packs || !P.iso_work ||
                        P.iso_work_bytes < bsls_isotonic_workspace_size(P.RP * P.nz)))
        return BSLS_E_WORKSPACE;
    return BSLS_OK;
}

template <int RP>
void launch_spmm_at(const bsls_bbm_problem &P, hipStream_t st) {
    const int G = bbm_row_lanes(P.at_nnz, P.n, RP);
    bbm_spmm<RP, 0><<<grid_for(P.n, BBM_T / G), BBM_T, 0, st>>>(
        P, P.at_indptr, P.at_indices, P.at_val, P.r, P.w, P.n, G, 0, nullptr, nullptr);
}

template <int RP>
void launch_spmm_a(const bsls_bbm_problem &P, int64_t iter, const BBMWork &w, hipStream_t st) {
    const int G = bbm_row_lanes(P.a_nnz, P.m, RP);
    int grid = grid_for(P.m, BBM_T / G);
    if (grid > BBM_MAXB) grid = BBM_MAXB;
    if (P.roww)
        bbm_spmm<RP, 2><<<grid, BBM_T, 0, st>>>(P, P.a_indptr, P.a_indices, P.a_val, P.x, P.r, P.m,
                                                G, iter, w.p_fin, w.tk_fin);
    else
        bbm_spmm<RP, 1><<<grid, BBM_T, 0, st>>>(P, P.a_indptr, P.a_indices, P.a_val, P.x, P.r, P.m,
                                                G, iter, w.p_fin, w.tk_fin);
}

template <int RP>
void launch_grad(const bsls_bbm_problem &P, int64_t iter, const BBMWork &w, hipStream_t st) {
    int grid = grid_for(P.nz * RP, BBM_T);
    if (grid > BBM_MAXB) grid = BBM_MAXB;
    const int zc = (int)((iter - 1) & 1), zn = (int)(iter & 1);
    if (iter > 0)
        bbm_grad<RP><<<grid, BBM_T, 0, st>>>(P, iter, P.g[zc], P.g[zn], w.p_grad, w.tk_grad);
    else
        bbm_grad<RP><<<grid, BBM_T, 0, st>>>(P, 0, nullptr, P.g[0], w.p_grad, w.tk_grad);
}

template <int RP>
void launch_x(const bsls_bbm_problem &P, int64_t iter, const double *src, hipStream_t st) {
    const int grid = grid_for(P.n * RP, BBM_T);
    if (iter > 0)
        bbm_x<RP, true><<<grid, BBM_T, 0, st>>>(P, P.y, P.z[(iter - 1) & 1], P.z[iter & 1]);
    else
        bbm_x<RP, false><<<grid, BBM_T, 0, st>>>(P, src, nullptr, nullptr);
}

template <int RP>
int stage_rp(const bsls_bbm_problem &P, int stage, int64_t iter, hipStream_t st) {
    const BBMWork w = bbm_layout(P.work, RP);
    const int64_t cnt = P.nz * RP;
    switch (stage) {
        case 0:
            bbm_reset<<<1, BBM_MAXRP * BSLS_S_COUNT, 0, st>>>(P);
            BSLS_LAUNCH_CHECK();
            BSLS_CHECK(hipMemsetAsync(P.work, 0, (size_t)((char *)w.p_fin - (char *)P.work), st));
            return BSLS_OK;
        case 1:
            launch_spmm_a<RP>(P, iter, w, st);
            break;
        case 2:
            launch_spmm_at<RP>(P, st);
            break;
        case 3:
            launch_grad<RP>(P, iter, w, st);
            break;
        case 4:
            if (iter <= 0) return BSLS_E_ARG;
            bbm_step<<<dim3(grid_for(P.nz, BBM_T), (unsigned)RP), BBM_T, 0, st>>>(
                P, P.z[(iter - 1) & 1], P.g[iter & 1]);
            break;
        case 5:
            return bsls_isotonic_packs(P.y, P.pk_start, P.pk_mask, P.pk_len, P.npacks,
                                       P.long_packs, P.nlong, cnt, P.iso_work, P.iso_work_bytes,
                                       st);
        case 6:
            if (iter <= 0) return BSLS_E_ARG;
            launch_x<RP>(P, iter, nullptr, st);
            break;
        case 7:
            bbm_plus_one<<<grid_for(cnt, BBM_T), BBM_T, 0, st>>>(P.z[0], P.z[1], P.dz, cnt);
            BSLS_LAUNCH_CHECK();
            launch_x<RP>(P, 0, P.z[1], st);
            break;
        case 8:
            launch_x<RP>(P, 0, P.z[0], st);
            break;
        default:
            return BSLS_E_ARG;
    }
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}

int stage_any(const bsls_bbm_problem &P, int stage, int64_t iter, hipStream_t st) {
    switch (P.RP) {
        case 1: return stage_rp<1>(P, stage, iter, st);
        case 2: return stage_rp<2>(P, stage, iter, st);
        case 4: return stage_rp<4>(P, stage, iter, st);
        default: return stage_rp<8>(P, stage, iter, st);
    }
}

}  // namespace

extern "C" size_t bsls_bbm_workspace_size(int64_t m, int64_t n, int64_t nz, int64_t R) {
    (void)m;
    (void)n;
    (void)nz;
    if (R < 1 || R > BBM_MAXRP) return 0;
    return bbm_layout(nullptr, bbm_width(R)).bytes;
}

extern "C" int bsls_bbm_stage(const bsls_bbm_problem *p, int stage, int64_t iter, void *stream) {
    const int rc = check_bbm(p);
    if (rc != BSLS_OK) return rc;
    return stage_any(*p, stage, iter, (hipStream_t)stream);
}

extern "C" int bsls_bbm_prologue(const bsls_bbm_problem *p, void *stream) {
    const int rc = check_bbm(p);
    if (rc != BSLS_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    // reset; z[1] = z0 + 1, x = N z[1]; r(z0 + 1); g_prev -> g[0]; x = N z0; r(z0), f(z0)
    static const int steps[] = {0, 7, 1, 2, 3, 8, 1};
    for (int s : steps) {
        const int e = stage_any(*p, s, 0, st);
        if (e != BSLS_OK) return e;
    }
    return BSLS_OK;
}

extern "C" int bsls_bbm_iterate(const bsls_bbm_problem *p, int64_t first_iter, int64_t count,
                                void *stream) {
    const int rc = check_bbm(p);
    if (rc != BSLS_OK) return rc;
    if (first_iter < 1 || count < 0) return BSLS_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    static const int steps[] = {2, 3, 4, 5, 6, 1};
    for (int64_t i = first_iter; i < first_iter + count; ++i)
        for (int s : steps) {
            const int e = stage_any(*p, s, i, st);
            if (e != BSLS_OK) return e;
        }
    return BSLS_OK;
}
