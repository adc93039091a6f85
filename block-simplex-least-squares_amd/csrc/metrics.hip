// metrics.hip -- the link metrics of a fit by set (train / held out) and flow
// class: CrossValidation.post_process's metrics() (python/CrossValidation.py:
// 193-214, 246-274) as one table of sums per state (include/bsls_hip.h).
//
// Two launches, no hand-off between workgroups inside a kernel:
//   link_metrics_part  <<<(row chunks, nstates)>>>  one cells x 9 table per
//                      workgroup into `work`;
//   link_metrics_sum   <<<nstates>>>  adds the workgroups' tables in index
//                      order into `out`.
// Stream order between the two gives the visibility.
#include "bsls_common.hpp"

namespace bsls {

constexpr int LM_ROWS = 512;                            // rows (one per thread) of a workgroup
constexpr int LM_SEG = 32;                              // rows one scanning thread adds, in row order
constexpr int LM_NSEG = LM_ROWS / LM_SEG;
constexpr int LM_CELLS = 2 * (BSLS_LM_MAX_EDGES + 1);   // sets x classes, at most
constexpr int LM_SUM_THREADS = 1024;
constexpr int LM_SUM_RANGES = 8;                        // ranges of workgroup tables, at most

static_assert(LM_CELLS == 32 && LM_ROWS == LM_NSEG * LM_CELLS,
              "the scan gives thread t cell t % 32 of segment t / 32");
static_assert(LM_SUM_THREADS / (LM_CELLS * BSLS_LM_NV) >= 1, "one range at least");

__device__ __forceinline__ bool lm_is_max(int k) { return k == BSLS_LM_MAX_GEH; }

// Each thread takes one row: its cell (set * classes + class) and d2, geh, b
// go to LDS.  Then thread (cell c, segment g) adds the rows of its segment
// that fell into c, in row order -- a row is selected into its cell, never
// multiplied into another -- and the 16 segments of a cell are added in order.
__global__ __launch_bounds__(LM_ROWS) void link_metrics_part(
    const double *__restrict__ ax, int64_t ax_ld, const double *__restrict__ b,
    const double *__restrict__ roww, int64_t roww_ld, const double *__restrict__ edges,
    int nedges, int64_t m, double *__restrict__ part) {
    __shared__ double s_edges[BSLS_LM_MAX_EDGES + 1];
    __shared__ int s_cell[LM_ROWS];
    __shared__ double s_d2[LM_ROWS], s_geh[LM_ROWS], s_b[LM_ROWS];
    __shared__ double s_tab[LM_NSEG * LM_CELLS * BSLS_LM_NV];
    const int t = threadIdx.x;
    const int ncls = nedges + 1, ncells = 2 * ncls;
    if (t < nedges) s_edges[t] = edges[t];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * LM_ROWS + t;
    const int64_t s = blockIdx.y;
    int cell = -1;
    double d2 = 0.0, geh = 0.0, bi = 0.0;
    if (i < m) {
        const double a = ax[s * ax_ld + i];
        bi = b[i];
        int set = 0;
        if (roww) set = (roww[s * roww_ld + i] != 0.0) ? 0 : 1;
        int cls = 0;
        for (int e = 0; e < nedges; ++e) cls += (s_edges[e] <= bi) ? 1 : 0;
        const double diff = a - bi, plus = a + bi;
        d2 = diff * diff;
        geh = sqrt((2.0 * d2) / plus);
        cell = set * ncls + cls;
    }
    s_cell[t] = cell;
    s_d2[t] = d2;
    s_geh[t] = geh;
    s_b[t] = bi;
    __syncthreads();
    const int c = t % LM_CELLS, seg = t / LM_CELLS;
    double v[BSLS_LM_NV];
#pragma unroll
    for (int k = 0; k < BSLS_LM_NV; ++k) v[k] = 0.0;
    if (c < ncells) {
        for (int j = 0; j < LM_SEG; ++j) {
            const int r = seg * LM_SEG + j;
            if (s_cell[r] != c) continue;
            const double g = s_geh[r];
            v[BSLS_LM_COUNT] += 1.0;
            v[BSLS_LM_SSQ] += s_d2[r];
            v[BSLS_LM_SUM_GEH] += g;
            v[BSLS_LM_MAX_GEH] = nan_max(v[BSLS_LM_MAX_GEH], g);
            v[BSLS_LM_UNDER_5] += (g < 5.0) ? 1.0 : 0.0;
            v[BSLS_LM_UNDER_1] += (g < 1.0) ? 1.0 : 0.0;
            v[BSLS_LM_UNDER_0_5] += (g < 0.5) ? 1.0 : 0.0;
            v[BSLS_LM_UNDER_0_05] += (g < 0.05) ? 1.0 : 0.0;
            v[BSLS_LM_SUM_B] += s_b[r];
        }
    }
#pragma unroll
    for (int k = 0; k < BSLS_LM_NV; ++k) s_tab[(seg * LM_CELLS + c) * BSLS_LM_NV + k] = v[k];
    __syncthreads();
    double *dst = part + ((size_t)s * gridDim.x + blockIdx.x) * (size_t)(ncells * BSLS_LM_NV);
    for (int u = t; u < ncells * BSLS_LM_NV; u += LM_ROWS) {
        const int cc = u / BSLS_LM_NV, k = u % BSLS_LM_NV;
        double acc = s_tab[cc * BSLS_LM_NV + k];
        for (int g = 1; g < LM_NSEG; ++g) {
            const double x = s_tab[(g * LM_CELLS + cc) * BSLS_LM_NV + k];
            acc = lm_is_max(k) ? nan_max(acc, x) : acc + x;
        }
        dst[u] = acc;
    }
}

// One workgroup per state: the nchunks tables in Q = min(8, 1024 / values)
// contiguous ranges, each added in index order by one thread per value, then
// the ranges in order.  Q and the ranges depend on nedges and m only.
__global__ __launch_bounds__(LM_SUM_THREADS) void link_metrics_sum(
    const double *__restrict__ part, int64_t nchunks, int nvals, double *__restrict__ out) {
    __shared__ double red[LM_SUM_RANGES * LM_CELLS * BSLS_LM_NV];
    const int t = threadIdx.x;
    int Q = LM_SUM_THREADS / nvals;
    Q = Q > LM_SUM_RANGES ? LM_SUM_RANGES : Q;
    const int64_t per = (nchunks + Q - 1) / Q;
    const double *src = part + (size_t)blockIdx.x * (size_t)nchunks * nvals;
    if (t < Q * nvals) {
        const int q = t / nvals, u = t % nvals;
        const bool is_max = lm_is_max(u % BSLS_LM_NV);
        const int64_t lo = q * per, hi = (lo + per < nchunks) ? lo + per : nchunks;
        double acc = 0.0;
        for (int64_t ch = lo; ch < hi; ++ch) {
            const double x = src[(size_t)ch * nvals + u];
            acc = is_max ? nan_max(acc, x) : acc + x;
        }
        red[q * nvals + u] = acc;
    }
    __syncthreads();
    if (t < nvals) {
        const bool is_max = lm_is_max(t % BSLS_LM_NV);
        double acc = red[t];
        for (int q = 1; q < Q; ++q) {
            const double x = red[q * nvals + t];
            acc = is_max ? nan_max(acc, x) : acc + x;
        }
        out[(size_t)blockIdx.x * nvals + t] = acc;
    }
}

static bool lm_sizes_ok(int64_t m, int nstates, int nedges) {
    // (row chunks are a grid's x extent)
    return m >= 1 && m <= (int64_t)LM_ROWS * 0x7fffffff && nstates >= 1 && nstates <= 1024 &&
           nedges >= 0 && nedges <= BSLS_LM_MAX_EDGES;
}

}  // namespace bsls

using namespace bsls;

extern "C" size_t bsls_link_metrics_work_size(int64_t m, int nstates, int nedges) {
    if (!lm_sizes_ok(m, nstates, nedges)) return 0;
    const size_t nchunks = (size_t)((m + LM_ROWS - 1) / LM_ROWS);
    return nchunks * (size_t)nstates * (size_t)(2 * (nedges + 1) * BSLS_LM_NV) * sizeof(double);
}

extern "C" int bsls_link_metrics(const double *ax, int64_t ax_ld, const double *b,
                                 const double *roww, int64_t roww_ld, const double *edges,
                                 int nedges, int64_t m, int nstates, double *out, void *work,
                                 void *stream) {
    if (!lm_sizes_ok(m, nstates, nedges) || !ax || !b || !out || !work) return BSLS_E_ARG;
    if (ax_ld < m || (roww && roww_ld != 0 && roww_ld < m) || (nedges > 0 && !edges))
        return BSLS_E_ARG;
    const int64_t nchunks = (m + LM_ROWS - 1) / LM_ROWS;
    const int nvals = 2 * (nedges + 1) * BSLS_LM_NV;
    link_metrics_part<<<dim3((unsigned)nchunks, (unsigned)nstates), LM_ROWS, 0,
                        (hipStream_t)stream>>>(ax, ax_ld, b, roww, roww ? roww_ld : 0, edges,
                                               nedges, m, (double *)work);
    BSLS_LAUNCH_CHECK();
    link_metrics_sum<<<nstates, LM_SUM_THREADS, 0, (hipStream_t)stream>>>(
        (const double *)work, nchunks, nvals, out);
    BSLS_LAUNCH_CHECK();
    return BSLS_OK;
}
