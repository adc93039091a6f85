// bb_reg.hpp -- the weighted L2 regulariser of the BB engine
// (bsls_bb_problem.reg_w; python/CrossValidation.py:140-148, ISTTT.py:88-92):
// one streaming kernel that leaves N'(w o (N z + x0)) for the next K2 and
// sum_i w_i (N z + x0)_i^2 for the next K1 finish.  Part of bb.hip's
// translation unit.
#pragma once

namespace bsls {

// x entry i of xh = N z + x0 and q_i = w_i xh_i.  The differences are bb_z2x's
// (SciPy's csr_matvec over N's row: a -1 and a +1 in column order), x0 is 1 at
// a block's last entry (j < 0) and 0 elsewhere.
__device__ __forceinline__ double reg_q(const bsls_bb_problem &P, const double *__restrict__ z,
                                        int64_t i, int32_t &j, double &xh) {
    j = P.xz[i];
    const int32_t jp = (i > 0) ? P.xz[i - 1] : -1;
    const double w = P.reg_w[i];
    const double zp = (jp >= 0) ? z[jp] : 0.0;
    if (j >= 0) xh = z[j] - zp;
    else xh = (0.0 - zp) + 1.0;
    return w * xh;
}

// One thread per x entry, 256 to a workgroup (xz and reg_w coalesced; the z
// gathers are two adjacent entries).  q_{i+1} comes through LDS; the entry
// after the workgroup's last is its one halo, formed by thread 0.  The sum:
// block sums (a fixed tree), then the last-arriving workgroup adds the slots
// in index order and re-zeroes the tickets for the next launch -- no atomics
// on doubles, the same bits every run.  A stopped run (as K2, K3 and K1)
// returns before it writes anything.
__global__ __launch_bounds__(256) void bb_reg(bsls_bb_problem P, const double *__restrict__ z,
                                              int64_t iter) {
    __shared__ double sq[256 + 1];
    __shared__ double red[256 / WAVE];
    if (iter > 0 && P.scal[BSLS_S_STOP] != 0.0) return;
    const int64_t base = (int64_t)blockIdx.x * 256;
    const int64_t i = base + threadIdx.x;
    int32_t j = -1;
    double xh = 0.0, q = 0.0;
    if (i < P.n) q = reg_q(P, z, i, j, xh);
    sq[threadIdx.x] = q;
    if (threadIdx.x == 0) {
        int32_t jh;
        double xhh;
        sq[256] = (base + 256 < P.n) ? reg_q(P, z, base + 256, jh, xhh) : 0.0;
    }
    __syncthreads();
    // (j >= 0: not a block's last entry, so entry i + 1 exists; 0.0 + q: the
    // row sum of N' starts from +0.0, so a q_i of -0.0 -- w_i = 0 under a
    // negative xh_i -- leaves SciPy's +0.0)
    if (j >= 0) P.reg_g[j] = (0.0 + q) - sq[threadIdx.x + 1];
    double s[1] = {q * xh};
    block_sum<1>(s, red);
    char *wk = reinterpret_cast<char *>(P.reg_work);
    double tot[1];
    if (last_block_sum<1>(s, reinterpret_cast<double *>(wk + REG_PART_OFF),
                          reinterpret_cast<unsigned *>(wk + REG_TICKET_OFF), tot, red) &&
        threadIdx.x == 0)
        *reinterpret_cast<double *>(wk) = tot[0];
}

static size_t reg_work_bytes(int64_t n) {
    return REG_PART_OFF + (size_t)(grid_for(n, 256) + 1) * 8;
}

static void launch_bb_reg(const bsls_bb_problem &P, const double *z, int64_t iter,
                          hipStream_t st) {
    bb_reg<<<grid_for(P.n, 256), 256, 0, st>>>(P, z, iter);
}

}  // namespace bsls
