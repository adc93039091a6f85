// bbm.hpp -- the batched BB engine's workspace layout and per-column helpers
// (csrc/bbm.hip; struct bsls_bbm_problem in include/bsls_hip.h).
#pragma once
#include "bsls_common.hpp"

namespace bsls {

// The reducing launches (the A-side SpMM's finish, bbm_grad) run at most
// BBM_MAXB workgroups, each looping over its share: the second stage of a sum
// then reads a bounded number of partials, in index order.
constexpr int BBM_MAXB = 2048;
constexpr int BBM_T = 256;            // threads per workgroup, every kernel here
constexpr int BBM_MAXRP = 8;

struct BBMWork {
    unsigned *tk_fin;                 // TICKET_BYTES each
    unsigned *tk_grad;
    double *p_fin;                    // BBM_MAXB x (2 RP): rr, held per column
    double *p_grad;                   // BBM_MAXB x (4 RP): the four BB sums per column
    size_t bytes;
};

inline BBMWork bbm_layout(void *base, int64_t RP) {
    BBMWork w;
    char *p = (char *)base;
    const size_t tk = ((size_t)TICKET_BYTES + 63) & ~(size_t)63;
    w.tk_fin = (unsigned *)p;
    w.tk_grad = (unsigned *)(p + tk);
    w.p_fin = (double *)(p + 2 * tk);
    w.p_grad = w.p_fin + (size_t)BBM_MAXB * 2 * RP;
    w.bytes = 2 * tk + (size_t)BBM_MAXB * 6 * RP * sizeof(double);
    return w;
}

inline int bbm_width(int64_t R) { return R <= 1 ? 1 : R <= 2 ? 2 : R <= 4 ? 4 : 8; }

// Lanes per row of an SpMM launch: a power of two, a multiple of RP, at most a
// wave -- the smallest whose RP-wide entry slots (G / RP of them) cover the
// mean row in one pass, so short rows (A': the routes' 16 links) share a wave
// and long ones (A: ~160 routes per link) take a whole one.
inline int bbm_row_lanes(int64_t nnz, int64_t rows, int RP) {
    const double mean = rows > 0 ? (double)nnz / (double)rows : 1.0;
    int G = RP;
    while (G < WAVE && (double)(G / RP) < mean) G *= 2;
    return G;
}

// a thread's NS values of column j spread over the NS * RP slots of a block
// sum (zeros elsewhere: x + 0.0 is exact, so each column's sum is the sum of
// its own terms in the tree's fixed order)
template <int RP, int NS>
__device__ __forceinline__ void bbm_spread(const double (&mine)[NS], int j, double (&v)[NS * RP]) {
#pragma unroll
    for (int c = 0; c < RP; ++c)
#pragma unroll
        for (int s = 0; s < NS; ++s) v[c * NS + s] = (c == j) ? mine[s] : 0.0;
}

}  // namespace bsls
