// bb_device.hpp -- device helpers shared by the BB engine's kernels (K1, K2,
// K3 and the tenants): column scales, the phase stamps, write-through stores,
// the stopping rule, the fixed-point r and the fx_sums scale.  Part of
// bb.hip's translation unit.
#pragma once

namespace bsls {

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

// bsls_bb_problem.reg_work: the result word sum_i w_i xh_i^2 on a 64-B line of
// its own, then bb_reg's tickets, then its partials (bb_reg.hpp)
constexpr size_t REG_TICKET_OFF = 64;
constexpr size_t REG_PART_OFF = REG_TICKET_OFF + ((TICKET_BYTES + 63) / 64) * 64;
__device__ __forceinline__ double reg_sum_word(const bsls_bb_problem &P) {
    return *reinterpret_cast<const double *>(P.reg_work);
}

__device__ __forceinline__ void bb_record_f(const bsls_bb_problem &P, int64_t iter, double rr,
                                            bool iterating) {
    double *s = P.scal;
    const double nr = sqrt(rr);
    double fx = 0.5 * (nr * nr);  // 0.5 * la.norm(r)**2, main.py:53
    // bsls_bb_problem.reg_w: + 0.5 sum_i w_i (N z + x0)_i^2, the word the
    // bb_reg launched before this kernel left (CrossValidation.py:141)
    if (P.reg_w) fx += 0.5 * reg_sum_word(P);
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

}  // namespace bsls
