// pava_fast.hpp -- wave-parallel PAVA v1 from one prefix sum: the unique
// isotonic fit (isotonic_regression.h:13-58) under the north star's 1e-12
// contract, not the reference's pooling order and roundings.
//
// Same contract as pava_v1_wave_c (pava_wave.hpp): one pack of whole blocks,
// at most 64 elements, one per lane; block starts in the wave-uniform mask B;
// the expanded fit returned in y.  The isotonic fit is unique and pooling
// adjacent violators in any order reaches it, so the run structure is nothing
// but the wave-uniform head mask H (the run of head h is [h, next head)), and
// the arithmetic is ONE block-segmented prefix sum (DPP row_shr / row_bcast,
// as warm_test), kept in this wave's LDS slice as
//   pi[l] = y_b + ... + y_l      (b = the start of l's block)
//   pe[l] = y_b + ... + y_(l-1)  (0 at a block start).
// A pass: every head h finds its run's last lane e and the previous head p
// with mask searches, takes S_h = pi[e] - pe[h] and S_p = pe[h] - pe[p], and
// violates iff S_h len_p < S_p len_h (its run's mean is below the previous
// run's); the ballot of violating heads that are not block starts leaves H.
// A chain of descending runs pools in one pass, as in the reference.  A pass
// writes no LDS, compacts nothing, keeps no weights and needs no barrier.
//
// A run of length 1 is its element, never a prefix difference (S = y, read
// from the register / one DPP shift): neighbours compare on their raw values,
// so an input that is non-decreasing within every block comes back bit for
// bit (ties, -0.0), and a lane whose final run has length 1 returns its input.
//
// When a pass removes nothing every lane divides once, m = S / len, and the
// heads compare the divided means themselves (m_h < m_prev: pool again), so
// the output is non-decreasing within every block exactly -- the
// cross-multiplied test alone could leave an inversion of an ulp.
//
// The loop is counted: at most 64 iterations, each continuing one strictly
// shrinks H.  Non-finite input cannot keep a wave running (NaN compares are
// false: no head leaves, the loop exits).  No atomics: deterministic.
//
// Accuracy (the header's comment, include/bsls_hip.h, words the two tiers).
#pragma once
#include "pava_wave.hpp"

// BSLS_ISO_FAST_KO (timing knock-outs, never in the product build): 1 = the
// scan, the division and the expansion with no pooling pass, 2 = one pass.
#ifndef BSLS_ISO_FAST_KO
#define BSLS_ISO_FAST_KO 0
#endif

namespace bsls {

// y: this lane's element (lanes < L, 1 <= L <= 64); B: block starts (bit 0 is
// taken as set); pi / pe: this wave's 64 + 64 doubles of LDS.  On return y =
// the expanded fit.  Runs with all lanes active (DPP reads).
__device__ __forceinline__ void pava_fast_wave(double &y, int L, uint64_t B, double *pi,
                                               double *pe) {
    const int l = lane_id();
    const bool act = l < L;
    B |= 1ull;
    const uint64_t mle = mask_le(l), mlt = mask_lt(l);
    const int b = hi_bit(B & mle);                           // this lane's block start
    // block-segmented inclusive scan: s = y_b + ... + y_l
    double s = act ? y : 0.0;
    double u;
    u = dpp_mov_d<0x111, 0xF>(s);                            // row_shr:1
    s += (l - 1 >= b) ? u : 0.0;
    u = dpp_mov_d<0x112, 0xF>(s);                            // row_shr:2
    s += (l - 2 >= b) ? u : 0.0;
    u = dpp_mov_d<0x114, 0xF>(s);                            // row_shr:4
    s += (l - 4 >= b) ? u : 0.0;
    u = dpp_mov_d<0x118, 0xF>(s);                            // row_shr:8
    s += (l - 8 >= b) ? u : 0.0;
    u = dpp_mov_d<0x142, 0xA>(s);                            // row_bcast:15 -> rows 1, 3
    s += ((l & 16) != 0 && b <= (l & ~15) - 1) ? u : 0.0;
    u = dpp_mov_d<0x143, 0xC>(s);                            // row_bcast:31 -> rows 2, 3
    s += (l >= 32 && b <= 31) ? u : 0.0;
    const double yprev = dpp_shr1_d(y);                      // lane 0: unused (a block start)
    const double sprev = dpp_shr1_d(s);
    const double el = (l == b) ? 0.0 : sprev;
    pi[l] = s;
    pe[l] = el;
    uint64_t H = mask_lt(L);
    double m = y;
    for (int pass = 0; pass < WAVE; ++pass) {
        // this lane as a head: its run [l, e], the previous head p
        const uint64_t above = H & ~mle;
        const int e = above ? lo_bit(above) - 1 : L - 1;
        uint64_t V = 0ull;
        if (!(BSLS_ISO_FAST_KO == 1 || (BSLS_ISO_FAST_KO == 2 && pass > 0))) {
            const uint64_t below = H & mlt;
            const int p = below ? hi_bit(below) : 0;
            const int lr = e - l + 1, lp = l - p;
            // (the reads stay under the length-1 tests, a divergent branch
            // each: both issued ahead of the selects measured 0.1 us slower
            // on C3, profiles/iso_fast_C3.txt)
            const double sr = (lr == 1) ? y : pi[e] - el;
            const double sp = (lp == 1) ? yprev : el - pe[p];
            V = ballot_b(sr * (double)lp < sp * (double)lr) & H & ~B;
        }
        if (!V) {
            // nothing pools: every lane takes its run's mean, and the heads
            // compare the divided means
            const int h = hi_bit(H & mle);                   // bit 0 never leaves H
            const int len = e - h + 1;
            const double sm = (len == 1) ? y : pi[e] - pe[h];
            m = sm / (double)len;
            const double mp = dpp_shr1_d(m);                 // the previous run's, at a head
            V = ballot_b(m < mp) & H & ~B;
            if (!V || BSLS_ISO_FAST_KO != 0) break;
        }
        H &= ~V;
    }
    if (act) y = m;
}

}  // namespace bsls
