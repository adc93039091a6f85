// bb_k3.hpp -- K3 of the BB engine, t, z = clip01(PAVA(z - t g)), x = N z, and
// the prologue's z + 1 and x = N z.  Part of bb.hip's translation unit (the
// launches: bb_launch.hpp).
#pragma once

namespace bsls {

// x entry i of N z; for a scaled incidence K1 gathers colv[i] * x_i instead,
// the product SciPy's csr_matvec forms for every entry of column i.
__device__ __forceinline__ void x_put(const bsls_bb_problem &P, int64_t i, double v) {
    P.x[i] = P.colv ? colv_at(P, i) * v : v;
}

__device__ __forceinline__ int64_t zend(const bsls_bb_problem &P, int64_t b) {
    return (b + 1 < P.nblocks) ? P.zstarts[b + 1] : P.nz;
}
__device__ __forceinline__ int64_t xend(const bsls_bb_problem &P, int64_t b) {
    return (b + 1 < P.nblocks) ? P.xstarts[b + 1] : P.n;
}

// K3: t, z_new = clip01(PAVA(z - t g)) per block, x = N z_new.  One wave per
// pack of whole z-blocks (<= 64 entries, one lane each): the PAVA passes run
// wave-parallel (pava_wave.hpp, bit-identical to the serial reference); a
// block longer than 64 entries gets a pack of its own and the serial PAVA.
// sc = scal[STOP], scal[SUMDG], scal[DZDG], scal[DGDG], loaded by the caller
// together with its other first loads (one round trip, not three)
__device__ __forceinline__ bool bb_step_t(const bsls_bb_problem &P, int64_t iter,
                                          const double (&sc)[4], double &t) {
    double *s = P.scal;
    if (sc[0] != 0.0) return false;
    if (P.early_exit && sc[1] == 0.0) {  // BB.py:22
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            s[BSLS_S_STOP] = (double)BSLS_STOP_NOCHANGE;
            s[BSLS_S_ITER] = (double)iter;
            s[BSLS_S_ZBUF] = (double)((iter - 1) & 1);
        }
        return false;
    }
    t = sc[2] / sc[3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        s[BSLS_S_T] = t;
        if (fabs(t) <= 1e-10 || fabs(t) > 1e10) s[BSLS_S_WARN] += 1.0;
    }
    return true;
}

#ifndef BSLS_K3_SGPRS
#define BSLS_K3_SGPRS 80
#endif

// Each wave takes K3_PPW packs (w, w + W, ...; W = waves in the grid) and
// issues every load of all of them -- metadata, then z, g and the column
// scales -- before the first PAVA.  MERGE (K3_PPW = 2): the two packs' PAVA
// share the wave after their first passes (pava_v1_wave_pair).
// (at most 80 SGPRs: 256-thread blocks are admitted 8 per CU only up to 80,
// MI355X_MICROARCH.md "Residency"; the merged form otherwise takes 83 and 7)
template <int K3_PPW, bool MERGE, int CV = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(BSLS_K3_SGPRS)))
void bb_k3(bsls_bb_problem P, int64_t iter,
                                             const double *__restrict__ zc,
                                             const double *__restrict__ g,
                                             double *__restrict__ zn,
                                             double *__restrict__ dzo,
                                             int32_t *__restrict__ wsc, int rec,
                                             uint64_t *__restrict__ hd, int kinit,
                                             unsigned long long *rmax_clear = nullptr) {
    PH_DECL;
    PH(0);
    const double sc[4] = {P.scal[BSLS_S_STOP], P.scal[BSLS_S_SUMDG], P.scal[BSLS_S_DZDG],
                          P.scal[BSLS_S_DGDG]};
    // fx_sums: K2, which read max|r|, has finished and the next K1 finish has
    // not begun: the slots back to 0 for it
    if (rmax_clear && blockIdx.x == 0 && threadIdx.x < RMAX_SLOTS) rmax_clear[threadIdx.x] = 0ull;
    // kinit (stage 15): the next K1's r initialisation folded in (its atomic
    // group sums add into r): r = target on the shard_role 1 rank, 0 on the
    // others; once stopped, role 1 keeps its r and the others write 0 -- as
    // bb_k1_init, one launch fewer
    auto init_r = [&](bool stopped) {
        const int64_t gs = (int64_t)gridDim.x * blockDim.x;
        const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (stopped) {
            k1_stopped_rows(P, 0, P.m, t0, gs);
            return;
        }
        const bool add = P.shard_role == 1;
        for (int64_t row = t0; row < P.m; row += gs) {
            const double v = add ? P.target[row] : 0.0;
            P.r[row] = (P.r_fx > 0.0) ? r_fx_of(P, v) : v;
        }
    };
    // rec (stage 13, the sliced sharded schedule): stage 12 folded in -- f and
    // the stopping test of iter - 1 from the all-reduced scal[RR] and the kept
    // scal[PGG] / scal[PDGDG], decided alike by every workgroup (the same
    // inputs), recorded by workgroup 0; on a stop every workgroup returns
    if (rec && !(iter - 1 > 0 && sc[0] != 0.0)) {
        double *s = P.scal;
        const int64_t it = iter - 1;
        const double nr = sqrt(s[BSLS_S_RR]);
        const double fx = 0.5 * (nr * nr);
        const int reason = it > 0 ? bb_stop_reason(P, it, fx, s[BSLS_S_PGG], s[BSLS_S_PDGDG]) : 0;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            s[BSLS_S_FX] = fx;
            if (it > 0) {
                s[BSLS_S_ITER] = (double)it;
                s[BSLS_S_ZBUF] = (double)(it & 1);
            }
            if (reason) {
                s[BSLS_S_STOP] = (double)reason;
                for (int q = 0; q < 4; ++q) s[BSLS_S_SUMDG + q] = s[BSLS_S_PSUMDG + q];
            }
        }
        if (reason) {
            if (kinit) init_r(true);
            return;
        }
    }
    const int l = lane_id();
    const int wv = threadIdx.x / WAVE;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int64_t w0 = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + wv);   // wave-uniform
    __shared__ double pv_y[4][64];
    __shared__ int pv_p[4][128];
    __shared__ int pv_c[4][65];
    int64_t z0[K3_PPW], b0[K3_PPW];
    int L[K3_PPW];
    uint64_t B[K3_PPW], H[K3_PPW];
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q) {
        // unconditional loads at a clamped index (straight-line, one round trip)
        const int64_t pk = w0 + q * nw;
        const int64_t pc = pk < P.npacks ? pk : P.npacks - 1;
        z0[q] = P.pk_z0[pc];
        b0[q] = P.pk_b0[pc];
        L[q] = pk < P.npacks ? P.pk_len[pc] : 0;
        B[q] = (uint64_t)P.pk_mask[pc];
        H[q] = hd ? hd[pc] : 0ull;
    }
    double zv[K3_PPW], gv[K3_PPW], cv[K3_PPW], cv2[K3_PPW];
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q) {
        const bool act = l < L[q] && L[q] <= WAVE;
        const bool bend = (l == L[q] - 1) || (l < 63 && ((B[q] >> (l + 1)) & 1ull));
        const int64_t xi = z0[q] + l + b0[q] + __popcll(B[q] & mask_le(l)) - 1;
        cv[q] = cv2[q] = 1.0;
        if (P.colv) {
            // the column scales of this lane's x entries, loaded before the
            // PAVA so their round trip overlaps it (x_put's products)
            cv[q] = act ? colv_t<CV>(P, xi) : 1.0;
            cv2[q] = (act && bend) ? colv_t<CV>(P, xi + 1) : 1.0;
        }
        zv[q] = act ? zc[z0[q] + l] : 0.0;
        gv[q] = act ? g[z0[q] + l] : 0.0;
    }
    double t;
    const bool go = bb_step_t(P, iter, sc, t);
    if (kinit) init_r(!go);
    if (!go) return;
    PH(1);
    double yv[K3_PPW];
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q)   // x_next = x - t g (BB.py:29)
        yv[q] = (l < L[q] && L[q] <= WAVE) ? zv[q] - t * gv[q] : 0.0;
#ifdef BSLS_PHASE_STAMPS
    // (the stamp after z and g have landed: it waits for them through yv)
    asm volatile("" ::"v"(yv[0]));
    PH(2);
#endif
    if (BSLS_K3_KO != 1) {
        // warm start: the last run partition of each pack, tested first; a
        // pack that passes needs no reference pass, and a partition that
        // fails is repaired -- its unsplittable runs kept pooled -- and the
        // reference passes continue from it (pava_warm_repair)
        bool need[K3_PPW], store[K3_PPW];
        uint64_t Hn[K3_PPW];
#pragma unroll
        for (int q = 0; q < K3_PPW; ++q) {
            need[q] = L[q] > 0 && L[q] <= WAVE;
            store[q] = need[q];
            if (hd && need[q] && (H[q] & B[q]) == B[q] && (H[q] & ~mask_lt(L[q])) == 0ull) {
                store[q] = pava_warm_repair(yv[q], L[q], B[q], H[q], pv_y[wv], pv_p[wv],
                                            pv_c[wv], &Hn[q]);
                need[q] = false;
            }
        }
        if (MERGE && K3_PPW == 2 && need[0] && need[K3_PPW - 1]) {
            pava_v1_wave_pair(yv[0], L[0], B[0], yv[K3_PPW - 1], L[K3_PPW - 1], B[K3_PPW - 1],
                              pv_y[wv], pv_p[wv], pv_c[wv], &Hn[0], &Hn[K3_PPW - 1]);
        } else {
#pragma unroll
            for (int q = 0; q < K3_PPW; ++q)
                if (need[q])
                    pava_v1_wave_c(yv[q], L[q], B[q], pv_y[wv], pv_p[wv], pv_c[wv], &Hn[q]);
        }
        if (hd) {
#pragma unroll
            for (int q = 0; q < K3_PPW; ++q)   // the new partition for the next call
                if (store[q] && l == 0) hd[w0 + q * nw] = Hn[q];
        }
    }
    PH(3);
#pragma unroll
    for (int q = 0; q < K3_PPW; ++q) {
        if (L[q] == 0) break;
        if (L[q] <= WAVE) {
            const bool act = l < L[q];
            const bool bstart = (B[q] >> l) & 1ull;
            const int bl = __popcll(B[q] & mask_le(l)) - 1;   // block within the pack
            const bool bend = (l == L[q] - 1) || (l < 63 && ((B[q] >> (l + 1)) & 1ull));
            const double v = clip01(yv[q]);
            const double vprev = shfl_d(v, l > 0 ? l - 1 : 0);
            const int nb = __popcll(B[q]);
            const __amdgpu_buffer_rsrc_t rz =
                __builtin_amdgcn_make_buffer_rsrc(zn + z0[q], 0, L[q] * 8, 0x00020000);
            const __amdgpu_buffer_rsrc_t rd =
                __builtin_amdgcn_make_buffer_rsrc(dzo + z0[q], 0, L[q] * 8, 0x00020000);
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(
                P.x + z0[q] + b0[q], 0, (L[q] + nb) * 8, 0x00020000);
            if (act) {
                wt_store_f64(rz, l * 8, v);
                wt_store_f64(rd, l * 8, v - zv[q]);   // next K2's z - z_prev
                const double d = v - (bstart ? 0.0 : vprev);
                const int xo = (l + bl) * 8;
                wt_store_f64(rx, xo, P.colv ? cv[q] * d : d);
                if (bend) wt_store_f64(rx, xo + 8, P.colv ? cv2[q] * (0.0 - v) : (0.0 - v));
            }
        } else if (!P.long_packs && l == 0) {
            // one block longer than a wave: serial PAVA in global memory
            // (with P.long_packs bb_k3_long takes it, a workgroup per block)
            const int64_t xs = P.xstarts[b0[q]];
            for (int64_t j = z0[q]; j < z0[q] + L[q]; ++j) {
                zn[j] = zc[j] - t * g[j];
                wsc[j] = 1;
            }
            pava_v1(zn, wsc, z0[q], z0[q] + L[q], 1);
            double prev = 0.0;
            int64_t xo = xs;
            for (int64_t j = z0[q]; j < z0[q] + L[q]; ++j) {
                const double v = clip01(zn[j]);
                zn[j] = v;
                dzo[j] = v - zc[j];
                x_put(P, xo++, v - prev);
                prev = v;
            }
            x_put(P, xo, 0.0 - prev);
        }
    }
    PH(4);
    PH_FLUSH(PH_K3);
}

// K3 for one z-block longer than a wave, one 1024-thread workgroup per block
// (after bb_k3 in the same stream): z - t g, PAVA v1 by the whole workgroup
// (pava_long.hpp, bit-identical), clip, dz and x as bb_k3's serial path.
// t as bb_step_t, without its writes (bb_k3 made them).
__global__ __launch_bounds__(LONG_T) void bb_k3_long(bsls_bb_problem P, int64_t iter,
                                                     const double *__restrict__ zc,
                                                     const double *__restrict__ g,
                                                     double *__restrict__ zn,
                                                     double *__restrict__ dzo) {
    __shared__ int64_t sh[LONG_T / 64 + 1];
    __shared__ int flag;
    const double *s = P.scal;
    if (s[BSLS_S_STOP] != 0.0) return;
    if (P.early_exit && s[BSLS_S_SUMDG] == 0.0) return;
    const double t = s[BSLS_S_DZDG] / s[BSLS_S_DGDG];
    const int64_t q = P.long_packs[blockIdx.x];
    const int64_t z0 = P.pk_z0[q], b0 = P.pk_b0[q], L = P.pk_len[q];
    const int64_t off = P.long_off[blockIdx.x], tot = P.long_off[P.nlong];
    double *Y0 = (double *)P.long_scratch + off;
    double *Y1 = (double *)P.long_scratch + tot + off;
    int32_t *W = (int32_t *)((double *)P.long_scratch + 2 * tot);
    int32_t *W0 = W + off, *W1 = W + tot + off, *CH = W + 2 * tot + blockIdx.x + off;
    for (int64_t j = threadIdx.x; j < L; j += LONG_T) zn[z0 + j] = zc[z0 + j] - t * g[z0 + j];
    __syncthreads();
    pava_v1_long(zn + z0, L, Y0, Y1, W0, W1, CH, sh, &flag);
    for (int64_t j = threadIdx.x; j < L; j += LONG_T) {
        const double v = clip01(zn[z0 + j]);
        zn[z0 + j] = v;
        dzo[z0 + j] = v - zc[z0 + j];
    }
    __syncthreads();
    const int64_t xs = P.xstarts[b0];
    for (int64_t j = threadIdx.x; j <= L; j += LONG_T) {
        const double v = (j < L) ? zn[z0 + j] : 0.0;
        const double prev = (j > 0) ? zn[z0 + j - 1] : 0.0;
        x_put(P, xs + j, v - prev);
    }
}

// Prologue helpers (BB.py:14-15: x_prev = x + 1); bb_z2x writes N z.
__global__ __launch_bounds__(256) void bb_plus_one(const double *__restrict__ a,
                                                   double *__restrict__ o,
                                                   double *__restrict__ dz, int64_t nz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nz) {
        const double v = a[i], w = v + 1;
        o[i] = w;
        dz[i] = v - w;   // iteration 1's z - z_prev
    }
}

// one thread per x entry (coalesced; C5 418 -> ~20 us against a thread per
// block): xz[i] is entry i's z index, -1 for a block's last entry (blocks
// have >= 2 routes); the same differences K3 forms (v - prev, prev = 0.0 at a
// block's first entry, 0.0 - z_last at its last)
__global__ __launch_bounds__(256) void bb_z2x(bsls_bb_problem P, const double *__restrict__ z) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n) return;
    const int32_t j = P.xz[i];
    const int32_t jp = (i > 0) ? P.xz[i - 1] : -1;
    double v;
    if (j >= 0) v = z[j] - (jp >= 0 ? z[jp] : 0.0);
    else v = 0.0 - z[jp];
    x_put(P, i, v);
}

}  // namespace bsls
