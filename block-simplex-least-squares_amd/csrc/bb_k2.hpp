// bb_k2.hpp -- K2 of the BB engine, g = N'(A' r) with dg and the BB sums: the
// tile kernel, the panel kernel and the sliced schedule's stage 12.  Part of
// bb.hip's translation unit (the launches: bb_launch.hpp).
#pragma once

namespace bsls {

// K2's epilogue rows per thread per batch (K2E; round 6: 4 -- C3's 3.8 rows
// per thread fit one batch, C5's 19 run five at the speed of three of 8, and
// the kernel drops from 124 to 86 VGPRs: C3 13.2k -> 13.4k it/s, C5 and the
// 8-way C5 rank the same, tools/gpu_r06k.sh; A/B builds: BSLS_K2E.  Loading
// the first batch's z indices and scales before the walk instead, to land
// under it, measured no gain: 13.2k)
#ifndef BSLS_K2E
#define BSLS_K2E 4
#endif

// K2 on a tile image: w = A'r for row block rb (+ its halo row) in LDS, summed
// over r's column groups (one group: in CSR order, bit-identical to SciPy;
// several: partials in wpart, summed in group order by the block's last
// workgroup); then g = N'w, dg and the four BB sums, as bb_k2.  MODE 1: stored
// values; MODE 2: scaled incidence, each term colv[row] * r_i (SciPy's
// product; the rows' scales sit in LDS beside the sums); MODE 3: scaled
// incidence with several groups (no bit pattern to keep): w_i = colv_i *
// sum r, one product per row after the group sums, and the whole LDS for rows.
// FUSE (stage 8, column-sharded): every workgroup first sums r_i^2 over its
// slice of r (already the all-reduced residual; slice blockIdx of nrb * G, so
// the linear read also warms the caches the walk gathers r from), the
// finishing workgroup of row block rb adds its groups' slices in group order
// (through wpart's tail, see bsls_bb_problem.wpart), and the last one records
// f and runs the stopping test of iteration iter - 1 before it stores this
// iteration's sums.  (At the end of the finishing workgroups only, the slice
// sums cost 13 us of tail in the 8-way rehearsal.)
// FUSE 2 (stage 10, the sliced schedule): the same r^2, but over this rank's
// rows [P.rr_lo, P.rr_hi) of r only (1/world of m: the other ranks sum the
// rest), stored with the sums as scal[RR] for the all-reduce; the last
// workgroup keeps iteration iter - 1's sums in scal[PSUMDG..PGG] for the
// stop test that follows the all-reduce (stage 12), instead of testing.
// K2 of a stopped sharded run: the driver still all-reduces scal[SUMDG..RR]
// after every K2 it enqueues, so the shard_role 2 ranks zero their copy and
// the sum leaves role 1's -- the stop iteration's sums -- instead of world
// times them, growing with every iteration enqueued past the stop
// (fuse 2 all-reduces scal[RR] with the four sums)
template <int FUSE>
__device__ __forceinline__ void k2_stopped_sums(const bsls_bb_problem &P) {
    if (P.shard_role == 2 && blockIdx.x == 0 && threadIdx.x == 0)
        for (int q = 0; q < (FUSE == 2 ? 5 : 4); ++q) P.scal[BSLS_S_SUMDG + q] = 0.0;
}

// K2's last workgroup, one thread: the reduced sums tot into scal (bb_k2t and
// bb_k2).  FUSE 1 first records f and runs the stopping test of iteration
// iter - 1 on tot[4] = ||r||^2; FUSE 2 keeps iteration iter - 1's sums in
// scal[PSUMDG..PGG] and stores tot[4] as scal[RR].
template <int FUSE>
__device__ __forceinline__ void k2_store_sums(const bsls_bb_problem &P, int64_t iter,
                                              const double (&tot)[FUSE ? 5 : 4]) {
    if constexpr (FUSE == 1) {
        bb_record_f(P, iter - 1, tot[4], iter - 1 > 0);
        // stopped at iter - 1: keep that iteration's sums (what the
        // unfused schedule leaves in scal); g[iter & 1], written by this
        // launch, is the other buffer -- the stopping iterate's g is untouched
        if (P.scal[BSLS_S_STOP] != 0.0) {
            // (the sums all-reduced after this launch: as k2_stopped_sums)
            if (P.shard_role == 2)
                for (int q = 0; q < 4; ++q) P.scal[BSLS_S_SUMDG + q] = 0.0;
            return;
        }
    }
    if constexpr (FUSE == 2) {
        double *sc = P.scal;
        for (int q = 0; q < 4; ++q) sc[BSLS_S_PSUMDG + q] = sc[BSLS_S_SUMDG + q];
        sc[BSLS_S_RR] = tot[4];
    }
    P.scal[BSLS_S_SUMDG] = tot[0];
    P.scal[BSLS_S_DZDG] = tot[1];
    P.scal[BSLS_S_DGDG] = tot[2];
    P.scal[BSLS_S_GG] = tot[3];
}

// gsel >= 0 (bsls_bb_k2_part): only column group gsel, one workgroup per row
// block -- the link-part pipeline of the sharded schedule launches the groups
// one by one, each as soon as its rows of r are all-reduced.  The launches
// are ordered on one stream, so the roles are fixed: groups < G - 1 leave
// their partial row sums (and r^2 slices) in wpart and return; the last group
// adds them in group order and runs the epilogue -- no tickets.  Its slice of
// ||r||^2 stays inside its own link range (rows of r the earlier parts'
// exchanges have not finished may not be read).
// FX (bsls_bb_problem.fx_sums: gsel < 0, FUSE 0, MODE 1 / 3, dealt images):
// the walk's row sums in two integer words (tiles.hpp fx_add: order-free),
// scaled from fx_a2 * max|r| (rmax: the slots K1's finish keeps); after the
// walk the rows -- the halo row too -- are converted in place to doubles (one
// group of a scaled incidence: to w_i = colv_i * sum, the epilogue's product),
// and the group hand-off and the N' epilogue run as in the float form.
// REG (bsls_bb_problem.reg_w: FUSE 0, !FX, gsel < 0): the epilogue loads
// reg_g[j] with g_prev[j] and dz[j] and forms g = (w_i - w_{i+1}) + reg_g[j],
// the reference's order (CrossValidation.py:142-144), before the store of g
// and the four sums.
template <int MODE, bool ITER, int FUSE = 0, int CV = 0, bool FX = false, bool REG = false>
__global__ __launch_bounds__(1024) void bb_k2t(bsls_bb_problem P, const double *__restrict__ dzv,
                                               const double *__restrict__ gp,
                                               double *__restrict__ gout, double *part,
                                               unsigned *ticket, unsigned *tk2rb, int64_t iter,
                                               int gsel, const unsigned long long *rmax = nullptr) {
    static_assert(!FX || (FUSE == 0 && (MODE == 1 || MODE == 3)), "FX: the single-GCD dealt K2");
    static_assert(!REG || (FUSE == 0 && !FX), "REG: the single-GCD float K2");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double red[5 * 16];
    __shared__ int row_last;
    PH_DECL;
    PH(0);
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        if (gsel < 0 || gsel == P.ATt.ngroups - 1) k2_stopped_sums<FUSE>(P);
        return;
    }
    PH(1);
    const bsls_tiles &T = P.ATt;
    int64_t rb, g;
    if (gsel >= 0) {
        rb = blockIdx.x;
        g = gsel;
    } else {
        tile_map(T, blockIdx.x, T.nrb, rb, g);
    }
    const int HR = (int)tile_lds_doubles(T, false);
    double *rows = lds;
    double *rc = lds + HR;
    const int64_t i0 = rb * T.H;
    const int64_t nloc = (i0 + T.H + 1 <= P.n) ? T.H + 1 : P.n - i0;   // rows incl. the halo
    const int64_t G = T.ngroups;
    double rr[1] = {0.0};
    if constexpr (FUSE) {
        if (ITER) {
            // the slice's loads RR at a time, all in flight (a load-then-add
            // loop waited out one memory latency per element, at the start of
            // every workgroup); same left-to-right order, padding adds +0
            constexpr int RR = 4;
            const int64_t ns = T.nrb * G, sl = rb * G + g;
            const bool cut = FUSE == 2 && P.rr_hi > P.rr_lo;
            int64_t lo = cut ? P.rr_lo : 0, span = (cut ? P.rr_hi : P.m) - lo;
            int64_t q0 = lo + sl * span / ns, q1 = lo + (sl + 1) * span / ns;
            if (gsel >= 0) {
                // this part's link range, cut to the rank's slice, over the row blocks
                const int64_t a = T.group_col[g] > lo ? T.group_col[g] : lo;
                const int64_t b = T.group_col[g + 1] < lo + span ? T.group_col[g + 1] : lo + span;
                const int64_t w = b > a ? b - a : 0;
                q0 = a + rb * w / T.nrb;
                q1 = a + (rb + 1) * w / T.nrb;
            }
            for (int64_t i0 = q0 + threadIdx.x; i0 < q1; i0 += RR * (int64_t)blockDim.x) {
                double v[RR];
#pragma unroll
                for (int q = 0; q < RR; ++q) {
                    const int64_t i = i0 + (int64_t)q * blockDim.x;
                    v[q] = (i < q1) ? r_load(P, i) : 0.0;
                }
#pragma unroll
                for (int q = 0; q < RR; ++q) rr[0] += v[q] * v[q];
            }
        }
    }
    // (the clear and its barrier: under the dealt walk's first loads, tiles.hpp
    // tile_walk_dealt's `mid`)
    auto clear = [&]() {
        PH(2);
        for (int i = threadIdx.x; i < HR; i += blockDim.x) {
            rows[i] = 0.0;
            if (MODE == 2) rc[i] = (i < nloc) ? colv_t<CV>(P, i0 + i) : 0.0;
            if (FX) rc[i] = 0.0;   // (the low words: integer 0)
        }
        __syncthreads();
        PH(3);
    };
    if constexpr (FX) {
        double fxs, inv;
        const bool bad = fx_scale(P.fx_a2 * rmax_of(rmax), fxs, inv);
        tile_walk_any<(MODE == 3 ? 0 : MODE), true>(T, rb, g, P.r, rows, rc, fxs, 1.0, clear);
        PH(4);
        __syncthreads();
        const double inv_lo = ldexp(inv, -fx_lo_shift(T.cols));
        for (int i = threadIdx.x; i < (int)nloc; i += blockDim.x) {
            const double v = fx_row(rows, i, HR, inv, inv_lo, bad);
            rows[i] = (MODE == 3 && G == 1) ? colv_t<CV>(P, i0 + i) * v : v;
        }
    } else if (P.r_fx > 0.0) {
        tile_walk_any<(MODE == 3 ? 0 : MODE), false, true>(T, rb, g, P.r, rows, rc, 1.0,
                                                            1.0 / P.r_fx, clear);
    } else {
        tile_walk_any<(MODE == 3 ? 0 : MODE)>(T, rb, g, P.r, rows, rc, 1.0, 1.0, clear);
    }
    PH(4);
    __syncthreads();
    PH(5);
    // wpart's tail: one slot per (group, row block) for the slices' r^2 sums
    double *rrp = P.wpart + G * T.nrb * (T.H + 1);
    if (FUSE && ITER && G > 1) {
        block_sum<1>(rr, red);
        if (threadIdx.x == 0)
            __hip_atomic_store(&rrp[g * T.nrb + rb], rr[0], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    bool fin = true;
    // dealt image, one group (MODE 3): w_i = colv_i * (sum of r over row i),
    // one product per row (the sums' order is not fixed anyway), formed in the
    // epilogue below; several groups: by the finishing workgroup
    // (FX: the conversion above formed the products already)
    const bool scale_epi = !FX && MODE == 3 && G == 1;
    if (G > 1 && gsel >= 0) {
        // the part pipeline: fixed roles (see above)
        if (gsel < G - 1) {
            double *wp = P.wpart + (g * T.nrb + rb) * (T.H + 1);
            for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x) wp[i] = rows[i];
            return;
        }
        for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x) {
            double o = 0.0;
            for (int64_t c = 0; c < G - 1; ++c)
                o += __hip_atomic_load(&P.wpart[(c * T.nrb + rb) * (T.H + 1) + i], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            o += rows[i];
            rows[i] = (MODE == 3) ? colv_t<CV>(P, i0 + i) * o : o;
        }
        __syncthreads();
    } else if (G > 1) {
        double *wp = P.wpart + (g * T.nrb + rb) * (T.H + 1);
        for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x)
            __hip_atomic_store(&wp[i], rows[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        fin = rowblock_last(tk2rb, rb, G, &row_last);
        if (fin) {
            for (int64_t i = threadIdx.x; i < nloc; i += blockDim.x) {
                double o = 0.0;
                for (int64_t c = 0; c < G; ++c)
                    o += __hip_atomic_load(&P.wpart[(c * T.nrb + rb) * (T.H + 1) + i],
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                rows[i] = (MODE == 3) ? colv_t<CV>(P, i0 + i) * o : o;
            }
            __syncthreads();
        }
    }
    constexpr int NS = FUSE ? 5 : 4;
    double sums[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sums[q] = 0.0;
    if (fin && BSLS_TILE_KO != 4) {   // (KO 4: no epilogue -- timing builds only)
        // K2E rows per thread per batch: every z index, then every operand of
        // the batch in flight at once (two round trips per batch instead of
        // two per row: C5's 19 rows per thread made the epilogue ~90 us)
        const int64_t iend = (nloc < T.H) ? nloc : T.H;
        constexpr int K2E = BSLS_K2E;
        for (int64_t ib = threadIdx.x; ib < iend; ib += K2E * blockDim.x) {
            int32_t jq[K2E];
            double ca[K2E], cb[K2E], gq[K2E], dq[K2E];
            [[maybe_unused]] double rq[REG ? K2E : 1];
#pragma unroll
            for (int q = 0; q < K2E; ++q) {
                const int64_t i = ib + (int64_t)q * blockDim.x;
                // (j < 0: a block's last x entry, also the matrix's last row)
                jq[q] = (i < iend) ? P.xz[i0 + i] : -1;
                ca[q] = cb[q] = 1.0;
                if (scale_epi && i < iend) {
                    ca[q] = colv_t<CV>(P, i0 + i);
                    cb[q] = (i + 1 < nloc) ? colv_t<CV>(P, i0 + i + 1) : 0.0;
                }
            }
#pragma unroll
            for (int q = 0; q < K2E; ++q) {
                gq[q] = dq[q] = 0.0;
                if (ITER && jq[q] >= 0) {
                    gq[q] = gp[jq[q]];
                    if (dzv) dq[q] = dzv[jq[q]];
                }
                if constexpr (REG) rq[q] = (jq[q] >= 0) ? P.reg_g[jq[q]] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < K2E; ++q) {
                const int64_t i = ib + (int64_t)q * blockDim.x;
                const int32_t j = jq[q];
                if (j < 0) continue;
                const double wa = scale_epi ? ca[q] * rows[i] : rows[i];
                const double wb = scale_epi ? cb[q] * rows[i + 1] : rows[i + 1];
                double gv = wa - wb;
                if constexpr (REG) gv = gv + rq[q];
                gout[j] = gv;
                if (ITER) {
                    const double dg = gv - gq[q];
                    const double dz = dq[q];
                    sums[0] += dg;
                    sums[1] += dz * dg;
                    sums[2] += dg * dg;
                    sums[3] += gv * gv;
                }
            }
        }
    }
    PH(6);
    if (!ITER || !fin) {
        PH_FLUSH(PH_K2);
        return;
    }
    if constexpr (FUSE) {
        if (G == 1) {
            sums[4] = rr[0];
        } else if (threadIdx.x == 0) {
            // (the group partials' hand-off above orders these slots too)
            double o = 0.0;
            for (int64_t c = 0; c < G; ++c)
                o += __hip_atomic_load(&rrp[c * T.nrb + rb], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            sums[4] = o;
        }
    }
    block_sum<NS>(sums, red);
    double tot[NS];
    // one slot per row block, summed in row-block order: with several groups
    // the finishing workgroup of a block varies from run to run, so its
    // blockIdx must not decide where the block's sums enter the reduction
    const bool last = (G == 1) ? last_block_sum<NS>(sums, part, ticket, tot, red)
                               : last_of_sum<NS>(sums, part, (unsigned)rb, (unsigned)T.nrb, ticket,
                                                 tot, red);
    if (last && threadIdx.x == 0) k2_store_sums<FUSE>(P, iter, tot);
    PH(7);
    PH_FLUSH(PH_K2);
}

// Stage 12 (the sliced schedule, after the all-reduce of scal[SUMDG..RR]):
// f(iter - 1) from the summed ||r||^2 and the stopping test of iter - 1 on
// its own g.g and dg.dg (kept by stage 10 in scal[PSUMDG..PGG]); on a stop the
// scal sums go back to that iteration's, as the unfused schedule leaves them.
__global__ void bb_shard_record(bsls_bb_problem P, int64_t iter) {
    if (threadIdx.x != 0) return;
    double *s = P.scal;
    const int64_t it = iter - 1;
    if (it > 0 && s[BSLS_S_STOP] != 0.0) return;
    const double rr = s[BSLS_S_RR];
    const double nr = sqrt(rr);
    const double fx = 0.5 * (nr * nr);      // 0.5 * la.norm(r)**2, main.py:53
    s[BSLS_S_FX] = fx;
    if (it <= 0) return;
    s[BSLS_S_ITER] = (double)it;
    s[BSLS_S_ZBUF] = (double)(it & 1);
    const int reason = bb_stop_reason(P, it, fx, s[BSLS_S_PGG], s[BSLS_S_PDGDG]);
    if (reason) {
        s[BSLS_S_STOP] = (double)reason;
        for (int q = 0; q < 4; ++q) s[BSLS_S_SUMDG + q] = s[BSLS_S_PSUMDG + q];
    }
}

// K2: g = N'(A' r); with ITER also dg = g - g_prev and the BB sums.  The
// workgroup's 16 panels (x-rows) are summed over every chunk of r; then lane
// position p of a panel has w_i in acc[p] and w_{i+1} in acc[p + 1] (the halo
// row), so N'w = w_i - w_{i+1} needs no exchange.  The column scales are
// loaded before the chunk loop; the epilogue's z indices and operands after
// it (the walk holds 122 of the 128 VGPRs; loading the indices early measured
// no faster).  The ITER epilogue reads g_prev and dz = z - z_prev (K3 wrote
// dz from the z's it holds, bit-identical to the subtraction here): 15.2 MB
// that no walk overlaps, where z and z_prev were 22.8 MB.
// REG: as bb_k2t.
template <int MODE, bool ITER, int FUSE = 0, bool REG = false>
__global__ __launch_bounds__(1024) void bb_k2(bsls_bb_problem P, const double *__restrict__ dzv,
                                              const double *__restrict__ gp,
                                              double *__restrict__ gout, double *part,
                                              unsigned *ticket, int64_t iter) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (ITER && P.scal[BSLS_S_STOP] != 0.0) {
        k2_stopped_sums<FUSE>(P);
        return;
    }
    const bsls_panels &M = P.AT;
    const int wv = threadIdx.x / WAVE, lane = lane_id();
    const int64_t panel = (int64_t)blockIdx.x * PANEL_WAVES + wv;
    const int64_t i0 = panel * M.prow;
    const bool live = panel < M.npanels;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double sc[4] = {0.0, 0.0, 0.0, 0.0};
    if (MODE == 2) {
        // unconditional loads at clamped rows (all in flight together)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + 64 * q + lane;        // halo row included
            const bool ok = live && 64 * q + lane <= M.prow && i < P.n;
            const double v = colv_at(P, ok ? i : 0);
            sc[q] = ok ? v : 0.0;
        }
    }
    panel_chunks<MODE>(M, blockIdx.x, wv, 0, M.nchunks, P.r, lds, s, sc);
    // w_{i+1}: the next lane, or lane 0 of the next slice (the halo row is
    // row prow of the panel)
    double nx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double dn = __shfl_down(s[q], 1, WAVE);
        const double wrap = (q < 3) ? __shfl(s[q < 3 ? q + 1 : q], 0, WAVE) : 0.0;
        nx[q] = (lane < 63) ? dn : wrap;
    }
    __syncthreads();   // the chunk table becomes the reduction scratch below
    constexpr int NS = FUSE ? 5 : 4;
    double sums[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sums[q] = 0.0;
    // epilogue operands: unconditional loads at clamped indices, all in flight
    int32_t j[4];
    double gpj[4], dzj[4];
    [[maybe_unused]] double rgj[REG ? 4 : 1];
    static_assert(!REG || FUSE == 0, "REG: the single-GCD K2");
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int pos = 64 * q + lane;
        const int64_t i = i0 + pos;
        const bool ok = live && pos < M.prow && i < P.n;
        const int32_t jj = P.xz[ok ? i : 0];
        j[q] = ok ? jj : -1;
    }
    if (ITER) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int32_t jc = j[q] >= 0 ? j[q] : 0;
            gpj[q] = gp[jc];
            dzj[q] = dzv ? dzv[jc] : 0.0;
        }
    }
    if constexpr (REG) {
#pragma unroll
        for (int q = 0; q < 4; ++q) rgj[q] = P.reg_g[j[q] >= 0 ? j[q] : 0];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (j[q] >= 0) {
            double g = s[q] - nx[q];
            if constexpr (REG) g = g + rgj[q];
            gout[j[q]] = g;
            if (ITER) {
                const double dg = g - gpj[q];
                const double dz = dzj[q];
                sums[0] += dg;
                sums[1] += dz * dg;
                sums[2] += dg * dg;
                sums[3] += g * g;
            }
        }
    }
    if (!ITER) return;
    if constexpr (FUSE) {   // stage 8 / 10: this workgroup's slice of ||r||^2 (see bb_k2t)
        const bool cut = FUSE == 2 && P.rr_hi > P.rr_lo;
        const int64_t lo = cut ? P.rr_lo : 0, span = (cut ? P.rr_hi : P.m) - lo;
        const int64_t q0 = lo + (int64_t)blockIdx.x * span / gridDim.x;
        const int64_t q1 = lo + ((int64_t)blockIdx.x + 1) * span / gridDim.x;
        for (int64_t i = q0 + threadIdx.x; i < q1; i += blockDim.x) {
            const double v = P.r[i];
            sums[4] += v * v;
        }
    }
    block_sum<NS>(sums, lds);
    double tot[NS];
    if (last_block_sum<NS>(sums, part, ticket, tot, lds) && threadIdx.x == 0)
        k2_store_sums<FUSE>(P, iter, tot);
}

}  // namespace bsls
