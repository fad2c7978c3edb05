// The text of the sweep kernel (no include guard: sf_band_sweep.h and sf_band_solve.h each compile it once).
//   SFB_SWEEP_KERNEL  the kernel's name
//   SFB_SWEEP_KEEP    0: logdet and Gram matrix only, L is never written anywhere (k_band_forms)
//                     1: the kernel takes a second argument sf_band_keep and additionally stores every block when it is
//                        final, straight from the registers that hold it (layout: sfb_keep_block): F_k = L_kk^-1 from the
//                        diagonal step, L_{k+1+I,k} and the forward-substituted right-hand sides from the solves.  A block in
//                        the accumulator layout is element lane + 64 r of its 256 doubles.
#if SFB_SWEEP_KEEP
#define SFB_KEPT(kb, j) , kept_at(kb, j)
#else
#define SFB_KEPT(kb, j)
#endif
template <int NRB>
#if SFB_SWEEP_KEEP
__global__ __launch_bounds__(1024) void SFB_SWEEP_KERNEL(sf_band_args a, sf_band_keep kp) {
    typedef double __attribute__((address_space(1))) * gkeep_t;  // global_store, not flat
    const gkeep_t keep = (gkeep_t)(kp.fac + (int64_t)blockIdx.x * kp.sfac);
    a.nhalf = 1;  // (only the single top-down sweep keeps its factor: the halves' code is not compiled)
#else
__global__ __launch_bounds__(1024) void SFB_SWEEP_KERNEL(sf_band_args a) {
#endif
    extern __shared__ double lds[];
    const int b = a.nhalf == 2 ? blockIdx.x >> 1 : blockIdx.x;
    const int half = a.nhalf == 2 ? blockIdx.x & 1 : 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nthreads = blockDim.x, nwaves = nthreads >> 6;
    const int nbr = a.nbr;
    constexpr int NR = NRB * BB, LDG = NR + 1;
    const sfb_lds L = sfb_lds_layout(nbr, NRB);        // (the launch passes L.bytes)
    double* Wb = lds + L.Wb;
    double* RH = lds + L.RH;
    double* Fb2 = lds + L.Fb2;
    double* G = lds + L.G;                             // row stride LDG
    double* pv = lds + L.pv;
    double* red = lds + L.red;
    typedef __attribute__((address_space(3))) int lds_int_t;  // ds_read / ds_add, not flat accesses
    // progress flags of the software pipeline (all monotonic):
    //   [0] F_k published (k+1)          [1] waves that placed block 0 of the newest row (4 per step)
    //   [2] X_{k+1,k} published (k+1)    [3] wave 0 done with column k (k+1)
    //   [4] workers done with column k (k+1)   [5] worker barrier arrivals   [7] a spin timed out
    volatile lds_int_t* sync = (volatile lds_int_t*)(lds + L.sync);
    volatile lds_int_t* ptab = (volatile lds_int_t*)(lds + L.ptab);  // [16 waves][SFB_PT] (I << 8 | J) update pairs, [..][SFB_PT-1] = count

    const int n = a.n, W = a.halfwidth, nrhs = a.r.nrhs;
    const int nblk = (n + BB - 1) / BB;
    const int rev = half ? nblk * BB - 1 : -1;                            // reversed indexing (bottom-up half)
    const int kend = a.nhalf == 2 ? (half ? a.kend1 : a.kend0) : nblk;   // block columns to eliminate
    const double* __restrict__ band = a.band + (int64_t)b * a.sband;
    const sf_band_rhs R = a.r.of(b);                                      // this matrix's right-hand sides
    const int row_elems = nbr * BB * BB, all_elems = row_elems + NR * BB;
    auto wrap = [&](int slot) { return slot >= nbr ? slot - nbr : slot; };  // slot in [0, 2 nbr)
#if SFB_SWEEP_KEEP
    // block j of column kb's record.  Uniform, and told so: the base stays in scalar registers and the lane's element is the
    // only vector part of the address (as a running vector pointer it costs the two registers the sweep does not have)
    auto kept_at = [&](int kb, int j) {
        const unsigned long long p = (unsigned long long)(keep + sfb_keep_block(kb, j, nbr, NRB));
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)p), hi = __builtin_amdgcn_readfirstlane((unsigned)(p >> 32));
        return (gkeep_t)(((unsigned long long)hi << 32) | lo);
    };
    // A block in the accumulator layout to its place: scalar base + the lane's byte offset 8 * lane, rows 4 r at 512 r bytes.
    // Written out, the lane number taken from v_mbcnt: as C++ the address (or, hoisted out of the sweep's loop, the lane's
    // offset) occupies vector registers through the whole step, which the sweep does not have -- it spilled to scratch.
    auto keep_store = [&](gkeep_t dst, const sf_d4& v) {
        unsigned off;
        asm volatile(
            "v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshlrev_b32 %0, 3, %0\n\t"
            "global_store_dwordx2 %0, %1, %5\n\tglobal_store_dwordx2 %0, %2, %5 offset:512\n\t"
            "global_store_dwordx2 %0, %3, %5 offset:1024\n\tglobal_store_dwordx2 %0, %4, %5 offset:1536"
            : "=&v"(off)
            : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"(dst)
            : "memory");
    };
#endif

    // ---- initial window: block rows 0 .. nbr-1
    for (int gb = 0; gb < nbr; ++gb)
        for (int e = tid; e < all_elems; e += nthreads) {
            const double v = sfb_fetch(band, R.rhs, R.rhs0, gb, e, nbr, n, W, a.ldb, nrhs, R.ldr, rev);
            if (e < row_elems) {
                const int blk = e >> 8, gc = gb - nbr + 1 + blk;
                if (gc >= 0) Wb[sfb_pair(gb, gc) * BS + ((e >> 4) & 15) * BLD + (e & 15)] = v;
            } else {
                const int q = e - row_elems, r = q >> 4;
                RH[((r >> 4) * nbr + gb) * BS + (r & 15) * BLD + (q & 15)] = v;
            }
        }
    for (int e = tid; e < NR * LDG; e += nthreads) G[e] = 0.0;
    if (tid < 16) sync[tid] = 0;

    const int l15 = lane & 15, lq = lane >> 4;
    // Wave 0: Cholesky of the 16 x 16 diagonal block AND the inverse of its factor in the MFMA accumulator layout: the
    // step of SF_POTRF16_ACC (sf_device.h, explained there) without L^T and with the identity set in the load loop.
    // Its own copy: written with the macro the sweep compiles to another instruction order.
    int bad = 0;
    auto potrf16 = [&](int kb, int ks) {  // ks = kb % nbr
        const double* D = Wb + sfb_pair(ks, ks) * BS;
        sf_d4 acc, f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = lq + 4 * r;
            acc[r] = D[max(row, l15) * BLD + min(row, l15)];  // only the lower triangle is maintained
            f[r] = row == l15 ? 1.0 : 0.0;
        }
        double p = sf_readlane_d(acc[0], 0);
        double pkeep = 1.0;  // lane j keeps pivot j: one LDS store and one sign test after the loop
#pragma unroll
        for (int j = 0; j < BB; ++j) {
            const int qj = j & 3, rj = j >> 2;
            pkeep = lane == j ? p : pkeep;
            const double rs = sf_rsqrt(p);
            const bool in_q = lq == qj;
            const double v = (in_q && l15 > j) ? acc[rj] * rs : 0.0;  // l_ij, i = l15 > j
            const double g = in_q ? f[rj] * rs : 0.0;                 // row j of F, scaled
            if (in_q) f[rj] = g;
            if (j + 1 < BB) {
                const double an = sf_readlane_d(acc[(j + 1) >> 2], ((j + 1) & 3) * 16 + j + 1);
                const double vn = sf_readlane_d(v, qj * 16 + j + 1);
                p = __builtin_fma(-vn, vn, an);
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 1);  // blgp = neg:[1,0,0]: -A B + C
            f = __builtin_amdgcn_mfma_f64_16x16x4f64(v, g, f, 0, 0, 1);
        }
        if (lane < BB) pv[(kb & 1) * BB + lane] = pkeep;
        const unsigned long long neg = __ballot(lane < BB && !(pkeep > 0.0));
        if (neg && !bad) bad = kb * BB + __ffsll((long long)neg);
#pragma unroll
        for (int r = 0; r < 4; ++r) Fb2[(kb & 1) * BS + (lq + 4 * r) * BLD + l15] = f[r];
#if SFB_SWEEP_KEEP
        keep_store(kept_at(kb, 0), f);
#endif
    };

    // Prefetch roles, fixed per thread: waves >= 4 load the band (groups of 256 threads = one 16 x 16
    // block each, element (pr, pc) of it), waves 1..3 the right-hand-side columns.  Per slot: a running
    // source pointer (one block row further every step) and the LDS offset of the element inside its
    // destination block; whether a slot loads at all is a per-thread constant, whether its row is still
    // inside the matrix is one comparison per step (top-down sweeps only).
    const int ngroups = sfb_loader_groups(nwaves);     // 256-thread groups of band loaders (1..3)
    const int pg = wave >= 4 ? (wave - 4) >> 2 : 0;    // this wave's group (uniform)
    const bool band_loader = wave >= 4;
    typedef const double __attribute__((address_space(1))) * gptr_t;  // keeps the prefetch on global_load
    gptr_t pptr[SFB_PF];
    int poff[SFB_PF];
    int pmask = 0;                                     // bit q: slot q loads; bit 4+q: identity padding when out of range
    int prow;                                          // padded-matrix row of this thread's elements (next block row)
    const int pstep = (rev >= 0 ? -BB : BB) * (band_loader ? a.ldb : 1);  // doubles per step
    {
        const int lt = tid - 256, pr = (lt >> 4) & 15, pc = lt & 15;
        const int rt = tid - 64;
        prow = nbr * BB + (band_loader ? pr : (rt & 15));
#pragma unroll
        for (int q = 0; q < SFB_PF; ++q) {
            if (band_loader) {
                const int blk = pg + q * ngroups;
                const int d = (nbr - 1 - blk) * BB + pr - pc;
                const int io = rev >= 0 ? rev - prow + d : prow;  // larger original index of the pair
                const bool okd = blk < nbr && d >= 0 && d <= W;
                pmask |= (okd ? 1 : 0) << q;
                pmask |= ((blk < nbr && d == 0) ? 16 : 0) << q;
                pptr[q] = (gptr_t)(band + (int64_t)io * a.ldb + (okd ? d : 0));
                poff[q] = pr * BLD + pc;
            } else {
                const int e = rt + q * 192, r = e >> 4;
                const int io = rev >= 0 ? rev - prow : prow;
                const bool okr = wave >= 1 && e < NR * BB && r < nrhs;
                pmask |= (okr ? 1 : 0) << q;
                pptr[q] = (gptr_t)(R.row(r) + io);
                poff[q] = (wave >= 1 && e < NR * BB) ? (e >> 8) * nbr * BS + ((e >> 4) & 15) * BLD + (e & 15) : -1;
            }
        }
    }
    double pf[SFB_PF];                                 // prefetched values (band or rhs), final when they land
    double ld_acc = 0.0;                               // wave `logwave`, lanes 0..15: partial sums of log(pivot)
    __syncthreads();

    const int nb1 = nbr - 1, RB = nb1 + NRB;
    auto spin_until = [&](int which, int target) {
        int guard = 0;
        while (sync[which] < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++guard > (1 << 22)) {  // cannot happen; keeps a logic error from hanging the GPU
                sync[7] = 1;
                break;
            }
        }
        asm volatile("" ::: "memory");
    };
    auto publish = [&](int which, int value) {  // after this wave's LDS writes have landed
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) sync[which] = value;
    };
    // ---- block addressing.  Every 16 x 16 block lives at lds + index * BS: window blocks by ring-slot pair,
    //      then the right-hand-side ring (index NBW + rb * nbr + slot).  Which blocks an operation touches
    //      depends on the ring phase ks = k % nbr only, so each wave tabulates its operations ONCE, lane ks
    //      of a VGPR holding the packed block indices for that phase; per step one v_readlane replaces
    //      the scalar index arithmetic (pair(), wrap(), the band/rhs/Gram case split), which otherwise
    //      costs more issue time than the MFMAs it feeds.
    const int NBW = nbr * (nbr + 1) / 2;
    auto idxP = [&](int ks_, int I) {  // row block I below the diagonal block of column ks_
        return I < nb1 ? sfb_pair(wrap(ks_ + 1 + I), ks_) : NBW + (I - nb1) * nbr + ks_;
    };
    auto pack_update = [&](int ks_, int I, int J) {  // A | B << 8 | C << 16 | gram << 24
        int c, gram = 0;
        if (J >= nb1) {
            c = (I - nb1) * 4 + (J - nb1);
            gram = 1;
        } else if (I < nb1) {
            c = sfb_pair(wrap(ks_ + 1 + I), wrap(ks_ + 1 + J));
        } else {
            c = NBW + (I - nb1) * nbr + wrap(ks_ + 1 + J);
        }
        return idxP(ks_, I) | (idxP(ks_, J) << 8) | (c << 16) | (gram << 24);
    };
    const int tl = lane < nbr ? lane : 0;  // ring phase this lane tabulates
    const int oAB = l15 * BLD + 4 * lq;   // operand fragment (K slice lq = columns 4 lq .. 4 lq + 3 of row l15)
    // X = P F^T in place (B operand = rows of F = L_kk^-1; K slice lq of MFMA kk stands for k = 4 lq + kk
    // in both operands: contiguous, paired LDS reads)
#if SFB_SWEEP_KEEP
    auto xsolve = [&](int pidx, const double* Fb, gkeep_t kept) {  // kept: where the solved block is stored
#else
    auto xsolve = [&](int pidx, const double* Fb) {
#endif
        double* P = lds + pidx * BS;
        sf_d4 acc = {0.0, 0.0, 0.0, 0.0};
        const double* Ap = P + oAB;
        const double* Bp = Fb + oAB;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ap[kk], Bp[kk], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) P[(lq + 4 * r) * BLD + l15] = acc[r];
#if SFB_SWEEP_KEEP
        keep_store(kept, acc);
#endif
    };
    // Trailing update  C -= P_I P_J^T  of block (I, J), I >= J, of [band rows below ; rhs rows] x [same]
    // (Gram blocks accumulate with the same sign: G = -Z Z^T, negated on output), split into its operand
    // reads and its MFMAs + write-back so that the next block's operands can be read under the MFMAs.
    auto load_ops = [&](int w, sf_d4& c, sf_d4& av, sf_d4& bv, int& ldc) -> double* {
        const double* Ap = lds + (w & 255) * BS + oAB;
        const double* Bp = lds + ((w >> 8) & 255) * BS + oAB;
        const int ci = (w >> 16) & 255;
        double* Cb;
        if (w >> 24) {
            ldc = LDG;
            Cb = G + ((ci >> 2) * BB) * LDG + (ci & 3) * BB + lq * LDG + l15;
        } else {
            ldc = BLD;
            Cb = lds + ci * BS + lq * BLD + l15;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = Cb[4 * r * ldc];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            av[kk] = Ap[kk];
            bv[kk] = Bp[kk];
        }
        return Cb;
    };
    auto mma_store = [&](double* Cb, int ldc, sf_d4 c, const sf_d4& av, const sf_d4& bv) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) c = __builtin_amdgcn_mfma_f64_16x16x4f64(av[kk], bv[kk], c, 0, 0, 1);  // neg:[1,0,0]
#pragma unroll
        for (int r = 0; r < 4; ++r) Cb[4 * r * ldc] = c[r];
    };

    // ---- division of labour.  Wave 0 runs the sequential chain by itself and never meets a barrier:
    //          potrf(k) -> F_k | X_{k+1,k} = A_{k+1,k} F_k^T | D_{k+1} -= X X^T | potrf(k+1) ...
    //      The other waves ("workers") trail by one column: they solve the rest of block column k against
    //      F_k, apply column k to the window (every block pair except (0,0)), fetch the next 16 rows from
    //      HBM and place them into the slots column k retires.  Flags in LDS order the two.
    const int nworkers = nwaves - 1;
    const int logwave = nwaves - 4;                    // accumulates log(pivot): no solves, the smallest share of updates
    const int wpos = sfb_worker_pos(wave, nwaves);     // position of this wave among the workers
    if (tid >= 1 && tid < nwaves) {
        // pair list of wave `tid`: round robin over the workers, those on wave 0's SIMD last (the
        // remainder goes to the others)
        const int w = tid, wp = sfb_worker_pos(w, nwaves);
        const int npairs = RB * (RB + 1) / 2;
        int cnt = 0;
        for (int t = 1 + wp; t < npairs; t += nworkers) {
            int I = 0;
            while ((I + 1) * (I + 2) / 2 <= t) ++I;
            if (cnt < SFB_PT - 1) ptab[w * SFB_PT + cnt] = (I << 8) | (t - I * (I + 1) / 2);
            ++cnt;
        }
        ptab[w * SFB_PT + SFB_PT - 1] = cnt < SFB_PT ? cnt : SFB_PT - 1;
        if (cnt >= SFB_PT) sync[7] = 1;  // cannot happen for the window sizes the launcher admits
    }
    __syncthreads();

    if (wave == 0) {
        // lane ks: P0 = block (k+1, k) | D_{k+1} << 8
        const int tab0 = idxP(tl, 0) | (sfb_pair(wrap(tl + 1), wrap(tl + 1)) << 8);
        __builtin_amdgcn_s_setprio(3);  // the other waves of this SIMD do bulk MFMA work
        int ks = 0;
        for (int kb = 0; kb < kend; ++kb, ks = wrap(ks + 1)) {
            potrf16(kb, ks);
            publish(0, kb + 1);
            const int w0 = __builtin_amdgcn_readlane(tab0, ks);
            const int p0 = w0 & 255;
            spin_until(4, kb);                       // column kb-1 fully applied by the workers
            xsolve(p0, Fb2 + (kb & 1) * BS SFB_KEPT(kb, 1));
            publish(2, kb + 1);
            {                                        // the next diagonal block
                sf_d4 c, av, bv;
                int ldc;
                double* Cb = load_ops(p0 | (p0 << 8) | ((w0 >> 8) << 16), c, av, bv, ldc);
                mma_store(Cb, ldc, c, av, bv);
            }
            publish(3, kb + 1);
        }
        __builtin_amdgcn_s_setprio(0);
    } else {
        const int mycnt = __builtin_amdgcn_readfirstlane(ptab[wave * SFB_PT + SFB_PT - 1]);
        // operation tables (lane = ring phase)
        int tabu[SFB_PT - 1];
#pragma unroll
        for (int p = 0; p < SFB_PT - 1; ++p) {
            const int e = __builtin_amdgcn_readfirstlane(ptab[wave * SFB_PT + (p < mycnt ? p : 0)]);
            tabu[p] = p < mycnt ? pack_update(tl, e >> 8, e & 255) : 0;
        }
        const int xI0 = 1 + wpos, xI1 = 1 + wpos + nworkers;  // row blocks this wave solves (at most two)
        const int tabx = (xI0 < RB ? idxP(tl, xI0) : 0) | ((xI1 < RB ? idxP(tl, xI1) : 0) << 8);
        int tabp = 0;  // destination block of prefetch slot q when column slot `lane` retires
#pragma unroll
        for (int q = 0; q < SFB_PF; ++q) {
            const int blk = pg + q * ngroups;
            tabp |= (band_loader ? (blk < nbr ? sfb_pair(tl, wrap(tl + 1 + blk)) : 0) : NBW + tl) << (8 * q);
            if (band_loader && blk >= nbr) poff[q] = -1;
        }
        int arrivals = 0;
        auto worker_barrier = [&]() {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            arrivals += nworkers;
            if (lane == 0) __hip_atomic_fetch_add((lds_int_t*)&sync[5], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            spin_until(5, arrivals);
        };
        int ks = 0;
        for (int kb = 0; kb < kend; ++kb, ks = wrap(ks + 1)) {
            // ---- solve block column kb (row block 0 is wave 0's)
            const int wx = __builtin_amdgcn_readlane(tabx, ks);
            spin_until(0, kb + 1);
            if (xI0 < RB) {
                if (xI0 == nb1 - 1 && kb > 0) spin_until(1, 4 * kb);  // the newest row: placed by four waves
                xsolve(wx & 255, Fb2 + (kb & 1) * BS SFB_KEPT(kb, 1 + xI0));
            }
            if (xI1 < RB) {
                if (xI1 == nb1 - 1 && kb > 0) spin_until(1, 4 * kb);
                xsolve((wx >> 8) & 255, Fb2 + (kb & 1) * BS SFB_KEPT(kb, 1 + xI1));
            }
            worker_barrier();
            // ---- HBM prefetch of block row kb + nbr (lands under the updates)
            if (kb + 1 < kend) {
                // straight-line code: all loads are issued back to back, nothing here reads their results.
                // Rows beyond the matrix (padding up to a multiple of 16) become identity rows; a bottom-up
                // sweep never leaves the matrix (its order is a multiple of 16).
                const bool inr = rev >= 0 || prow < n;
                const int live = inr ? pmask : 0;
#pragma unroll
                for (int q = 0; q < SFB_PF; ++q) {
                    pf[q] = (!inr && ((pmask >> (4 + q)) & 1)) ? 1.0 : 0.0;
                    if ((live >> q) & 1) pf[q] = *pptr[q];
                    pptr[q] += pstep;
                }
                prow += BB;
            }
            // ---- apply column kb to the window (operands of the next block are read while the matrix
            //      core works on the current one)
            spin_until(2, kb + 1);
            {
                sf_d4 cA, aA, bA, cB, aB, bB;
                double *pA = nullptr, *pB = nullptr;
                int ldA = BLD, ldB = BLD;
                if (mycnt > 0) pA = load_ops(__builtin_amdgcn_readlane(tabu[0], ks), cA, aA, bA, ldA);
#pragma unroll
                for (int p = 0; p < SFB_PT - 1; p += 2) {
                    if (p + 1 < SFB_PT - 1 && p + 1 < mycnt) pB = load_ops(__builtin_amdgcn_readlane(tabu[p + 1 < SFB_PT - 1 ? p + 1 : 0], ks), cB, aB, bB, ldB);
                    if (p < mycnt) mma_store(pA, ldA, cA, aA, bA);
                    if (p + 2 < SFB_PT - 1 && p + 2 < mycnt) pA = load_ops(__builtin_amdgcn_readlane(tabu[p + 2 < SFB_PT - 1 ? p + 2 : 0], ks), cA, aA, bA, ldA);
                    if (p + 1 < SFB_PT - 1 && p + 1 < mycnt) mma_store(pB, ldB, cB, aB, bB);
                }
            }
            if (wave == logwave && lane < BB) ld_acc += log(pv[(kb & 1) * BB + lane]);  // (its share of updates is the smallest)
            worker_barrier();
            if (wave == 1) publish(4, kb + 1);
            // ---- the prefetched rows land in the slots of column kb
            if (kb + 1 < kend) {
                spin_until(3, kb + 1);
                const int wp = __builtin_amdgcn_readlane(tabp, ks);
#pragma unroll
                for (int q = 0; q < SFB_PF; ++q)
                    if (poff[q] >= 0) lds[((wp >> (8 * q)) & 255) * BS + poff[q]] = pf[q];
                if (wave >= 4 && wave < 8) {  // group 0 holds block 0 = (new row, column kb+1) in its first register
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane == 0) __hip_atomic_fetch_add((lds_int_t*)&sync[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }
    __syncthreads();

    // ---- outputs
    if (wave == logwave && lane < BB) red[lane] = ld_acc;
    __syncthreads();
    double ldsum = 0.0;
    if (tid == 0) {
        for (int i = 0; i < BB; ++i) ldsum += red[i];
        if (sync[7] && a.info) a.info[b] = SF_INFO_INTERNAL;  // a pipeline flag wait timed out
        else if (bad && a.info && a.info[b] == 0) {
            // bottom-up half: report the column in the original numbering
            a.info[b] = half ? nblk * BB - bad + 1 : bad + a.info_off;
        }
    }
    if (a.nhalf == 2) {
        // what is left of the separator (block rows/columns kend .. kend+nb1-1): A_MM minus this half's
        // Schur contribution, its right-hand-side columns, the partial Gram matrix and log-determinant
        const int nm = nb1 * BB;
        const int64_t slot2 = (int64_t)b * 2 + half;
        double* dM = a.dumpM + slot2 * nm * nm;
        for (int e = tid; e < nm * nm; e += nthreads) {
            const int i = e / nm, j = e - i * nm;
            if (j > i) continue;
            const int rs = (kend + (i >> 4)) % nbr, cs = (kend + (j >> 4)) % nbr;
            dM[e] = Wb[sfb_pair(rs, cs) * BS + (i & 15) * BLD + (j & 15)];
        }
        double* dR = a.dumpR + slot2 * NR * nm;
        for (int e = tid; e < NR * nm; e += nthreads) {
            const int r = e / nm, j = e - r * nm;
            dR[e] = RH[((r >> 4) * nbr + (kend + (j >> 4)) % nbr) * BS + (r & 15) * BLD + (j & 15)];
        }
        double* dG = a.dumpG + slot2 * nrhs * nrhs;
        for (int e = tid; e < nrhs * nrhs; e += nthreads) dG[e] = sfb_gram(G, LDG, e / nrhs, e % nrhs);
        if (tid == 0) a.dumpL[slot2] = ldsum;
        return;
    }
    if (tid == 0) a.logdet[b] = ldsum + (a.logdet_add ? a.logdet_add[b] : 0.0);
    double* out = a.gram + (int64_t)b * nrhs * nrhs;
    const double* gadd = a.gram_add ? a.gram_add + (int64_t)b * nrhs * nrhs : nullptr;
    for (int e = tid; e < nrhs * nrhs; e += nthreads) out[e] = sfb_gram(G, LDG, e / nrhs, e % nrhs) + (gadd ? gadd[e] : 0.0);
}
#undef SFB_KEPT
