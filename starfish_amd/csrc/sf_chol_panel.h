// The narrow panel step: sf_panel_args / sf_panel_task, the body sf_panel_body and its kernel k_chol_panel.
// Used by the fused, wide and band sequences (the kernel) and by the panel tasks of k_potrf_dataflow (the body).
#pragma once
#include "sf_device.h"
#include "sf_chol_tile.h"

// ---------------------------------------------------------------------------------------------
// Fused left-looking panel step (panel width = tile edge = 128).  One workgroup owns a 128-row slab
// of the panel [k0, k0 + pw) and does, without leaving the CU:
//   1  T  = C[slab, panel] - L[slab, :k0] L[panel rows, :k0]^T          long K, the k_gemm_nt main loop
//   2  L  = T W,  W = L_kk^-T (Wt = L_kk^-1 from k_diag_lds)            K = pw, triangular
//   3  L -> C[slab, panel] in place;  rhs[slab] -= L z_k                (forward substitution rides along)
//   4  S  = C[slab, slab] - L L^T                                       K = pw, lower triangle only
// Steps 2 and 4 take their A operand from the accumulators through LDS (32-column chunks): the panel
// scratch T of the unfused scheme is never written or read back, and the short-K launches G and R
// (0.3 of peak, all tiles of a round in the same memory phase) are gone.  In step 2 the chunks are
// visited in DESCENDING k order: L block columns need exactly the chunks up to their own, so a wave
// dumps a T block at the moment its registers become the accumulators of the L block -- no second
// accumulator set.  Step 4 uses the 36-blocks-on-8-waves layout of sf_syrk_diag_tile.
// pw == 0: nothing but the copy of the diagonal tile to Sout (start of the factorisation).
struct sf_panel_args {
    double* C;
    int64_t sC;
    int lda, n;
    int k0, pw;       // panel columns [k0, k0 + pw), pw in {0, 64, 128}
    int row0, nslab;  // nslab slabs of 128 rows, the first at row0 (multiple of 128); the last one may be shorter
    int slab_step;    // distance between consecutive slabs of this launch, in slabs (slab groups are interleaved)
    // split-K for launches that cannot fill the chip (late panels, small batches): mode 1 = ksplit workgroups per
    // slab each accumulate kchunk K-slabs and park their 128 x 128 partial sum in `part`; mode 2 = one workgroup
    // per slab adds the partial sums in fixed order (deterministic) and runs steps 2-4; mode 0 = everything at once
    int ksplit, kchunk;
    double* part;     // [tiles * ksplit][128 * 128]
    const double* Wt; // [batch] x sW: Wt[c][k] = (L_kk^-1)[c][k], row stride SF_LDT
    int64_t sW;
    double* rhs;      // [batch] x ldr or NULL
    int ldr;
    double* Sout;     // updated diagonal tile goes here (row stride ldS) instead of in place when non-NULL
    int64_t sS;
    int ldS;
    const double* genY;  // matrix-free start (see sf_gemm_args)
    const unsigned char* tilemap;
    int64_t sY;
    int ldy, mpad, nt128;
    // bordered band matrices (sf_launch_potrf_band): rows < nband have no entries further than kband columns left of
    // the diagonal, so the K loop of a slab starts at its first non-zero column; rows >= nband (the border: dense
    // rows that ride along) form one extra slab at xrow0, the last of the launch.  All 0 for dense matrices.
    int kband, nband, xrow0;
    // shifted frame (sf_potrf_front_pad): C, rhs and genY point fp (lda + 1) / fp / fp elements BEFORE the data, n / k0 /
    // row0 / the tile map count in that frame.  Rows and columns < fp are virtual (identity): every K loop starts at
    // column fp, the panel-0 accesses that would touch a virtual column are predicated.  0 for unshifted matrices.
    int fp;
    int prio;  // wave priority (s_setprio) of the whole workgroup: the chain's launches share their SIMDs with bulk workgroups
    // dataflow sequence (k_potrf_dataflow): the K range of a partial-sum task ends at K slab kstop (0: at the panel); MODE 3
    // (partial sums added, then the K slabs [ktail, panel) in the same workgroup) starts its own loop at ktail; before the
    // triangular solve the workgroup waits until *wflag >= wval (the counter the diagonal-tile task publishes)
    int kstop, ktail;
    const int* wflag;
    int wval;
    int* abort_flag;
};

// The fields of a step that differ from task to task inside k_potrf_dataflow (everything else of sf_panel_args is constant
// over a factorisation and stays in the kernel arguments: a per-task copy of the whole structure does not fit the SGPRs)
struct sf_panel_task {
    int k0, pw, row0, nslab, slab_step;
    int ksplit, kchunk, kstop, ktail;
    double* part;
    const double* Wt;
    int64_t sW;
    double* Sout;
    const int* wflag;
    int wval;
    int* abort_flag;
    int* lds_int;  // one int of LDS for the wait's broadcast
    int* top_flag; // dataflow chain / front task: counter set to top_val as soon as L is stored (before step 4)
    int top_val;
    const int* sflag;  // ... and the counter (>= sval) that says the slab's diagonal tile is ready for step 4
    int sval;
    long long* stamps;  // tuning builds: wall-clock stamps {K work done, diagonal tile there, L published, step 4 may start}
    int prio;
};
__device__ __forceinline__ sf_panel_task sf_task_of(const sf_panel_args& g) {
    sf_panel_task q;
    q.k0 = g.k0;
    q.pw = g.pw;
    q.row0 = g.row0;
    q.nslab = g.nslab;
    q.slab_step = g.slab_step;
    q.ksplit = g.ksplit;
    q.kchunk = g.kchunk;
    q.kstop = g.kstop;
    q.ktail = g.ktail;
    q.part = g.part;
    q.Wt = g.Wt;
    q.sW = g.sW;
    q.Sout = g.Sout;
    q.wflag = g.wflag;
    q.wval = g.wval;
    q.abort_flag = g.abort_flag;
    q.lds_int = nullptr;
    q.top_flag = nullptr;
    q.top_val = 0;
    q.sflag = nullptr;
    q.sval = 0;
    q.stamps = nullptr;
    q.prio = g.prio;
    return q;
}

// a pointer the compiler must treat as wave-uniform (an SGPR pair): the operand base of the direct-to-LDS loads
__device__ __forceinline__ const double* sf_uniform_ptr(const double* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (const double*)(((unsigned long long)hi << 32) | lo);
}

// granule swizzle of the main loop's LDS image (see k_chol_panel)
__device__ __forceinline__ int sf_swz(int row) {
    const int t = (row >> 1) & 7;
    return t ^ ((((t >> 1) ^ (t >> 2)) & 1) << 1);
}

// one 16-wide K block of the triangular solve for the 16-column blocks ni >= NI_LO of a wave
template <int NI_LO>
__device__ __forceinline__ void sf_solve_step(sf_d4 (&acc)[2][4], const double* Ab, const double* Bb) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        double a[2], bb[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = Ab[i * 16 * CLD + ks * 4];
#pragma unroll
        for (int i = NI_LO; i < 4; ++i) bb[i] = Bb[i * 16 * GLD + ks * 4];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = NI_LO; ni < 4; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], bb[ni], acc[mi][ni], 0, 0, 0);
    }
}

// MODE 0: the whole step; 1: split-K partial sums only; 2: partial sums added in split order + steps 2-4; 3: as 2, with the
// K slabs [g.ktail, panel) accumulated by this workgroup after the partial sums (dataflow sequence: the chain's step).
// `id` = tile (MODE 1: tile * ksplit + split) index; sm / red: 4 * GT * GLD + 2 * GT doubles of LDS.
// (GA: `const sf_panel_args`, or the same in the constant address space -- the kernel arguments of k_potrf_dataflow)
// (MODE 3 with ksplit = 0, ktail = 0 is MODE 0, and with ktail = the panel's K slab count it is MODE 2: k_potrf_dataflow runs
// every task type but the partial sums through ONE inlined copy of <3> -- see there.)
template <bool RHS, int MODE, class GA>
__device__ __forceinline__ void sf_panel_body(GA& g, const sf_panel_task& tk, const int id, double* __restrict__ sm,
                                              double (*red)[GT], const int tid) {
    constexpr int TM = 2, TN = 4;
    double(*As)[GT * GLD] = (double(*)[GT * GLD]) sm;
    double(*Bs)[GT * GLD] = (double(*)[GT * GLD])(sm + 2 * GT * GLD);
    double* Ach = sm;  // 128 x CLD chunk buffer of the epilogue (aliases As)

    // (integer division runs on the VALU: without the readfirstlane its wave-uniform results -- and every address and loop
    // bound derived from them -- would live in VGPRs)
    const int tile = __builtin_amdgcn_readfirstlane(MODE == 1 ? id / tk.ksplit : id);
    const int sp = __builtin_amdgcn_readfirstlane(MODE == 1 ? id - tile * tk.ksplit : 0);
    const int b = __builtin_amdgcn_readfirstlane(tile / tk.nslab);
    const int sl = tile - b * tk.nslab;
    const int row0 = (g.xrow0 && sl == tk.nslab - 1) ? g.xrow0 : tk.row0 + sl * tk.slab_step * GT;
    const int rows_here = min(GT, ((g.nband && row0 < g.nband) ? g.nband : g.n) - row0);
    const int pw = tk.pw, k0 = tk.k0;
    const int cfp = k0 == 0 ? g.fp : 0;  // panel columns below cfp are virtual (zero below the diagonal tile)
    if (tk.prio) __builtin_amdgcn_s_setprio(2);

    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // rows wm*32.., cols wn*64..; waves w and w + 4 share a SIMD: they get different column halves, because in
    // the triangular solve the two halves have different amounts of work
    const int wm = w >> 1, wn = (w ^ (w >> 2)) & 1;
    const int l15 = lane & 15, lq = lane >> 4;
    double* Cb = g.C + (int64_t)b * g.sC;

    sf_d4 acc[TM][TN];
    if (pw > 0) {
        // ---------------------------------------------------------------- 1: long-K update
        const int lr = tid >> 3, lc = (tid & 7) * 2;
        const double* Ap[2];
        const double* Bp[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            Ap[p] = Cb + (int64_t)(row0 + min(lr + 64 * p, rows_here - 1)) * g.lda + lc;
            Bp[p] = Cb + (int64_t)(k0 + min(lr + 64 * p, pw - 1)) * g.lda + lc;
        }
        // Operand staging: DIRECT global -> LDS loads (global_load_lds_dwordx4: no staging registers, no ds_write
        // pass).  A wave instruction deposits 64 consecutive 16-byte granules = 8 unpadded rows of a 16-double K slab;
        // bank conflicts are avoided by an XOR swizzle of the granule index with sf_swz(row), applied on the SOURCE
        // address here and on the fragment reads below (the LDS image itself is lane-linear).  The swizzle is made
        // for the lane groups of ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...: each holds all 16 rows of a
        // fragment once, rows 0-3 / 12-15 with one granule column and rows 4-11 with the column two further): with
        // t = (row >> 1) & 7, rows with t in {2,3,4,5} get t ^ 2, the others t -- 16 distinct 16-byte bank slots.
        const int grow = lane >> 3, gpos = lane & 7;  // row within the 8-row group, granule slot within the row
        // (addresses = a wave-uniform base in SGPRs, advanced along K by scalar adds, + a 32-bit lane offset: four VGPRs
        // instead of four 64-bit pointers advanced by VALU adds -- the kernel sits at the 128-VGPR limit, and a pointer that
        // spills is reloaded inside the K loop, where the wait for the scratch load also waits for the operand loads)
        unsigned Aoff[2], Boff[2];
        const double* Abase = sf_uniform_ptr(Cb + (int64_t)row0 * g.lda);
        const double* Bbase = sf_uniform_ptr(Cb + (int64_t)k0 * g.lda);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = 16 * w + 8 * q + grow;
            const int c = gpos ^ sf_swz(row);
            Aoff[q] = (unsigned)(min(row, rows_here - 1) * g.lda + 2 * c) * 8u;
            Boff[q] = (unsigned)(min(row, pw - 1) * g.lda + 2 * c) * 8u;
        }
        typedef __attribute__((address_space(3))) void* lds_ptr;
        double* A2 = sm;                // [2][128 x 16]
        double* B2 = sm + 2 * GT * GK;  // [2][128 x 16]
        // (inline asm: hipcc drains vmcnt(0) before the next LDS read of ANY buffer when it sees the builtin in
        // flight; the loads are therefore hidden from it and waited for by hand right before the barrier)
        const unsigned ldsA = (unsigned)(size_t)(lds_ptr)A2, ldsB = (unsigned)(size_t)(lds_ptr)B2;
        auto glds16 = [&](const double* sbase, unsigned voff, unsigned lds_dst) {
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(voff), "s"(sbase), "s"(lds_dst)
                         : "memory");
        };
        auto gload = [&](int kt, int buf) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const unsigned off = (unsigned)(buf * GT * GK + (16 * w + 8 * q) * GK) * 8u;
                glds16(sf_uniform_ptr(Abase + kt * GK), Aoff[q], ldsA + off);
                glds16(sf_uniform_ptr(Bbase + kt * GK), Boff[q], ldsB + off);
            }
        };
        auto gwait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
        const int nk_all = k0 / GK;
        // band: the K loop starts at the first column where both operands can be non-zero (a band slab's own rows;
        // for the dense border rows the panel's rows decide -- what lies left of that was never even written)
        const int klo = g.kband ? min(max((row0 < g.nband ? row0 : k0) - g.kband, 0) / GK, nk_all) : min(g.fp / GK, nk_all);
        const int nk_lim = (MODE == 1 && tk.kstop > 0) ? min(tk.kstop, nk_all) : nk_all;
        const int kbeg = MODE == 1 ? min(klo + sp * tk.kchunk, nk_lim) : (MODE == 3 ? min(max(tk.ktail, klo), nk_all) : klo);
        const int kend = MODE == 1 ? min(kbeg + tk.kchunk, nk_lim) : (MODE == 2 ? kbeg : nk_all);
        const int nk = kend - kbeg;
        if (nk > 0) gload(kbeg, 0);

        bool generate = false;
        if (g.tilemap) generate = !g.tilemap[(int64_t)b * g.nt128 * g.nt128 + (row0 / GT) * g.nt128 + k0 / GT];
        if (MODE == 2 || (MODE == 3 && tk.ksplit > 0)) {
            // the partial sums of the split-K workgroups, added in split order
            const double* P = tk.part + (int64_t)tile * tk.ksplit * (GT * GT);
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = (sf_d4){0.0, 0.0, 0.0, 0.0};
            // Partial tiles are stored in ACCUMULATOR order -- element (mi, ni, r) of thread t at (((mi TN + ni) 2 + r / 2) 512 + t) 2
            // + r % 2 -- so that a lane reads its values as 16-byte loads, a wave instruction covers 1 KB, and eight loads are
            // in flight per wait: in the tile's row-major layout hipcc (at the 128-VGPR limit, one temporary) waited for every
            // single 8-byte load -- 256 load latencies in series, 125-180 us of the chain task's ~250 at eight partial sums.
            const double2* P2 = (const double2*)P;
            for (int q = 0; q < tk.ksplit; ++q) {
                const double2* Pq = P2 + (int64_t)q * (GT * GT / 2) + tid;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
                    double2 t[2 * TN];
#pragma unroll
                    for (int j = 0; j < 2 * TN; ++j) t[j] = Pq[(mi * 2 * TN + j) * 512];
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        acc[mi][ni][0] += t[2 * ni].x;
                        acc[mi][ni][1] += t[2 * ni].y;
                        acc[mi][ni][2] += t[2 * ni + 1].x;
                        acc[mi][ni][3] += t[2 * ni + 1].y;
                    }
                }
            }
        } else if (MODE == 1 && sp > 0) {
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = (sf_d4){0.0, 0.0, 0.0, 0.0};
        } else if (generate) {
            const double* Yb = g.genY + (int64_t)b * g.sY;
            const int gr = row0 + wm * (16 * TM) + l15;
            const int gc = k0 + wn * (16 * TN) + l15;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = (sf_d4){0.0, 0.0, 0.0, 0.0};
            for (int kk = 0; kk < g.mpad; kk += 4) {
                const double* yk = Yb + (int64_t)(kk + lq) * g.ldy;
                double ya[TM], yb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) ya[i] = yk[min(gr + i * 16, g.ldy + g.fp - 1)];
#pragma unroll
                for (int i = 0; i < TN; ++i) yb[i] = gc + i * 16 >= cfp ? yk[min(gc + i * 16, g.ldy + g.fp - 1)] : 0.0;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[mi], yb[ni], acc[mi][ni], 0, 0, 0);
            }
        } else {
            const double* Cin = Cb + (int64_t)row0 * g.lda + k0;
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    const int col = wn * (16 * TN) + ni * 16 + l15;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = wm * (16 * TM) + mi * 16 + lq + 4 * r;
                        double v = 0.0;
                        if (row < rows_here && col < pw && col >= cfp) v = Cin[(int64_t)row * g.lda + col];
                        acc[mi][ni][r] = v;
                    }
                }
        }
#ifdef SF_TUNING
        if (tk.stamps && tid == 0) tk.stamps[4] = wall_clock64();  // (issue point of the last partial-sum loads)
#endif
        gwait();
        __syncthreads();
        // (the accumulators come from compiler-counted loads: consume them here, so that hipcc places its own
        // vmcnt(0) for them BEFORE the loop and not inside it, where it would also drain the hand-counted prefetch)
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(acc[mi][ni][r]));
#ifdef SF_TUNING
        if (tk.stamps && tid == 0) tk.stamps[5] = wall_clock64();  // (partial sums added, first operand slab landed)
#endif
        // fragment reads: lane (l15, lq) takes the two granules 2 lq, 2 lq + 1 of its row = the four consecutive
        // k = 4 lq .. 4 lq + 3; MFMA j of a slab uses element j of every lane, i.e. slice lq of instruction j stands
        // for k = 4 lq + j -- in both operands (K is a summation index)
        // (a wave whose 32 rows lie beyond the matrix -- the last slab of an order that is not a multiple of 128,
        // e.g. 3008 = 23.5 slabs -- leaves the matrix core to the other waves: its tile is never stored.  cfg 3:
        // 5 % of the long-K MFMA work, 5650 -> 5940 order-evals/s)
        const bool wave_live = wm * (16 * TM) < rows_here;
        auto compute = [&](int cur) {
            const double* Ab = A2 + cur * GT * GK;
            const double* Bb = B2 + cur * GT * GK;
            if (!wave_live) return;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                double2 a[TM], bb[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int row = wm * (16 * TM) + i * 16 + l15;
                    a[i] = *(const double2*)(Ab + row * GK + 2 * ((2 * lq + h) ^ sf_swz(row)));
                }
#pragma unroll
                for (int i = 0; i < TN; ++i) {
                    const int row = wn * (16 * TN) + i * 16 + l15;
                    bb[i] = *(const double2*)(Bb + row * GK + 2 * ((2 * lq + h) ^ sf_swz(row)));
                }
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) {
                        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].x, bb[ni].x, acc[mi][ni], 0, 0, 1);  // neg:[1,0,0]
                        acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi].y, bb[ni].y, acc[mi][ni], 0, 0, 1);
                    }
            }
        };
        for (int kt = 0; kt + 1 < nk; ++kt) {
            gload(kbeg + kt + 1, (kt & 1) ^ 1);
            compute(kt & 1);
            gwait();
            __syncthreads();
        }
        if (nk > 0) compute((nk - 1) & 1);
        __syncthreads();  // the epilogue re-uses the LDS with its own layouts
        if (MODE == 1) {
            double2* P2 = (double2*)(tk.part + ((int64_t)tile * tk.ksplit + sp) * (GT * GT)) + tid;  // (accumulator order: see MODE 2)
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni) {
                    P2[((mi * TN + ni) * 2 + 0) * 512] = make_double2(acc[mi][ni][0], acc[mi][ni][1]);
                    P2[((mi * TN + ni) * 2 + 1) * 512] = make_double2(acc[mi][ni][2], acc[mi][ni][3]);
                }
            return;
        }

        // (dataflow sequence: the long-K loop above did not need the diagonal tile's factor; everything below does)
#ifdef SF_TUNING
        if (tk.stamps && tid == 0) tk.stamps[0] = wall_clock64();
#endif
        if (tk.wflag && !sf_df_wait(tk.wflag, tk.wval, tk.abort_flag, tid, tk.lds_int)) return;
#ifdef SF_TUNING
        if (tk.stamps && tid == 0) tk.stamps[1] = wall_clock64();
#endif
        // ---------------------------------------------------------------- 2: L = T W through LDS
        const int nsb = pw >> 4;  // 16-column blocks of the panel (4 or 8)
        const double* Wp[2];
#pragma unroll
        for (int p = 0; p < 2; ++p)
            Wp[p] = tk.Wt + (int64_t)b * tk.sW + (int64_t)min(lr + 64 * p, pw - 1) * SF_LDT + lc;
        double2 rw[2];
        auto wload = [&](int sb) {
#pragma unroll
            for (int p = 0; p < 2; ++p) rw[p] = *(const double2*)(Wp[p] + sb * 16);
        };
        auto wstore = [&](int buf) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                double* pb = &Bs[buf][(lr + 64 * p) * GLD + lc];
                pb[0] = rw[p].x;
                pb[1] = rw[p].y;
            }
        };
        // dump the two 16-column blocks of chunk q that this wave owns (accumulator -> operand layout)
        auto dump = [&](int q, bool zero) {
            if (wn != (q >> 1)) return;
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    if (half != (q & 1)) continue;
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            Ach[(wm * (16 * TM) + mi * 16 + lq + 4 * r) * CLD + nn * 16 + l15] = acc[mi][2 * half + nn][r];
                        if (zero) acc[mi][2 * half + nn] = (sf_d4){0.0, 0.0, 0.0, 0.0};
                    }
                }
        };
        if (nsb > 0) wload(nsb - 1);
        int buf = 0;
        // (fully unrolled: chunk and block indices are compile-time constants, only wave-uniform branches remain)
#pragma unroll
        for (int sbi = 0; sbi < GT / 16; ++sbi) {
            const int sb = GT / 16 - 1 - sbi;
            if (sb >= nsb) continue;  // narrow last panel
            if (sb & 1) {  // first block of chunk sb / 2 in descending order
                __syncthreads();  // everybody is done with the previous contents of the chunk buffer / As
                dump(sb >> 1, true);
            }
            wstore(buf);
            __syncthreads();
            if (sb > 0) wload(sb - 1);
            // W[k][c] = 0 for k > c: this wave's 64 columns need the blocks k <= 4 wn + 3 only (one wave-uniform
            // branch around a straight-line body; inside it the zero blocks of W are multiplied through, which
            // leaves the not-yet-dumped T blocks and the finished sums bit-for-bit unchanged.  Skipping block by
            // block -- a switch over four straight-line bodies -- makes hipcc spill ~250 VGPRs: measured, not kept)
            if (sb <= wn * TN + (TN - 1) && wave_live) {
                const double* Ab = &Ach[(wm * (16 * TM) + l15) * CLD + (sb & 1) * 16 + lq];
                const double* Bb = &Bs[buf][(wn * (16 * TN) + l15) * GLD + lq];
                sf_solve_step<0>(acc, Ab, Bb);
            }
            buf ^= 1;
        }

        // ---------------------------------------------------------------- 3: L in place, rhs -= L z
        double* Lout = Cb + (int64_t)row0 * g.lda + k0;
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) {
                const int col = wn * (16 * TN) + ni * 16 + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wm * (16 * TM) + mi * 16 + lq + 4 * r;
                    if (row < rows_here && col < pw && col >= cfp) Lout[(int64_t)row * g.lda + col] = acc[mi][ni][r];
                }
            }
        if (tk.top_flag) {
            // dataflow chain task: the slab's row is final HERE -- the next chain task's K work reads L, not the diagonal tile
            // that step 4 updates and parks for this workgroup's own D(k) -- so it is published before step 4, not after it
            __syncthreads();
            if (tid == 0) {
                sf_df_release();
                sf_df_set(tk.top_flag, tk.top_val);
#ifdef SF_TUNING
                if (tk.stamps) tk.stamps[2] = wall_clock64();
#endif
            }
        }
        if (RHS && g.rhs) {
            const double* z = g.rhs + (int64_t)b * g.ldr + k0;
            double zc[TN];
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) {
                const int col = wn * (16 * TN) + ni * 16 + l15;
                zc[ni] = (col < pw && col >= cfp) ? z[col] : 0.0;
            }
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double v = 0.0;
#pragma unroll
                    for (int ni = 0; ni < TN; ++ni) v = __builtin_fma(acc[mi][ni][r], zc[ni], v);
                    v += __shfl_xor(v, 1);
                    v += __shfl_xor(v, 2);
                    v += __shfl_xor(v, 4);
                    v += __shfl_xor(v, 8);
                    if (l15 == 0) red[wn][wm * (16 * TM) + mi * 16 + lq + 4 * r] = v;
                }
        }
    }

    // -------------------------------------------------------------------- 4: S = C[slab, slab] - L L^T
    // The L slab just stored is read back (L2) through the ordinary operand staging -- the accumulators are free
    // by now, so the 36 lower blocks fit one pass of 5 + 4 blocks per wave pair (see sf_syrk_diag_tile); keeping
    // L in registers and dumping it chunk by chunk needed two passes and 16 barriers.
    {
        const int p = w >> 1, h = w & 1;
        int bi[5], bj[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            if (h == 0) {
                bi[q] = 7 - p;
                bj[q] = q;
            } else {
                const int n_hi = 3 - p;  // blocks 5 .. 7-p of row 7-p, then blocks 0 .. p of row p
                const int qq = q < 4 ? q : 0;
                bi[q] = qq < n_hi ? 7 - p : p;
                bj[q] = qq < n_hi ? 5 + qq : qq - n_hi;
            }
        }
        const int nstore = h == 0 ? 5 : 4;
        const int nk2 = pw / GK;
        const int lr = tid >> 3, lc = (tid & 7) * 2;
        const double* Lp[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) Lp[q] = Cb + (int64_t)(row0 + min(lr + 64 * q, rows_here - 1)) * g.lda + k0 + lc;
        double2 rl[2];
        auto gload2 = [&](int kt) {
#pragma unroll
            for (int q = 0; q < 2; ++q) rl[q] = kt * GK + lc >= cfp ? *(const double2*)(Lp[q] + kt * GK) : make_double2(0.0, 0.0);
        };
        auto lstore2 = [&](int buf) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                double* pa = &As[buf][(lr + 64 * q) * GLD + lc];
                pa[0] = rl[q].x;
                pa[1] = rl[q].y;
            }
        };
        // (dataflow front tasks start on the slab's L rows; the slab's diagonal tile -- updated by the step of the previous
        // panel, possibly still running in another workgroup -- is only needed from here on)
        if (tk.sflag && !sf_df_wait(tk.sflag, tk.sval, tk.abort_flag, tid, tk.lds_int)) return;
#ifdef SF_TUNING
        if (tk.stamps && tid == 0) tk.stamps[3] = wall_clock64();
#endif
        __syncthreads();  // the L slab is visible to every wave of the workgroup; the LDS buffers are free
        if (nk2 > 0) gload2(0);
        const double* Sin = Cb + (int64_t)row0 * g.lda + row0;
        sf_d4 acc2[5];
        // (full slabs -- all but the last of a matrix whose order is not a multiple of 128 -- take straight-line loads and
        // stores: behind per-element predicates hipcc put every access into a block of its own and waited for it there,
        // twenty load and eighteen store latencies in series per task)
        const bool full_tile = rows_here == GT && row0 >= g.fp;
        if (full_tile) {
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * bi[q] + lq + 4 * r, col = 16 * bj[q] + l15;
                    acc2[q][r] = Sin[(int64_t)row * g.lda + col];  // (wave pairs with four blocks read a fifth one they never store)
                }
        } else {
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * bi[q] + lq + 4 * r, col = 16 * bj[q] + l15;
                    if (row0 + min(row, col) < g.fp)  // virtual rows / columns of the first tile: identity
                        acc2[q][r] = row == col ? 1.0 : 0.0;
                    else
                        acc2[q][r] = (q < nstore && row < rows_here && col < rows_here) ? Sin[(int64_t)row * g.lda + col] : 0.0;
                }
        }
        if (nk2 > 0) lstore2(0);
        __syncthreads();
        auto compute2 = [&](int cur) {
            const double* S = &As[cur][l15 * GLD + lq];
#pragma unroll
            for (int ks = 0; ks < GK / 4; ++ks) {
#pragma unroll
                for (int q = 0; q < 5; ++q)
                    acc2[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(S[bi[q] * 16 * GLD + ks * 4], S[bj[q] * 16 * GLD + ks * 4],
                                                                   acc2[q], 0, 0, 1);  // neg:[1,0,0]
            }
        };
        for (int kt = 0; kt + 1 < nk2; ++kt) {
            gload2(kt + 1);
            compute2(kt & 1);
            lstore2((kt & 1) ^ 1);
            __syncthreads();
        }
        if (nk2 > 0) compute2((nk2 - 1) & 1);
        const bool parked = tk.Sout && sl == 0;  // (only the first slab of a launch is the next diagonal tile)
        double* So = parked ? tk.Sout + (int64_t)b * g.sS : Cb + (int64_t)row0 * g.lda + row0;
        const int ldo = parked ? g.ldS : g.lda;
        if (full_tile) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * bi[q] + lq + 4 * r, col = 16 * bj[q] + l15;
                    So[(int64_t)row * ldo + col] = acc2[q][r];
                }
            if (nstore == 5) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * bi[4] + lq + 4 * r, col = 16 * bj[4] + l15;
                    So[(int64_t)row * ldo + col] = acc2[4][r];
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                if (q >= nstore) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * bi[q] + lq + 4 * r, col = 16 * bj[q] + l15;
                    if (row < rows_here && col < rows_here) So[(int64_t)row * ldo + col] = acc2[q][r];
                }
            }
        }
    }
    if (RHS && g.rhs && pw > 0) {
        __syncthreads();
        if (tid < rows_here) g.rhs[(int64_t)b * g.ldr + row0 + tid] -= red[0][tid] + red[1][tid];
    }
}

template <bool RHS, int MODE>
__global__ __launch_bounds__(512, 4) void k_chol_panel(sf_panel_args g) {
    __shared__ __attribute__((aligned(16))) double sm[4 * GT * GLD];
    __shared__ double red[2][GT];
    sf_panel_body<RHS, MODE>(g, sf_task_of(g), sf_xcd_remap(blockIdx.x, gridDim.x), sm, red, threadIdx.x);
}
