// The wide panel step: a pair of 128-column panels per launch, sf_panelw_args, sf_panelw_body and its kernel k_chol_panel_w.
// Used by the wide sequence alone (sf_panel_step_w, sf_launch_potrf_v3).
#pragma once
#include "sf_device.h"
#include "sf_chol_tile.h"
#include "sf_chol_panel.h"

// ---------------------------------------------------------------------------------------------
// WIDE fused panel step: a PAIR of 128-column panels [k0, k0 + 256) per launch.  ONE workgroup of 16 waves (1024
// threads, one per CU: 148 KB of LDS, 4 waves per SIMD) owns a 128-row slab and keeps the 128 x 256 tile in its
// accumulators (wave = 32 rows x 64 columns: two 16-column blocks of each panel), so the slab's L[slab, :k0] -- the
// A operand, the stream that comes from HBM -- is read once per 256 columns instead of once per 128: half the HBM
// traffic of the long-K update, three quarters of the L2 -> LDS traffic, half the tile read-modify-writes and half
// the launches of k_chol_panel.  The factorisation is POWER-bound at these batch sizes (profiles/r03_*: the same
// instruction stream with the operands kept in L2 runs 5 % faster at a 5 % higher clock), so traffic is time.
//   1  T  = C[slab, pair] - L[slab, :k0] L[pair rows, :k0]^T      K slabs of 16 through a THREE-stage LDS ring filled
//         by direct global -> LDS loads; the fragments of the next half slab are read before the barrier (the data of
//         slab k+1 is complete one barrier earlier), so no wave waits for LDS after a barrier
//   2a L1 = T1 W_k            (W_k = L_kk^-T, explicit inverse from k_diag_lds; descending 32-column chunks as in
//                              k_chol_panel: a wave dumps its T blocks when its registers become the L accumulators)
//   2b T2 -= L1 L21^T         (L21 = L[panel k+1 rows, panel k columns], left in place by the chain's narrow step)
//   2c L2 = T2 W_k+1
//   3  L -> C in place (the stores are issued under the MFMAs of step 4), rhs[slab] -= L1 z_k + L2 z_k+1
//   4  S  = C[slab, slab] - L L^T (K = 256): L goes from the accumulators into one 128 x 128 LDS image per panel; the 36
//         lower blocks of the tile are spread over the 16 waves (9 per SIMD) and accumulate over both panels in registers
// Same arithmetic as two consecutive k_chol_panel steps; the summation order of 2b differs (natural k order instead
// of the K-permuted fragments), so results agree to rounding, not bit for bit.
#define WST (3 * GT * GK)  // doubles per LDS stage: A 128 x 16, B 256 x 16
static constexpr size_t SF_PANELW_LDS = (3 * WST + 4 * GT) * sizeof(double);
struct sf_panelw_args {
    double* C;
    int64_t sC;
    int lda, n;
    int k0;            // pair columns [k0, k0 + 256), both panels full
    int row0, nslab;   // nslab slabs of 128 rows, the first at row0; the last may be shorter
    int slab_step;     // distance between the slabs of this launch, in slabs (the two slab groups are interleaved)
    const double* Wt0; // [batch] x sW: (L_kk^-1)[c][k], row stride SF_LDT
    const double* Wt1; // ... of panel k + 1
    int64_t sW;
    double* rhs;
    int ldr;
    double* Sout;      // the first slab's updated diagonal tile goes here (next diagonal tile) when non-NULL
    int64_t sS;
    int ldS;
    const double* genY;
    const unsigned char* tilemap;
    int64_t sY;
    int ldy, mpad, nt128;
    int fp;            // shifted frame, see sf_panel_args
#ifdef SF_TUNING
    long long* stamps; // tuning builds (SF_WIDE_STAMPS): 100 MHz wall-clock stamps of the phases of workgroup gridDim.x / 2
#endif
};
#ifdef SF_TUNING
#define SF_W_STAMP(i) do { if (g.stamps && blockIdx.x == gridDim.x / 2 && threadIdx.x == 0) g.stamps[i] = wall_clock64(); } while (0)
#else
#define SF_W_STAMP(i)
#endif

template <bool RHS>
__device__ __forceinline__ void sf_panelw_body(const sf_panelw_args& g, const int id, double* __restrict__ smw, const int tid) {
    constexpr int TM = 2, TN = 4;
    double* red = smw + 3 * WST;  // [4][GT]

    const int b = id / g.nslab;
    const int sl = id - b * g.nslab;
    const int row0 = g.row0 + sl * g.slab_step * GT;
    const int rows_here = min(GT, g.n - row0);
    const int k0 = g.k0;
    const int cfp = k0 == 0 ? g.fp : 0;  // pair columns below cfp are virtual (zero below the diagonal tile)

    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the four waves of a SIMD (w, w + 4, w + 8, w + 12) share a row group and take the four column groups: the
    // triangular phases give the column groups different amounts of work, every SIMD gets the same total
    const int wm = w & 3, wn = w >> 2;
    const int l15 = lane & 15, lq = lane >> 4;
    double* Cb = g.C + (int64_t)b * g.sC;
    // block ni of this wave: columns bc(ni) .. + 16 of the pair (ni 0, 1: panel k; ni 2, 3: panel k + 1)
#define WBC(ni) ((((ni) >> 1) * GT) + wn * 32 + (((ni)&1) * 16))
    const bool wave_live = wm * 32 < rows_here;

    sf_d4 acc[TM][TN];
    SF_W_STAMP(0);
    // ---------------------------------------------------------------- 1: long-K update
    {
        typedef __attribute__((address_space(3))) void* lds_ptr;
        const unsigned lds0 = (unsigned)(size_t)(lds_ptr)smw;
        const int grow = lane >> 3, gpos = lane & 7;
        // 384 rows of 8 granules per stage = 48 groups of 8 rows, three per wave; groups 0-15 are A rows, 16-47 B rows
        // (a wave-uniform base advanced along K by scalar adds + 32-bit lane offsets: see k_chol_panel)
        unsigned soff[3];
        const double* sbase = sf_uniform_ptr(Cb + g.fp);  // (K starts at column fp)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int G = 3 * w + j;
            const bool isA = G < 16;
            const int r = (isA ? G : G - 16) * 8 + grow;
            const int c = gpos ^ sf_swz(r);
            soff[j] = (unsigned)(((int64_t)(isA ? row0 + min(r, rows_here - 1) : k0 + r) * g.lda + 2 * c) * 8);
        }
        auto glds16 = [&](const double* sb, unsigned voff, unsigned lds_dst) {
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(voff), "s"(sb), "s"(lds_dst)
                         : "memory");
        };
        auto gload = [&](int kt, int stage) {
#pragma unroll
            for (int j = 0; j < 3; ++j) glds16(sf_uniform_ptr(sbase + kt * GK), soff[j], lds0 + (unsigned)(stage * WST * 8 + (3 * w + j) * 1024));
        };
        auto gwait = [&]() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };
        const int nk = max(k0 - g.fp, 0) / GK;
        if (nk > 0) gload(0, 0);
        if (nk > 1) gload(1, 1);

        // start of the tile: generated as Y^T Y (never materialised) or read from C, per 128-column half
        bool gen_half[2] = {false, false};
        if (g.tilemap) {
            const unsigned char* tm = g.tilemap + (int64_t)b * g.nt128 * g.nt128 + (row0 / GT) * g.nt128 + k0 / GT;
            gen_half[0] = !tm[0];
            gen_half[1] = !tm[1];
        }
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            if (gen_half[hf]) {
                const double* Yb = g.genY + (int64_t)b * g.sY;
                const int gr = row0 + wm * 32 + l15;
                const int gc = k0 + hf * GT + wn * 32 + l15;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) acc[mi][2 * hf + nn] = (sf_d4){0.0, 0.0, 0.0, 0.0};
                // (two K steps per round trip: mpad = 8 is one round of loads -- the workgroup has the CU to itself, every
                // dependent round trip of the prologue is exposed; the MFMA sequence per accumulator is unchanged)
                for (int kk = 0; kk < g.mpad; kk += 8) {
                    double ya[2][TM], yb[2][2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const double* yk = Yb + (int64_t)(min(kk + 4 * u, g.mpad - 4) + lq) * g.ldy;
#pragma unroll
                        for (int i = 0; i < TM; ++i) ya[u][i] = yk[min(gr + i * 16, g.ldy + g.fp - 1)];
#pragma unroll
                        for (int i = 0; i < 2; ++i) yb[u][i] = gc + i * 16 >= cfp ? yk[min(gc + i * 16, g.ldy + g.fp - 1)] : 0.0;
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        if (kk + 4 * u >= g.mpad) break;
#pragma unroll
                        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                            for (int nn = 0; nn < 2; ++nn)
                                acc[mi][2 * hf + nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[u][mi], yb[u][nn], acc[mi][2 * hf + nn], 0, 0, 0);
                    }
                }
            } else {
                const double* Cin = Cb + (int64_t)row0 * g.lda + k0;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int nn = 0; nn < 2; ++nn) {
                        const int col = WBC(2 * hf + nn) + l15;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = wm * 32 + mi * 16 + lq + 4 * r;
                            acc[mi][2 * hf + nn][r] = (row < rows_here && col >= cfp) ? Cin[(int64_t)row * g.lda + col] : 0.0;
                        }
                    }
            }
        }
        gwait();
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(acc[mi][ni][r]));
        SF_W_STAMP(1);

        // fragment reads (layout and swizzle of k_chol_panel; sf_swz of a fragment row depends on l15 only)
        const int sw = sf_swz(l15);
        const int e0 = 2 * ((2 * lq) ^ sw), e1 = 2 * ((2 * lq + 1) ^ sw);
        const int arow = (wm * 32 + l15) * GK, brow = (GT + wn * 32 + l15) * GK;
        auto frag = [&](int stage, int h, double2(&a)[TM], double2(&bb)[TN]) {
            const double* S = smw + stage * WST + (h ? e1 : e0);
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = *(const double2*)(S + arow + i * 16 * GK);
#pragma unroll
            for (int i = 0; i < TN; ++i) bb[i] = *(const double2*)(S + brow + ((i >> 1) * GT + (i & 1) * 16) * GK);
        };
        // (instructions lo .. hi - 1 of a 16-MFMA burst, in the order  x: (mi, ni) ...,  y: (mi, ni) ...)
        auto mfma_part = [&](const double2(&a)[TM], const double2(&bb)[TN], auto lo_t, auto hi_t) {
            constexpr int lo = decltype(lo_t)::value, hi = decltype(hi_t)::value;
#pragma unroll
            for (int i = lo; i < hi; ++i) {
                const int y = i >> 3, mi = (i >> 2) & 1, ni = i & 3;
                acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(y ? a[mi].y : a[mi].x, y ? bb[ni].y : bb[ni].x, acc[mi][ni], 0, 0, 1);  // neg:[1,0,0]
            }
        };
        typedef std::integral_constant<int, 0> I0;
        typedef std::integral_constant<int, 8> I8;
        typedef std::integral_constant<int, 16> I16;
        double2 a0[TM], b0[TN], a1[TM], b1[TN];
        int s0 = 0, s1 = 1, s2 = 2;  // stages of slab kt, kt + 1, kt + 2
        if (nk > 0 && wave_live) frag(0, 0, a0, b0);
        for (int kt = 0; kt < nk; ++kt) {
            // Order of a slab: the first eight MFMAs (their fragments were read before the barrier) go out BEFORE the slab's
            // loads and fragment reads.  All sixteen waves leave the barrier in step; whatever stands between it and a wave's first
            // MFMA -- three loads with their M0 moves, six LDS reads -- is time in which no wave of the CU feeds the matrix
            // pipes (one workgroup per CU: nobody else does).  Same box, potrf of cfg 2 (ms): loads first 47.1, after 4 / 8 / 12
            // MFMAs 46.7 / 46.5 / 46.55; loads after all sixteen 52.0 (then they no longer land within the slab);
            // profiles/r05_p_wide_k_loop_issue_order_ab.txt.  (s_setprio is a scheduling boundary for hipcc: the order holds.
            // The bursts run at raised priority: a wave with matrix work ready goes before the waves that are still issuing their
            // fragment reads -- cfg 2 48.77 -> 48.53 ms on the same box, three runs each.)
            if (wave_live) {
                __builtin_amdgcn_s_setprio(1);
                mfma_part(a0, b0, I0(), I8());
                __builtin_amdgcn_s_setprio(0);
            }
            if (kt + 2 < nk) gload(kt + 2, s2);
            if (wave_live) {
                frag(s0, 1, a1, b1);
                __builtin_amdgcn_s_setprio(1);
                mfma_part(a0, b0, I8(), I16());
                __builtin_amdgcn_s_setprio(0);
                if (kt + 1 < nk) frag(s1, 0, a0, b0);  // complete since the previous barrier
                __builtin_amdgcn_s_setprio(1);
                mfma_part(a1, b1, I0(), I16());
                __builtin_amdgcn_s_setprio(0);
            }
            gwait();
            __syncthreads();
            const int t = s0;
            s0 = s1;
            s1 = s2;
            s2 = t;
        }
    }

    // ---------------------------------------------------------------- 2: triangular solves through LDS
    // (round 6: the chunk buffers alternate -- a chunk is dumped while the previous one is still being read, so no barrier
    // stands in front of a dump)
    double* Ach0 = smw;                         // [2][128][CLD] chunks of the A operand (accumulator -> operand layout)
    double* Bs = smw + 2 * GT * CLD;            // [2][128][CLD] chunks of W  /  of L21
    const int lr = tid >> 3, lc = (tid & 7) * 2;  // staging: 128 rows x 8 threads, four doubles each
    // L = T W on the blocks NB, NB + 1 of every wave (NB = 0: panel k, NB = 2: panel k + 1), K blocks in descending order.
    // W is staged in 32-row chunks like T and L21 (the K blocks 2 c + 1 and 2 c meet at ONE barrier), and chunk c - 1 is
    // dumped and staged AHEAD of the MFMAs of chunk c: the T blocks its owners hand over are untouched until then, and its
    // buffers ((c - 1) & 1) were last read two chunks ago.  12 barriers in the phases 2a / 2b / 2c instead of 22; per task
    // 10.7 -> 9.3 us (2a), 17.2 -> 16.2 (2b), 12.4 -> 12.0 (2c): profiles/r07_a_wide_fixed_part_ab.txt.
    // (rw[0..1] / rw[2..3]: the chunks 3 and 2 of W, requested by the caller ahead of the phase that precedes the solve: every
    // global round trip of the epilogue -- W, L21, z, the diagonal tile -- is in flight before the phase that needs it: with one
    // workgroup per CU nothing else hides them; 78 -> ~66 us of fixed cost per task, profiles/r05_e_wide_kernel_phases_*.txt)
    auto w_rows = [&](const double* Wt) { return Wt + (int64_t)b * g.sW + (int64_t)lr * SF_LDT + 2 * lc; };
    auto w_chunk = [&](const double* Wp, int c, double2& r0, double2& r1) {
        r0 = *(const double2*)(Wp + c * 32);
        r1 = *(const double2*)(Wp + c * 32 + 2);
    };
    auto stage4 = [&](double* pb, double2 r0, double2 r1) {  // the thread's four doubles of a 128 x 32 chunk (row stride CLD)
        pb[0] = r0.x;
        pb[1] = r0.y;
        pb[2] = r1.x;
        pb[3] = r1.y;
    };
    auto solve = [&](const double* Wt, double2 (&rw)[4], auto nbtag, auto&& ahead) {
        constexpr int NB = decltype(nbtag)::value;
        const double* Wp = w_rows(Wt);
        auto stage = [&](int c, double2 r0, double2 r1) {
            double* Ach = Ach0 + (c & 1) * (GT * CLD);
            if (wn == c) {  // the chunk's owner waves hand their T blocks over
#pragma unroll
                for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            Ach[(wm * 32 + mi * 16 + lq + 4 * r) * CLD + nn * 16 + l15] = acc[mi][NB + nn][r];
                        acc[mi][NB + nn] = (sf_d4){0.0, 0.0, 0.0, 0.0};
                    }
            }
            stage4(Bs + (c & 1) * (GT * CLD) + lr * CLD + 2 * lc, r0, r1);
        };
        // (the phase before this one read the buffers of the other parity last: no barrier in front of the first dump)
        stage(3, rw[0], rw[1]);
        w_chunk(Wp, 1, rw[0], rw[1]);  // (a chunk is requested as soon as its registers are free: two chunks ahead)
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
            const int c = 3 - ci;
            __syncthreads();
            if (c == 3) {
                stage(2, rw[2], rw[3]);
                w_chunk(Wp, 0, rw[2], rw[3]);
            }
            if (c == 2) stage(1, rw[0], rw[1]);
            if (c == 1) {
                stage(0, rw[2], rw[3]);
            }
            if (c <= 1) ahead(c);  // (the caller's requests for the next phase: the W registers are free from here on)
#pragma unroll
            for (int sb = 2 * c + 1; sb >= 2 * c; --sb) {
                // W[k][c] = 0 for k > c: the wave's columns (blocks 2 wn, 2 wn + 1 of the panel) need K blocks <= 2 wn + 1
                if (sb <= 2 * wn + 1 && wave_live) {
                    const double* Ab = Ach0 + (c & 1) * (GT * CLD) + (wm * 32 + l15) * CLD + (sb & 1) * 16 + lq;
                    const double* Bb = Bs + (c & 1) * (GT * CLD) + (wn * 32 + l15) * CLD + (sb & 1) * 16 + lq;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        double a[TM], bb[2];
#pragma unroll
                        for (int i = 0; i < TM; ++i) a[i] = Ab[i * 16 * CLD + ks * 4];
#pragma unroll
                        for (int i = 0; i < 2; ++i) bb[i] = Bb[i * 16 * CLD + ks * 4];
#pragma unroll
                        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                            for (int nn = 0; nn < 2; ++nn)
                                acc[mi][NB + nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], bb[nn], acc[mi][NB + nn], 0, 0, 0);
                    }
                }
            }
        }
    };
    // ---- requested now, used later: the first two chunks of W_k
    double2 rw[4];
    w_chunk(w_rows(g.Wt0), 3, rw[0], rw[1]);
    w_chunk(w_rows(g.Wt0), 2, rw[2], rw[3]);
    __syncthreads();  // (the main loop's last reads of the ring are done)
    SF_W_STAMP(2);
    // 2b's L21 chunks: [128][CLD] beside the A chunk of the OTHER parity ((q & 1) ^ 1: the solves on either side of 2b end and
    // begin with the buffers 0 and 1, so neither phase change needs a barrier of its own)
    const double* L21 = Cb + (int64_t)(k0 + GT + lr) * g.lda + k0 + 2 * lc;
    auto l21 = [&](int q, double2& l0, double2& l1) {
        const bool real = 2 * lc + q * 32 >= cfp;
        l0 = real ? *(const double2*)(L21 + q * 32) : make_double2(0.0, 0.0);
        l1 = real ? *(const double2*)(L21 + q * 32 + 2) : make_double2(0.0, 0.0);
    };
    double2 n0 = make_double2(0.0, 0.0), n1 = n0;
    auto stage_l21 = [&](int q, double2 r0, double2 r1) { stage4(Bs + ((q & 1) ^ 1) * (GT * CLD) + lr * CLD + 2 * lc, r0, r1); };
    solve(g.Wt0, rw, std::integral_constant<int, 0>(), [&](int c) {
        if (c == 1) {
            l21(0, n0, n1);  // (in flight during a chunk of the solve)
        } else {
            stage_l21(0, n0, n1);  // (its buffer was last read by chunk 1 of the solve)
            l21(1, n0, n1);
        }
    });
    SF_W_STAMP(3);

    // 2b: T2 -= L1 L21^T, 32 columns of L1 at a time (chunk q = the blocks of the waves wn == q)
    // (chunk q + 1 is dumped and staged ahead of chunk q's MFMAs, like the solves' chunks)
    {
        auto dump = [&](int q) {  // the owner waves of chunk q hand their L1 blocks over
            double* Ach = Ach0 + ((q & 1) ^ 1) * (GT * CLD);
            if (wn == q) {
#pragma unroll
                for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            Ach[(wm * 32 + mi * 16 + lq + 4 * r) * CLD + nn * 16 + l15] = acc[mi][nn][r];
            }
        };
        dump(0);  // (its L21 chunk went in ahead of the solve's last chunk)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            __syncthreads();
            if (q + 1 < 4) {
                dump(q + 1);
                stage_l21(q + 1, n0, n1);
                if (q + 2 < 4) l21(q + 2, n0, n1);  // (in flight under this chunk's MFMAs)
            }
            // (the second solve's first chunks of W, a chunk of MFMAs or more ahead of their use, once registers are free)
            if (q == 2) w_chunk(w_rows(g.Wt1), 3, rw[0], rw[1]);
            if (q == 3) w_chunk(w_rows(g.Wt1), 2, rw[2], rw[3]);
            if (wave_live) {
                const double* Ab = Ach0 + ((q & 1) ^ 1) * (GT * CLD) + (wm * 32 + l15) * CLD + lq;
                const double* Bb = Bs + ((q & 1) ^ 1) * (GT * CLD) + (wn * 32 + l15) * CLD + lq;
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    double a[TM], bb[2];
#pragma unroll
                    for (int i = 0; i < TM; ++i) a[i] = Ab[i * 16 * CLD + ks * 4];
#pragma unroll
                    for (int i = 0; i < 2; ++i) bb[i] = Bb[i * 16 * CLD + ks * 4];
#pragma unroll
                    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                        for (int nn = 0; nn < 2; ++nn)
                            acc[mi][2 + nn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], bb[nn], acc[mi][2 + nn], 0, 0, 1);  // neg
                }
            }
        }
    }
    SF_W_STAMP(4);
    solve(g.Wt1, rw, std::integral_constant<int, 2>(), [](int) {});
    SF_W_STAMP(5);
    // ---- the slab's diagonal tile (step 4) is requested before the stores of step 3
    constexpr int TLD = 130;
    const int nsb = wn == 0 ? 3 : 2;
    int sbi[3], sbj[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int t = min(wm + 4 * (wn + 4 * j), 35);
        int bi = 0;
        while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
        sbi[j] = bi;
        sbj[j] = t - bi * (bi + 1) / 2;
    }
    sf_d4 acc2[3];
    {
        const double* Sin = Cb + (int64_t)row0 * g.lda + row0;
        if (rows_here == GT) {  // (full slab: straight-line loads -- see k_chol_panel, step 4)
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * sbi[j] + lq + 4 * r, col = 16 * sbj[j] + l15;
                    acc2[j][r] = Sin[(int64_t)row * g.lda + col];  // (a wave with two blocks reads a third one it never stores)
                }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * sbi[j] + lq + 4 * r, col = 16 * sbj[j] + l15;
                    acc2[j][r] = (j < nsb && row < rows_here && col < rows_here) ? Sin[(int64_t)row * g.lda + col] : 0.0;
                }
        }
    }
    double zc[TN] = {0.0, 0.0, 0.0, 0.0};
    if (RHS && g.rhs) {
        const double* z = g.rhs + (int64_t)b * g.ldr + k0;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) zc[ni] = WBC(ni) + l15 >= cfp ? z[WBC(ni) + l15] : 0.0;
    }

    // ---------------------------------------------------------------- 3: L in place, rhs -= L z
    // (the stores of L themselves are issued under the MFMAs of step 4, two per group of eight, each panel's under its own
    // half: the CU's store path takes ~9 us for the 256 KB of a task, and in front of step 4 every wave waited at its first
    // barrier for the last store to be ISSUED -- 5-6 us in the phase stamps; store + step 4 per task 30 -> 23 us,
    // profiles/r07_a_wide_fixed_part_ab.txt.  The MFMA part of a half is at its MFMA time, 8.1 us, with the blocks as they
    // are: no new split of the 36 blocks was built.  Spreading panel k's stores over step 2b, or moving the sums of L z
    // behind the first half's MFMAs, costs registers the compiler takes from scratch: not built.)
    double* Lout = Cb + (int64_t)row0 * g.lda + k0;
    auto store_L = [&](int half, int s) {  // store s = 0 .. 15 of the wave's two blocks of panel k + half
        const int mi = s >> 3, ni = 2 * half + ((s >> 2) & 1), r = s & 3;
        const int row = wm * 32 + mi * 16 + lq + 4 * r, col = WBC(ni) + l15;
        if (row < rows_here && col >= cfp) Lout[(int64_t)row * g.lda + col] = acc[mi][ni][r];
    };
    {
        if (RHS && g.rhs) {
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
                    if (l15 == 0) red[wn * GT + wm * 32 + mi * 16 + lq + 4 * r] = v;
                }
        }
    }

    SF_W_STAMP(6);
    // ---------------------------------------------------------------- 4: S = C[slab, slab] - L L^T, K = 256
    // L is taken from the accumulators through ONE LDS image per panel (Ts, 128 x 128, row stride 130: the operand reads of
    // a wave instruction hit distinct 8-byte banks per half wave), not read back from global memory: the 36 lower blocks
    // of the tile are spread 9 per SIMD (3 + 2 + 2 + 2 over its waves: block t = wm + 4 (wn + 4 j) of the row-major
    // lower-triangular enumeration) and accumulate over both panels in registers -- four barriers, no K-slab staging loop,
    // no cross-wave reduction.
    {
        double* Ts = smw;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            __syncthreads();  // the previous contents of the LDS image are dead
#pragma unroll
            for (int nn = 0; nn < 2; ++nn)
#pragma unroll
                for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        Ts[(wm * 32 + mi * 16 + lq + 4 * r) * TLD + wn * 32 + nn * 16 + l15] = acc[mi][2 * half + nn][r];
            __syncthreads();
#ifdef SF_TUNING
            if (g.stamps) {  // stamps 9 + 3 half ..: dump done | diagonal-tile loads landed | MFMA part done
                SF_W_STAMP(9 + 3 * half);
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(acc2[j][r]));
                SF_W_STAMP(10 + 3 * half);
            }
#endif
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j >= nsb) continue;
                const double* Pa = Ts + (sbi[j] * 16 + l15) * TLD + lq;
                const double* Pb = Ts + (sbj[j] * 16 + l15) * TLD + lq;
#pragma unroll
                for (int u = 0; u < GT / 32; ++u) {
#pragma unroll
                    for (int ks = 8 * u; ks < 8 * u + 8; ++ks)
                        acc2[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(Pa[ks * 4], Pb[ks * 4], acc2[j], 0, 0, 1);  // neg:[1,0,0]
                    if (4 * j + u < 8) {  // (every wave has two blocks at least: eight groups per half, sixteen stores)
                        store_L(half, 2 * (4 * j + u));
                        store_L(half, 2 * (4 * j + u) + 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            SF_W_STAMP(11 + 3 * half);
        }
        SF_W_STAMP(7);
        const bool parked = g.Sout && sl == 0;  // (only the first slab of a launch is the next diagonal tile)
        double* So = parked ? g.Sout + (int64_t)b * g.sS : Cb + (int64_t)row0 * g.lda + row0;
        const int ldo = parked ? g.ldS : g.lda;
        if (rows_here == GT) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * sbi[j] + lq + 4 * r, col = 16 * sbj[j] + l15;
                    So[(int64_t)row * ldo + col] = acc2[j][r];
                }
            if (nsb == 3) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * sbi[2] + lq + 4 * r, col = 16 * sbj[2] + l15;
                    So[(int64_t)row * ldo + col] = acc2[2][r];
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (j >= nsb) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * sbi[j] + lq + 4 * r, col = 16 * sbj[j] + l15;
                    if (row < rows_here && col < rows_here) So[(int64_t)row * ldo + col] = acc2[j][r];
                }
            }
        }
    }
    if (RHS && g.rhs) {
        // (red was written before the barriers of step 4)
        if (tid < rows_here)
            g.rhs[(int64_t)b * g.ldr + row0 + tid] -= (red[tid] + red[GT + tid]) + (red[2 * GT + tid] + red[3 * GT + tid]);
    }
#ifdef SF_TUNING
    if (g.stamps) {
        __syncthreads();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        SF_W_STAMP(8);
    }
#endif
#undef WBC
}
template <bool RHS>
__global__ __launch_bounds__(1024) void k_chol_panel_w(sf_panelw_args g) {
    extern __shared__ __attribute__((aligned(16))) double smw[];
    // (several tasks per workgroup -- the 5-15 us a CU needs to start a 16-wave workgroup with 148 KB of LDS amortised -- measured
    // without any gain at cfg 2 and cfg 3: profiles/r05_h_wide_tasks_per_workgroup_ab.txt)
    sf_panelw_body<RHS>(g, sf_xcd_remap(blockIdx.x, gridDim.x), smw, threadIdx.x);
}
#undef SF_W_STAMP
#undef WST
