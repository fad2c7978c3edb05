// Everything only sequence 1 uses (the unfused sequence of round 1, panels of SF_NB = 256 columns): the MFMA update
// kernel k_gemm_nt with its symmetric diagonal tile, the diagonal-block kernel k_diag_mfma, sf_launch_potrf_v1.
// (sf_debug_cholesky_sequence(1), and the automatic choice for small batches while the persistent kernel is off.)
#pragma once
#include "sf_device.h"
#include "sf_chol_host.h"

// Batched MFMA update  Cout = Cin -/+ A * B^T  on 128 x 128 tiles (v_mfma_f64_16x16x4_f64, 4 waves,
// each 64 x 64 = 4 x 4 MFMA tiles; K staged through LDS in slabs of GK with register prefetch).
// All operands are row-major blocks addressed from their own origin (the host passes pointers already
// offset to the block): A is M x K, B is Nc x K, C is M x Nc.
struct sf_gemm_args {
    const double* A;
    const double* B;
    const double* Cin;  // NULL: start from zero
    double* Cout;
    int64_t sA, sB, sCin, sCout;  // batch strides (doubles)
    int lda, ldb, ldcin, ldcout;
    int M, Nc, K;
    int tri;    // block is diagonal-aligned: skip tiles lying entirely above the diagonal
    int btri;   // B[c][k] == 0 for k > c: column tile tn only needs k < (tn + 1) * GT
    int remap_after, remap_shift;  // output row i >= remap_after is stored at row i + remap_shift
    // fused left-looking right-hand-side update, done by the tiles with tm == tn while B streams by:
    //   rhs[c] -= sum_k B[c][k] * z[k]
    double* rhs;
    const double* z;
    int64_t srhs, sz;
    // block-diagonal mode (diag_blocks > 0): the launch updates diag_blocks independent SF_NB x SF_NB
    // diagonal blocks; block j takes A/B at +j*dA and C at +j*dC (M = Nc = total rows covered)
    int diag_blocks;
    int64_t dA, dC;
    // matrix-free start: if tilemap says this 128 x 128 tile was never materialised, its initial value is
    // Y^T Y (rank-mpad product of the rows/columns of Y) instead of Cin
    const double* genY;
    const unsigned char* tilemap;
    int64_t sY;
    int ldy, mpad, nt128, tm_off, tn_off;
    int mt, nt;
    int no_syrk;  // diagonal tiles through the generic path (the launchers always leave it 0)
};

// Diagonal 128 x 128 tile of a symmetric update C -= P P^T (block-diagonal launches): only the 36 MFMA
// blocks on or below the diagonal are computed, dealt to the 8 waves in equal shares (rows p and 7-p of
// the 8 x 8 block grid hold 9 blocks; one wave takes 5 of them, its partner 4 plus a spare), and the single
// operand P is staged once instead of twice.  40 block products per slab instead of 64.
// Blocks above the diagonal are neither read nor written (nothing references them).
template <bool RHS>
__device__ __forceinline__ void sf_syrk_diag_tile(const sf_gemm_args& g, int b, int row0, double (*As)[GT * GLD]) {
    constexpr int NP = 2, RPP = 64;  // 512 threads (8 waves): two staging passes of 64 rows
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
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

    const int lr = tid >> 3, lc = (tid & 7) * 2;
    const double* Ap[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) Ap[q] = g.A + (int64_t)b * g.sA + (int64_t)(row0 + lr + RPP * q) * g.lda + lc;
    double2 ra[NP];
    const bool do_rhs = RHS && g.rhs;
    const double* zg = do_rhs ? g.z + (int64_t)b * g.sz + lc : nullptr;
    double2 zv = make_double2(0.0, 0.0);
    double part[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) part[q] = 0.0;
    auto gload = [&](int kt) {
#pragma unroll
        for (int q = 0; q < NP; ++q) ra[q] = *(const double2*)(Ap[q] + kt * GK);
        if (RHS && do_rhs) zv = *(const double2*)(zg + kt * GK);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            double* pa = &As[buf][(lr + RPP * q) * GLD + lc];
            pa[0] = ra[q].x;
            pa[1] = ra[q].y;
        }
        if (RHS && do_rhs) {
#pragma unroll
            for (int q = 0; q < NP; ++q) part[q] += ra[q].x * zv.x + ra[q].y * zv.y;
        }
    };
    const int nk = g.K / GK;
    if (nk > 0) gload(0);
    sf_d4 acc[5];
    const double* Cin = g.Cin + (int64_t)b * g.sCin + (int64_t)row0 * g.ldcin + row0;
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[q][r] = Cin[(int64_t)(16 * bi[q] + lq + 4 * r) * g.ldcin + 16 * bj[q] + l15];
    if (nk > 0) lstore(0);
    __syncthreads();
    auto compute = [&](int cur) {
        const double* S = &As[cur][l15 * GLD + lq];
#pragma unroll
        for (int ks = 0; ks < GK / 4; ++ks) {
#pragma unroll
            for (int q = 0; q < 5; ++q)
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(S[bi[q] * 16 * GLD + ks * 4], S[bj[q] * 16 * GLD + ks * 4],
                                                              acc[q], 0, 0, 1);  // blgp 1 = neg:[1,0,0]: -A B + C
        }
    };
    for (int kt = 0; kt + 1 < nk; ++kt) {
        gload(kt + 1);
        compute(kt & 1);
        lstore((kt & 1) ^ 1);
        __syncthreads();
    }
    if (nk > 0) compute((nk - 1) & 1);
    double* Cout = g.Cout + (int64_t)b * g.sCout + (int64_t)row0 * g.ldcout + row0;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        if (q >= nstore) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            Cout[(int64_t)(16 * bi[q] + lq + 4 * r) * g.ldcout + 16 * bj[q] + l15] = acc[q][r];
    }
    if (RHS && do_rhs) {
        double* rhs = g.rhs + (int64_t)b * g.srhs + row0;
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            double v = part[q];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            if ((tid & 7) == 0) rhs[lr + RPP * q] -= v;
        }
    }
}

// Occupancy note (measured on MI355X, tools/probes/mfma_clock.hip): ONE wave issues a
// v_mfma_f64_16x16x4_f64 only every ~140 cycles even with independent accumulators, two waves per
// SIMD reach one per ~100 cycles, four waves per SIMD saturate the 64-cycle pipe.  The kernel is
// therefore built for 4 waves/SIMD: 512 threads (8 waves, each 32 x 64 of the 128 x 128 tile = 2 x 4
// MFMA tiles = 64 accumulator VGPRs), <= 128 VGPRs, two workgroups per CU.
template <bool NEG, bool RHS>
__global__ __launch_bounds__(512, 4) void k_gemm_nt(sf_gemm_args g) {
    constexpr int TM = 2, TN = 4;
    constexpr int WN = 128 / (16 * TN);   // waves across columns
    constexpr int NP = 2;                 // staging passes of 64 rows each
    constexpr int RPP = 64;               // rows per staging pass
    __shared__ __attribute__((aligned(16))) double As[2][GT * GLD];
    __shared__ __attribute__((aligned(16))) double Bs[2][GT * GLD];

    const int id = sf_xcd_remap(blockIdx.x, gridDim.x);
    const int tiles = g.mt * g.nt;
    const int b = id / tiles;
    const int t = id - b * tiles;
    int tm, tn, rows_here, cols_here;
    if (g.diag_blocks) {
        // 2 x 2 tiles per SF_NB block, the upper-right one is never needed
        const int jb = t >> 2;
        tm = (t >> 1) & 1;
        tn = t & 1;
        if (tn > tm) return;
        const int blk = min(SF_NB, g.M - jb * SF_NB);  // the last block may be narrower
        rows_here = min(GT, blk - tm * GT);
        cols_here = min(GT, blk - tn * GT);
        if (rows_here <= 0 || cols_here <= 0) return;
        g.A += jb * g.dA;
        g.B += jb * g.dA;
        if (g.Cin) g.Cin += jb * g.dC;
        g.Cout += jb * g.dC;
        if (RHS && g.rhs) g.rhs += jb * SF_NB;
        if (NEG && tm == tn && rows_here == GT && g.K > 0 && g.A == g.B && g.Cin && !g.no_syrk) {
            sf_syrk_diag_tile<RHS>(g, b, tm * GT, As);
            return;
        }
    } else {
        tm = t / g.nt;
        tn = t - tm * g.nt;
        if (g.tri && tn * GT > tm * GT + GT - 1) return;
        rows_here = min(GT, g.M - tm * GT);
        cols_here = min(GT, g.Nc - tn * GT);
    }
    const int row0 = tm * GT, col0 = tn * GT;
    const int Kt = g.btri ? min(g.K, col0 + GT) : g.K;

    const int tid = threadIdx.x;
    const int lane = tid & 63, w = tid >> 6;
    const int wm = w / WN, wn = w % WN;  // rows wm*32.., cols wn*(16*TN)..
    const int l15 = lane & 15, lq = lane >> 4;

    // ---- global -> register -> LDS staging: thread covers rows lr+64p, two doubles at column lc.
    // Rows past the block edge are CLAMPED to the last valid row instead of being predicated: the
    // duplicated data only feeds accumulator rows / columns that are never stored, and the loads stay
    // branch-free (a predicated load makes hipcc wait for the whole vm queue).
    const int lr = tid >> 3, lc = (tid & 7) * 2;
    const double* Ap[NP];
    const double* Bp[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        Ap[p] = g.A + (int64_t)b * g.sA + (int64_t)(row0 + min(lr + RPP * p, rows_here - 1)) * g.lda + lc;
        Bp[p] = g.B + (int64_t)b * g.sB + (int64_t)(col0 + min(lr + RPP * p, cols_here - 1)) * g.ldb + lc;
    }
    double2 ra[NP], rb[NP];
    const bool do_rhs = RHS && g.rhs && (tm == tn);
    const double* zg = do_rhs ? g.z + (int64_t)b * g.sz + lc : nullptr;
    double2 zv = make_double2(0.0, 0.0);
    double part[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) part[p] = 0.0;

    auto gload = [&](int kt) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            ra[p] = *(const double2*)(Ap[p] + kt * GK);
            rb[p] = *(const double2*)(Bp[p] + kt * GK);
        }
        if (RHS && do_rhs) zv = *(const double2*)(zg + kt * GK);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            double* pa = &As[buf][(lr + RPP * p) * GLD + lc];
            double* pb = &Bs[buf][(lr + RPP * p) * GLD + lc];
            pa[0] = ra[p].x;
            pa[1] = ra[p].y;
            pb[0] = rb[p].x;
            pb[1] = rb[p].y;
        }
        if (RHS && do_rhs) {
#pragma unroll
            for (int p = 0; p < NP; ++p) part[p] += rb[p].x * zv.x + rb[p].y * zv.y;
        }
    };

    // the first operand slab is requested before the accumulators are initialised so that both
    // latencies overlap (matters for the short-K launches)
    const int nk = Kt / GK;
    if (nk > 0) gload(0);

    // ---- accumulators start as the C tile (read, or generated from Y when it was never materialised)
    sf_d4 acc[TM][TN];
    const double* Cin = g.Cin ? g.Cin + (int64_t)b * g.sCin + (int64_t)row0 * g.ldcin + col0 : nullptr;
    bool generate = false;
    if (g.tilemap && !g.diag_blocks)
        generate = !g.tilemap[(int64_t)b * g.nt128 * g.nt128 + (g.tm_off + tm) * g.nt128 + (g.tn_off + tn)];
    if (generate) {
        const double* Yb = g.genY + (int64_t)b * g.sY;
        // global pixel index of this lane's row / column (clamped: Y has ldy columns; rows past the
        // matrix edge are never stored)
        const int gr = (g.tm_off + tm) * GT + wm * (16 * TM) + l15;
        const int gc = (g.tn_off + tn) * GT + wn * (16 * TN) + l15;
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) acc[mi][ni] = (sf_d4){0.0, 0.0, 0.0, 0.0};
        for (int kk = 0; kk < g.mpad; kk += 4) {
            const double* yk = Yb + (int64_t)(kk + lq) * g.ldy;
            double ya[TM], yb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) ya[i] = yk[min(gr + i * 16, g.ldy - 1)];
#pragma unroll
            for (int i = 0; i < TN; ++i) yb[i] = yk[min(gc + i * 16, g.ldy - 1)];
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[mi], yb[ni], acc[mi][ni], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int ni = 0; ni < TN; ++ni) {
                const int col = wn * (16 * TN) + ni * 16 + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wm * (16 * TM) + mi * 16 + lq + 4 * r;
                    double v = 0.0;
                    if (Cin && row < rows_here && col < cols_here) v = Cin[(int64_t)row * g.ldcin + col];
                    acc[mi][ni][r] = v;
                }
            }
    }

    if (nk > 0) lstore(0);
    __syncthreads();

    auto compute = [&](int cur) {
        const double* Ab = &As[cur][(wm * (16 * TM) + l15) * GLD + lq];
        const double* Bb = &Bs[cur][(wn * (16 * TN) + l15) * GLD + lq];
#pragma unroll
        for (int ks = 0; ks < GK / 4; ++ks) {
            double a[TM], bb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = Ab[i * 16 * GLD + ks * 4];
#pragma unroll
            for (int i = 0; i < TN; ++i) bb[i] = Bb[i * 16 * GLD + ks * 4];
#pragma unroll
            for (int mi = 0; mi < TM; ++mi)
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], bb[ni], acc[mi][ni], 0, 0, NEG ? 1 : 0);  // the f64 MFMA's blgp bits negate: neg:[1,0,0]
        }
    };
    // steady state is ONE basic block: issue the next slab's global loads, run this slab's MFMAs from
    // LDS, then park the loaded slab in the other LDS buffer; the last slab is peeled
    for (int kt = 0; kt + 1 < nk; ++kt) {
        gload(kt + 1);
        compute(kt & 1);
        lstore((kt & 1) ^ 1);
        __syncthreads();
    }
    if (nk > 0) compute((nk - 1) & 1);

    double* Cout = g.Cout + (int64_t)b * g.sCout + col0;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi)
#pragma unroll
        for (int ni = 0; ni < TN; ++ni) {
            const int col = wn * (16 * TN) + ni * 16 + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wm * (16 * TM) + mi * 16 + lq + 4 * r;
                if (row < rows_here && col < cols_here) {
                    int orow = row0 + row;
                    if (orow >= g.remap_after) orow += g.remap_shift;
                    Cout[(int64_t)orow * g.ldcout + col] = acc[mi][ni][r];
                }
            }
        }

    if (RHS && do_rhs) {
        // the 8 threads sharing lr cover the 16 k-columns of a slab: fold them, one of them commits
        double* rhs = g.rhs + (int64_t)b * g.srhs + col0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            double v = part[p];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            const int rr = lr + RPP * p;
            if ((tid & 7) == 0 && rr < cols_here) rhs[rr] -= v;
        }
    }
}

// ------------------------------------------------------------------------------------ launchers
static int launch_gemm(sf_gemm_args g, int batch, bool neg, double flops, hipStream_t s) {
    if (g.M <= 0 || g.Nc <= 0) return SF_OK;
    g.mt = (g.M + GT - 1) / GT;
    g.nt = (g.Nc + GT - 1) / GT;
    if (g.diag_blocks) {  // 4 tile slots per block
        g.mt = g.diag_blocks;
        g.nt = 4;
    }
    const long long nblk = (long long)g.mt * g.nt * batch;
    if (nblk > 0x7fffffffLL) {
        sf_set_error("gemm grid too large");
        return SF_EINVAL;
    }
    void* tok;
    sf_prof_gemm_begin(s, flops, &tok);
    if (g.rhs)
        hipLaunchKernelGGL((k_gemm_nt<true, true>), dim3((unsigned)nblk), dim3(512), 0, s, g);
    else if (neg)
        hipLaunchKernelGGL((k_gemm_nt<true, false>), dim3((unsigned)nblk), dim3(512), 0, s, g);
    else
        hipLaunchKernelGGL((k_gemm_nt<false, false>), dim3((unsigned)nblk), dim3(512), 0, s, g);
    sf_prof_gemm_end(tok);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Panel scratch T (per matrix, row stride SF_LDT): rows [0, pw) the updated diagonal block,
// rows [pw, 2pw) the rows of W = L_kk^-T while the diagonal block is factored (k_diag_mfma),
// rows [2pw, ...) the updated rows below the diagonal block.

// ---------------------------------------------------------------------------------------------
// Diagonal-block step of one panel as ONE launch on the matrix cores (one workgroup of 16 waves per
// matrix, one 16 x 16 block of the current block column per wave): L_kk and its inverse for the pw x pw block (pw <= 256), LEFT-looking over 16-column block
// columns so that nothing is read-modify-written in memory:
//   U  every wave accumulates its blocks of column k in registers:  M(i,k) - sum_{j<k} L(i,j) L(k,j)^T
//      for the rows of the matrix block and  - sum_{e<=j<k} X(e,j) L(k,j)^T  for the rows of the "identity
//      block" E (whose solved rows X = rows of W = L_kk^-T).  A operands stream from L2, the row L(k,:)
//      shared by the whole column is staged in LDS once;
//   P  wave 0, which owns M(k,k), factorises it and inverts the factor in the MFMA accumulator layout
//      (column j of the symmetric block is register j/4 of quarter j%4 = a K-slice of the MFMA operands,
//      so every rank-1 elimination is one MFMA without data movement; pivots from scalars so that the
//      rsqrt chain overlaps the matrix core);
//   X  every wave solves the blocks it still holds as a product with the 16 x 16 inverse F and writes
//      them out: L to the matrix (and in place, as operand of later columns), W transposed to Wt.
// The identity block is implicit (row block e of E starts at column e with X = F^T).  Finally
// z_k = L_kk^-1 r_k as a product with the explicit inverse.  One launch per panel: one scheduling wait on the
// contended chip.
__global__ __launch_bounds__(1024) void k_diag_mfma(double* __restrict__ T, int64_t sT, int pw,
                                                      int* __restrict__ info, int info_off,
                                                      double* __restrict__ rhs, int ldr,
                                                      double* __restrict__ Cdiag, int ldc, int64_t sC,
                                                      double* __restrict__ Wt, int64_t sW) {
    constexpr int NT = 1024;  // 16 waves
    __shared__ double LK[(NT / 64 - 1) * DBS];  // L(k, j), j < k: the B operand of the whole block column
    __shared__ double ST[(NT / 64) * DBS];      // per-wave staging block (accumulator layout -> operand layout)
    __shared__ double Fb[DBS];       // inverse of the current 16 x 16 diagonal factor
    __shared__ double rz[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int nb = pw >> 4;
    double* Tb = T + (int64_t)b * sT;
    double* Eb = Tb + (int64_t)pw * SF_LDT;
    double* Cb = Cdiag + (int64_t)b * sC;
    double* Wb = Wt + (int64_t)b * sW;
    double* st = ST + wave * DBS;

    // Wt is lower triangular: zero the blocks above the diagonal (the buffer alternates between panels)
    for (int e = tid; e < nb * nb * 256; e += NT) {
        const int blk = e >> 8, bc = blk / nb, be = blk - bc * nb;
        if (be > bc) Wb[(int64_t)(bc * 16 + ((e >> 4) & 15)) * SF_LDT + be * 16 + (e & 15)] = 0.0;
    }
    int bad = 0;
    for (int k = 0; k < nb; ++k) {
        const int m = nb - 1 - k;  // matrix row blocks below the diagonal block
        // ---- stage L(k, 0..k-1) (final since the previous columns) in LDS
        for (int e = tid; e < k * 256; e += NT) {
            const int j = e >> 8, r = (e >> 4) & 15, cc = e & 15;
            LK[j * DBS + r * DLD + cc] = Tb[(int64_t)(16 * k + r) * SF_LDT + 16 * j + cc];
        }
        __syncthreads();
        // ---- U: block of this wave: t = 0 -> M(k,k), 1..m -> M(k+t,k), then E(e,k)
        sf_d4 acc[1];
        int kind[1];  // 0 none, 1 matrix row block, 2 inverse row block
        int ibk[1];
        {
            constexpr int u = 0;
            const int t = wave;
            kind[u] = 0;
            ibk[u] = 0;
            acc[u] = (sf_d4){0.0, 0.0, 0.0, 0.0};
            if (t <= m + k) {
                const bool isM = t <= m;
                const int ib = isM ? k + t : t - m - 1;
                kind[u] = isM ? 1 : 2;
                ibk[u] = ib;
                const double* rowp = (isM ? Tb : Eb) + (int64_t)(16 * ib) * SF_LDT;
                if (isM) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = lq + 4 * r;
                        // the diagonal block is read symmetrically from its lower triangle
                        acc[u][r] = (t == 0) ? rowp[(int64_t)max(row, l15) * SF_LDT + 16 * k + min(row, l15)]
                                             : rowp[(int64_t)row * SF_LDT + 16 * k + l15];
                    }
                }
                const int j0 = isM ? 0 : ib;  // X(e, j) exists for j >= e
                // K is a summation index: lane (l15, lq) takes the four CONTIGUOUS columns 4 lq .. 4 lq + 3
                // of its row (two 16-byte loads, full 128-B lines per 4 lanes) and MFMA kk uses element kk, i.e.
                // slice lq of instruction kk stands for k = 4 lq + kk -- in both operands.
                const double2* ap = (const double2*)(rowp + (int64_t)l15 * SF_LDT + 4 * lq);
                // A fragments stream from L2: four block columns in flight (clamped loads past the end)
                double2 av[4][2];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int jj = min(j0 + d, max(k - 1, 0));
                    av[d][0] = ap[8 * jj];
                    av[d][1] = ap[8 * jj + 1];
                }
                for (int j = j0; j < k; ++j) {
                    // rotating register window: block column j is consumed, j + 4 is requested
                    const double* lk = LK + j * DBS + l15 * DLD + 4 * lq;
                    const double a4[4] = {av[0][0].x, av[0][0].y, av[0][1].x, av[0][1].y};
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a4[kk], lk[kk], acc[u], 0, 0, 1);  // neg:[1,0,0]
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        av[d][0] = av[d + 1][0];
                        av[d][1] = av[d + 1][1];
                    }
                    const int jj = min(j + 4, max(k - 1, 0));
                    av[3][0] = ap[8 * jj];
                    av[3][1] = ap[8 * jj + 1];
                }
            }
        }
        // ---- P: wave 0 holds the updated diagonal block in acc[0]
        if (wave == 0) {
            sf_d4 a0 = acc[0], f, lt;
            double pkeep;
            SF_POTRF16_ACC(a0, lane, l15, lq, f, lt, pkeep);
            const unsigned long long neg = __ballot(lane < 16 && !(pkeep > 0.0));
            if (neg && !bad) bad = 16 * k + __ffsll((long long)neg);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = lq + 4 * r;
                Fb[row * DLD + l15] = f[r];
                Wb[(int64_t)(16 * k + row) * SF_LDT + 16 * k + l15] = f[r];  // diagonal block of L_kk^-1
                // X of the identity row block k is F^T: operand of later columns
                Eb[(int64_t)(16 * k + l15) * SF_LDT + 16 * k + row] = f[r];
                if (l15 >= row) {
                    Cb[(int64_t)(16 * k + l15) * ldc + 16 * k + row] = lt[r];          // L[i][j] -> matrix
                    Tb[(int64_t)(16 * k + l15) * SF_LDT + 16 * k + row] = lt[r];        // and in place
                }
            }
            kind[0] = 0;
        }
        __syncthreads();
        // ---- X: solve the blocks still held in registers, write them out
#pragma unroll
        for (int u = 0; u < 1; ++u) {
            if (kind[u] == 0) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) st[(lq + 4 * r) * DLD + l15] = acc[u][r];
            sf_d4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                x = __builtin_amdgcn_mfma_f64_16x16x4f64(st[l15 * DLD + kk * 4 + lq], Fb[l15 * DLD + kk * 4 + lq], x,
                                                         0, 0, 0);
            const int ib = ibk[u];
            double* rowp = (kind[u] == 1 ? Tb : Eb) + (int64_t)(16 * ib) * SF_LDT + 16 * k;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = lq + 4 * r;
                rowp[(int64_t)row * SF_LDT + l15] = x[r];  // in place: operand of the later columns
                if (kind[u] == 1) Cb[(int64_t)(16 * ib + row) * ldc + 16 * k + l15] = x[r];  // L
                else Wb[(int64_t)(16 * k + l15) * SF_LDT + 16 * ib + row] = x[r];             // (L^-T)^T
            }
        }
        __syncthreads();
    }
    if (tid == 0 && bad && info && info[b] == 0) info[b] = info_off + bad;
    // ---- z_k = L_kk^-1 r_k with the explicit inverse
    if (rhs) {
        double* rb = rhs + (int64_t)b * ldr;
        for (int i = tid; i < pw; i += NT) rz[i] = rb[i];
        __syncthreads();
        for (int i = tid; i < pw; i += NT) {
            const double* wrow = Wb + (int64_t)i * SF_LDT;
            double zacc = 0.0;
            for (int j = 0; j <= i; ++j) zacc = __builtin_fma(wrow[j], rz[j], zacc);
            rb[i] = zacc;
        }
    }
}

// Factor each n x n matrix in place (lower), panels of SF_NB columns:
//   Ur  T[below] <- C[k1:, k0:k1] - L[k1:, :k0] L[k0:k1, :k0]^T   LEFT-looking for everything below the
//                                                                diagonal block: C read once, long K
//   R   C[jj] -= L[j-rows, k0:k1] L[j-rows, k0:k1]^T for the future DIAGONAL blocks j > k (RIGHT-looking,
//       K = SF_NB): keeps the next diagonal block ready without a long-K launch of only a few tiles;
//       its diagonal tiles also apply rhs[j-rows] -= L[j-rows, k0:k1] z[k0:k1]
//   D   factor the diagonal block together with an identity block -> L_kk and W = L_kk^-T
//       (k_diag_mfma), L_kk -> matrix, W^T (F)
//   G   C[k1:, k0:k1] <- T[below] W                               MFMA (triangular B)
// With rhs != NULL (batch x ldr) the forward substitution L z = rhs is fused (R and D); z overwrites rhs.
//
// Lookahead (two streams): only the rows of the NEXT diagonal block are on the critical chain.
//   side:  D(k) F(k) | wait Ur(k) | Gt(k) Rnext(k -> k+1) | D(k+1) ...
//   main:  wait Gt(k-1) | Ur(k) | wait F(k) | Gr(k) Rrest(k) | ...
static int sf_launch_potrf_v1(double* A, int n, int lda, int64_t stride, int* info, const sf_potrf_scratch& ws, double* rhs,
                              int ldr, hipStream_t s, const sf_gen_args* gen, sf_exec* ex) {
    const int batch = ws.batch;
    double* T = ws.T;
    const int64_t sT = ws.sT, sW = ws.sW;
    SF_HIP(hipMemsetAsync(info, 0, sizeof(int) * (size_t)batch, s));

    SF_TRY(sf_exec_prepare(ex));
    hipStream_t c = ex->side;  // side ("critical chain") stream
    auto next_event = [&](hipEvent_t* e) { return sf_exec_event(ex, e); };
    hipEvent_t e_gt_prev = nullptr;
    SF_TRY(sf_exec_fork(ex, s, {c}));

    // R: right-looking update of `nblk` future diagonal blocks starting at row/col j0 with panel [k0,k1)
    auto launch_r = [&](int j0, int nrows, int k0, int pw, double* cout, int ldcout, int64_t scout,
                        int64_t dcout, hipStream_t st) -> int {
        sf_gemm_args g = {};
        g.A = g.B = A + (int64_t)j0 * lda + k0;
        g.Cin = A + (int64_t)j0 * lda + j0;
        g.Cout = cout;
        g.sA = g.sB = g.sCin = stride;
        g.sCout = scout;
        g.lda = g.ldb = g.ldcin = lda;
        g.ldcout = ldcout;
        g.M = g.Nc = nrows;
        g.K = pw;
        g.remap_after = 0x7fffffff;
        g.diag_blocks = (nrows + SF_NB - 1) / SF_NB;
        g.dA = (int64_t)SF_NB * lda;
        g.dC = dcout;
        if (rhs && pw > 0) {
            g.rhs = rhs + j0;
            g.z = rhs + k0;
            g.srhs = g.sz = ldr;
        }
        // algorithmic flops: lower triangle of every block
        double useful = 0.0;
        for (int r = 0; r < nrows; r += SF_NB) {
            const double bw = (nrows - r < SF_NB) ? nrows - r : SF_NB;
            useful += 0.5 * bw * (bw + 1);
        }
        return launch_gemm(g, batch, true, 2.0 * pw * useful * batch, st);
    };

    // diagonal block 0 goes to the panel scratch unchanged (K = 0: a copy)
    {
        const int pw0 = n < SF_NB ? n : SF_NB;
        SF_TRY(launch_r(0, pw0, 0, 0, T, SF_LDT, sT, 0, c));
    }
    int panel = 0;
    for (int k0 = 0; k0 < n; k0 += SF_NB, ++panel) {
        const int k1 = (k0 + SF_NB < n) ? k0 + SF_NB : n;
        const int pw = k1 - k0;
        const int nbelow = n - k1;
        const int ntop = nbelow < SF_NB ? nbelow : SF_NB;  // rows of the next diagonal block
        double* Wt = ws.Wbuf(panel & 1);  // alternating by panel parity
        hipEvent_t e_ur = nullptr, e_f, e_gt;
        // ---- Ur on the main stream: rows [k1, n) -> T rows [2pw, ...)
        if (nbelow > 0) {
            if (e_gt_prev) SF_HIP(hipStreamWaitEvent(s, e_gt_prev, 0));
            sf_gemm_args g = {};
            g.A = A + (int64_t)k1 * lda;
            g.B = A + (int64_t)k0 * lda;
            g.Cin = A + (int64_t)k1 * lda + k0;
            g.Cout = T + (int64_t)(2 * pw) * SF_LDT;
            g.sA = g.sB = g.sCin = stride;
            g.sCout = sT;
            g.lda = g.ldb = g.ldcin = lda;
            g.ldcout = SF_LDT;
            g.M = nbelow;
            g.Nc = pw;
            g.K = k0;
            g.remap_after = 0x7fffffff;
            sf_set_gen(g, gen, 0);  // (the unshifted frame)
            if (gen) {
                g.tm_off = k1 / GT;
                g.tn_off = k0 / GT;
            }
            SF_TRY(launch_gemm(g, batch, true, 2.0 * k0 * (double)nbelow * pw * batch, s));
            SF_TRY(next_event(&e_ur));
            SF_HIP(hipEventRecord(e_ur, s));
        }
        // ---- D + F on the side stream (T rows [0, pw) already hold the fully updated diagonal block)
        hipLaunchKernelGGL(k_diag_mfma, dim3(batch), dim3(1024), 0, c, T, sT, pw, info, k0, rhs ? rhs + k0 : nullptr, ldr,
                           A + (int64_t)k0 * lda + k0, lda, stride, Wt, sW);
        SF_LAUNCH_CHECK();
        if (nbelow <= 0) break;
        SF_TRY(next_event(&e_f));
        SF_HIP(hipEventRecord(e_f, c));
        // ---- G: T[below] W.  Top rows (next diagonal block) on the side stream, the rest on main.
        auto launch_g = [&](int row_lo, int nrows, hipStream_t st) -> int {
            sf_gemm_args g = {};
            g.A = T + (int64_t)(2 * pw + row_lo) * SF_LDT;
            g.B = Wt;
            g.Cout = A + (int64_t)(k1 + row_lo) * lda + k0;
            g.sA = sT;
            g.sB = sW;
            g.sCout = stride;
            g.lda = g.ldb = SF_LDT;
            g.ldcout = lda;
            g.M = nrows;
            g.Nc = pw;
            g.K = pw;
            g.btri = 1;
            g.remap_after = 0x7fffffff;
            return launch_gemm(g, batch, false, (double)nrows * pw * pw * batch, st);
        };
        SF_HIP(hipStreamWaitEvent(c, e_ur, 0));
        SF_TRY(launch_g(0, ntop, c));
        SF_TRY(next_event(&e_gt));
        SF_HIP(hipEventRecord(e_gt, c));
        e_gt_prev = e_gt;
        // next diagonal block: apply this panel's columns and park it in the panel scratch
        SF_TRY(launch_r(k1, ntop, k0, pw, T, SF_LDT, sT, 0, c));
        if (nbelow > ntop) {
            SF_HIP(hipStreamWaitEvent(s, e_f, 0));
            SF_TRY(launch_g(ntop, nbelow - ntop, s));
            // the diagonal blocks after the next one are updated in place
            const int j0 = k1 + ntop;
            if (j0 < n)
                SF_TRY(launch_r(j0, n - j0, k0, pw, A + (int64_t)j0 * lda + j0, lda, stride, (int64_t)SF_NB * lda + SF_NB, s));
        }
    }
    // join: the caller's stream continues only after the side chain is done
    SF_TRY(sf_exec_join(ex, s, c));
    return SF_OK;
}
