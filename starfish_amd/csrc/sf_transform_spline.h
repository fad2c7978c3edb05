// The quintic B-spline of the log-lambda grid: the banded solve of the collocation system (k_spline_solve), the same
// solve as a block-banded MFMA product with the precomputed inverse (k_spline_apply, the per-walker path), the FITPACK
// basis / interval helpers the evaluation kernels share, and the generic resample k_spline_eval.   transforms.py:39-42
#pragma once
#include "sf_device.h"
#include "sf_transform.h"
typedef double sf_d4x __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------- banded spline solve
// One lane per right-hand side; element j of system s lives at data[s_base(s) + j*estride].
// Systems are grouped: s = b*rows + r -> base = b*bstride + r*rstride.
// The recurrences are sequential in j and only ~20 waves exist (B*(m+2)/64), so the kernel is pure
// latency: every lane keeps the NEXT chunk of SCH rows (and lane l the factor row j0+l) in flight in
// registers while the current chunk is eliminated; factor rows are broadcast through LDS.
#define SCH 64
__global__ __launch_bounds__(64) void k_spline_solve(double* __restrict__ data, int nsys, int rows,
                                                     int64_t bstride, int64_t rstride, int64_t estride,
                                                     int n, const double* __restrict__ Lf,
                                                     const double* __restrict__ Uf,
                                                     const double* __restrict__ rdiag) {
    __shared__ double fac[SCH * (SF_KB + 1)];
    const int lane = threadIdx.x;
    int s = blockIdx.x * 64 + lane;
    const bool live = s < nsys;
    if (!live) s = nsys - 1;  // keep the wave converged; results of dead lanes are not stored
    const int b = s / rows, r = s - b * rows;
    double* x = data + (int64_t)b * bstride + (int64_t)r * rstride;
    const int nch = (n + SCH - 1) / SCH;

    double cur[SCH], nxt[SCH];
    double cf[SF_KB + 1], nf[SF_KB + 1];
    auto load_chunk = [&](int ch, double* v) {
        const int j0 = ch * SCH;
#pragma unroll
        for (int jj = 0; jj < SCH; ++jj) v[jj] = (j0 + jj < n) ? x[(int64_t)(j0 + jj) * estride] : 0.0;
    };
    auto store_chunk = [&](int ch, const double* v) {
        const int j0 = ch * SCH;
        if (!live) return;
#pragma unroll
        for (int jj = 0; jj < SCH; ++jj)
            if (j0 + jj < n) x[(int64_t)(j0 + jj) * estride] = v[jj];
    };
    auto load_fac = [&](int ch, const double* __restrict__ F, bool with_diag, double* f) {
        const int j = ch * SCH + lane;
#pragma unroll
        for (int k = 0; k < SF_KB; ++k) f[k] = (j < n) ? F[(int64_t)j * SF_KB + k] : 0.0;
        f[SF_KB] = (with_diag && j < n) ? rdiag[j] : 0.0;
    };
    auto publish_fac = [&](const double* f) {
        __syncthreads();  // everyone finished reading the previous chunk's factors
#pragma unroll
        for (int k = 0; k <= SF_KB; ++k) fac[lane * (SF_KB + 1) + k] = f[k];
        __syncthreads();
    };

    // ---------------- forward: y_j = b_j - sum_{k=1..KB} L[j][k] y_{j-k}
    double y1 = 0, y2 = 0, y3 = 0, y4 = 0, y5 = 0;
    load_fac(0, Lf, false, cf);
    load_chunk(0, cur);
    for (int ch = 0; ch < nch; ++ch) {
        publish_fac(cf);
        if (ch + 1 < nch) {
            load_fac(ch + 1, Lf, false, nf);
            load_chunk(ch + 1, nxt);
        }
#pragma unroll
        for (int jj = 0; jj < SCH; ++jj) {
            const double* l = &fac[jj * (SF_KB + 1)];
            // older terms first (off the critical path); the dependent step is a single fma
            const double part = cur[jj] - ((l[4] * y5 + l[3] * y4) + (l[2] * y3 + l[1] * y2));
            const double v = fma(-l[0], y1, part);
            cur[jj] = v;
            y5 = y4; y4 = y3; y3 = y2; y2 = y1; y1 = v;
        }
        store_chunk(ch, cur);
#pragma unroll
        for (int jj = 0; jj < SCH; ++jj) cur[jj] = nxt[jj];
#pragma unroll
        for (int k = 0; k <= SF_KB; ++k) cf[k] = nf[k];
    }
    // ---------------- backward: c_j = (y_j - sum_{k=1..KB} U[j][k] c_{j+k}) / U[j][j]
    double c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
    __threadfence_block();
    load_fac(nch - 1, Uf, true, cf);
    load_chunk(nch - 1, cur);
    for (int ch = nch - 1; ch >= 0; --ch) {
        publish_fac(cf);
        if (ch > 0) {
            load_fac(ch - 1, Uf, true, nf);
            load_chunk(ch - 1, nxt);
        }
        const int j0 = ch * SCH;
#pragma unroll
        for (int jj = SCH - 1; jj >= 0; --jj) {
            if (j0 + jj < n) {
                const double* u = &fac[jj * (SF_KB + 1)];
                const double part = (cur[jj] - ((u[4] * c5 + u[3] * c4) + (u[2] * c3 + u[1] * c2))) * u[SF_KB];
                const double v = fma(-(u[0] * u[SF_KB]), c1, part);
                cur[jj] = v;
                c5 = c4; c4 = c3; c3 = c2; c2 = c1; c1 = v;
            }
        }
        store_chunk(ch, cur);
#pragma unroll
        for (int jj = 0; jj < SCH; ++jj) cur[jj] = nxt[jj];
#pragma unroll
        for (int k = 0; k <= SF_KB; ++k) cf[k] = nf[k];
    }
}

int sf_launch_spline_solve(double* data, int B, int rows, int64_t bstride, int64_t rstride,
                           int64_t estride, int n, const double* Lf, const double* Uf, const double* rdiag,
                           hipStream_t s) {
    const int nsys = B * rows;
    hipLaunchKernelGGL(k_spline_solve, dim3((nsys + 63) / 64), dim3(64), 0, s, data, nsys, rows, bstride,
                       rstride, estride, n, Lf, Uf, rdiag);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Fully parallel variant for the per-walker path: the collocation matrix of the fixed log-lambda grid is
// well conditioned (cond ~ 15) and its inverse decays like 0.43^|i-j|, so c_i = sum_{|d| <= SF_IW}
// Ainv[i][i+d] y_{i+d} with the band precomputed at context creation (truncation < 1e-23 relative).
// That is a block-banded matrix product and runs on v_mfma_f64_16x16x4_f64:
//   C[16 i's][rows] = sum over the 9 input blocks kb of  T[ib][kb] (16 x 16)  x  Y[16 k's][rows]
// One wave owns one block of 16 outputs and keeps its 9 T blocks in registers (36 A fragments) while it
// loops over a chunk of walkers, so the 9.4 MB table is read B/chunk times, not B times; the B operand
// (lane (k, r) <- y[b][r][k], every row contiguous as the FFT kernel writes it) and the result are addressed
// straight in HBM/L2: no LDS.
// The walker loop is software pipelined: the fragments of walker b+1 are in flight while the matrix
// core works on walker b.
// y is [B][rows][n], c is [B][n][rows] (what k_eval_rows reads); tblk is [n/16][SF_IBLK][16][16] (zero outside
// the band / the matrix).  A launch covers the rows row0 .. row0 + 16 NCB - 1 (the register budget stops at NCB = 2).
#define SF_IBLK (2 * (SF_IW / 16) + 1)
template <int NCB>
__global__ __launch_bounds__(256) void k_spline_apply(const double* __restrict__ y, double* __restrict__ c,
                                                      int rows, int n, const double* __restrict__ tblk, int B,
                                                      int wchunk, int row0) {
    const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
    const int ib = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ib * 16 >= n) return;
    double a[SF_IBLK][4];
#pragma unroll
    for (int kb = 0; kb < SF_IBLK; ++kb)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            a[kb][kk] = tblk[(((int64_t)ib * SF_IBLK + kb) * 16 + l15) * 16 + 4 * lq + kk];  // K slice lq of MFMA kk <-> k = 4 lq + kk
    const int nblk16 = n / 16;
    const int b0 = blockIdx.y * wchunk, b1 = min(B, b0 + wchunk);
    double bA[SF_IBLK][4][NCB], bB[SF_IBLK][4][NCB];
    // lane (r = l15, lq) takes the four CONTIGUOUS inputs 4 lq .. 4 lq + 3 of row r of a block (the same
    // permutation of the summation index as in the coefficient fragments): one 32-byte load per block
    auto fetch = [&](int b, double (&dst)[SF_IBLK][4][NCB]) {
        const double* yb = y + (int64_t)b * n * rows;
#pragma unroll
        for (int kb = 0; kb < SF_IBLK; ++kb) {
            int kblk = ib - SF_IW / 16 + kb;  // blocks outside the matrix carry zero coefficients
            kblk = kblk < 0 ? 0 : (kblk >= nblk16 ? nblk16 - 1 : kblk);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int r = row0 + cb * 16 + l15;
                const double2* p = (const double2*)(yb + (int64_t)(r < rows ? r : 0) * n + kblk * 16 + 4 * lq);
                const double2 lo = p[0], hi = p[1];  // rows >= `rows` are never stored
                dst[kb][0][cb] = lo.x;
                dst[kb][1][cb] = lo.y;
                dst[kb][2][cb] = hi.x;
                dst[kb][3][cb] = hi.y;
            }
        }
    };
    auto compute = [&](int b, const double (&bv)[SF_IBLK][4][NCB]) {
        sf_d4x acc[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = (sf_d4x){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < SF_IBLK; ++kb)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb)
                    acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kb][kk], bv[kb][kk][cb], acc[cb], 0, 0, 0);
        double* cb_ = c + (int64_t)b * n * rows;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int i = ib * 16 + lq + 4 * r4;
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int r = row0 + cb * 16 + l15;
                if (r < rows && i < n) cb_[(int64_t)i * rows + r] = acc[cb][r4];
            }
        }
    };
    if (b0 < b1) fetch(b0, bA);
    for (int b = b0; b < b1; b += 2) {  // ping-pong: the fragments of the next walker are in flight
        if (b + 1 < b1) fetch(b + 1, bB);
        compute(b, bA);
        if (b + 1 < b1) {
            if (b + 2 < b1) fetch(b + 2, bA);
            compute(b + 1, bB);
        }
    }
}

int sf_launch_spline_apply(const double* y, double* c, int B, int rows, int n, const double* tblk, hipStream_t s) {
    const int ncb = (rows + 15) / 16;  // (rows = m + 2 <= SF_MAX_M + 2: at most 3 column blocks)
    if (ncb > 3 || n % 16) {
        sf_set_error("spline_apply: rows=%d n=%d not supported", rows, n);
        return SF_EINVAL;
    }
    // enough waves to fill the chip (n/16 output blocks x walker chunks), long enough chunks to amortise
    // the register-resident coefficient blocks
    int wchunk = 32;
    while (wchunk > 4 && (int64_t)(n / 16) * ((B + wchunk - 1) / wchunk) < 2048) wchunk >>= 1;
    const dim3 grid((n / 16 + 3) / 4, (B + wchunk - 1) / wchunk);
    if (ncb == 1) hipLaunchKernelGGL(k_spline_apply<1>, grid, dim3(256), 0, s, y, c, rows, n, tblk, B, wchunk, 0);
    else hipLaunchKernelGGL(k_spline_apply<2>, grid, dim3(256), 0, s, y, c, rows, n, tblk, B, wchunk, 0);
    SF_LAUNCH_CHECK();
    if (ncb == 3) {  // m = 31, 32: the rows past the first 32 in a second pass
        hipLaunchKernelGGL(k_spline_apply<1>, grid, dim3(256), 0, s, y, c, rows, n, tblk, B, wchunk, 32);
        SF_LAUNCH_CHECK();
    }
    return SF_OK;
}

// ------------------------------------------------------------------------ spline evaluation
// FITPACK fpbspl: the six non-zero quintic B-splines on [t[ell], t[ell+1]) at x, knots scaled by s.
__device__ __forceinline__ void sf_bspl6(const double* __restrict__ t, double s, int ell, double x,
                                         double h[6]) {
    double tk[12];  // t[ell-5 .. ell+6] scaled
#pragma unroll
    for (int i = 0; i < 12; ++i) tk[i] = t[ell - 5 + i] * s;
    double hh[5];
    h[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= 5; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
#pragma unroll
        for (int i = 1; i <= j; ++i) {
            // li = ell + i, lj = li - j  -> tk index = (.) - (ell - 5)
            const double tli = tk[5 + i], tlj = tk[5 + i - j];
            const double f = hh[i - 1] / (tli - tlj);
            h[i - 1] = h[i - 1] + f * (tli - x);
            h[i] = f * (x - tlj);
        }
    }
}

// splev interval search: largest ell in [5, ncoef-1] with t[ell]*s <= x
__device__ __forceinline__ int sf_find_interval(const double* __restrict__ t, double s, int ncoef, double x) {
    int lo = 5, hi = ncoef - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid] * s <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Generic resample (free function): out[r][q] = spline_r(xq[q]); coefficients coef[r][j] row-major.
__global__ __launch_bounds__(256) void k_spline_eval(const double* __restrict__ coef, int rows, int ncoef,
                                                     const double* __restrict__ t,
                                                     const double* __restrict__ xq, int nq,
                                                     double* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const double x = xq[q];
    const int ell = sf_find_interval(t, 1.0, ncoef, x);
    double h[6];
    sf_bspl6(t, 1.0, ell, x, h);
    for (int r = 0; r < rows; ++r) {
        const double* c = coef + (int64_t)r * ncoef + ell - 5;
        double sp = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) sp = sp + c[j] * h[j];
        out[(int64_t)r * nq + q] = sp;
    }
}

int sf_launch_spline_eval(const double* coef, int rows, int ncoef, const double* t, const double* xq, int nq,
                          double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_spline_eval, dim3((nq + 255) / 256), dim3(256), 0, s, coef, rows, ncoef, t, xq, nq,
                       out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
