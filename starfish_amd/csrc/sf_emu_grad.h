// The emulator training likelihood's gradient in its hyper-parameters: the contraction of sf_grad_frame.h with alpha =
// V^-1 w_hat for V = v11 = iPhiPhi / lambda_xi + blockdiag_c K_c, K_c[g,h] = variance_c exp(-1/2 sum_p ((x_gp - x_hp) / l_cp)^2)
// (sf_transform_v11.h; row i = component i / M, grid point i % M) and theta the LOGS of lambda_xi, variance_c, l_cp:
//     log lambda_xi   -iPhiPhi_ij / lambda_xi                         every entry of the dense n x n array
//     log variance_c  K_c[g,h]                                        where i / M == j / M == c
//     log l_cp        K_c[g,h] ((x_gp - x_hp) / l_cp)^2               where i / M == j / M == c
// iPhiPhi is dense to this layer, so every 64 x 64 block of V^-1 of the lower triangle is formed.  A layer of sf_fill.hip; the
// scaled coordinates are staged as k_v11_build_batch stages them.
//
//   k_emu_grad      the frame's block-row kernel.  It walks J = 0 .. I in order.  Per pair: the tile, the lambda_xi slot sum
//                   A_ij iPhiPhi_ij (the 16 consecutive columns of a quarter-wave are one 128-byte segment of a row; the
//                   factor -1 / lambda_xi is applied once, to the block row's sum), and, where the component ranges of the
//                   pair's rows and columns meet (the rbf test of k_v11_build_batch), the kernel entries: A_ij variance_c
//                   exp(-1/2 d2) once per entry, kept in the tile's registers, then one component at a time (M = 27 puts up
//                   to four in 64 rows) its sum and its sums weighted with the squared scaled differences of each grid axis,
//                   the entries of other components masked, flushed together.  The partial sums are zero for the components
//                   the block row does not hold.
// The tile runs on v_mfma_f64_16x16x4_f64 through sf_inv_sweep: it is a matrix product, n^3 / 3 flops over the lower tiles.
// The entries run on plain VALU arithmetic: the contraction with dV / d theta is an element-wise product, each entry behind
// an exp that costs more than the 2 + P multiply-adds it feeds, so the matrix cores would have nothing to do.
// iPhiPhi and the grid are not read for rows and columns >= n.
#pragma once

#define SF_EG_PMAX 8                      // grid axes (SF_V11_PMAX of the build)
#define SF_EG_NQ (1 + SF_EG_PMAX)         // sums of a component: variance, then one per axis
#define SF_EG_SUMS (1 + SF_LEAF * SF_EG_NQ)  // running sums of a block row: lambda_xi, then at most 64 components

struct sf_emu_grad_args {
    const double* grid;     // [M][P]
    int M, P, m, n;         // n = m M
    const double* hyper;    // [batch][hyper_stride]: lambda_xi, variances[m], lengthscales[m][P] (raw)
    int hyper_stride;
    const double* iphiphi;  // [n][n]
    const double* L;        // [batch] x stride: the factored matrices after the inverse's launch (X^T above)
    int npad, lda;
    int64_t stride;
    const double* winv;     // [batch][npad / 64][64][64]
    const double* alpha;    // [batch][ld_alpha]: V^-1 w_hat
    int ld_alpha;
    sf_grad_out o;
};

// Row (column) g of v11 staged at slot t of a 64-row block, as k_v11_build_batch stages it: the scaled coordinates
// x[p][t] = grid[g % M][p] / l_cp with the lengthscales of its own component c = g / M, and comp[t] = c; zeros and -1 for
// g >= n, where nothing is read.  Returns the variance of the component (0 for g >= n).
__device__ __forceinline__ double sf_emu_grad_stage(const sf_emu_grad_args& a, const double* hb, int g, int t,
                                                    double (*x)[SF_LEAF], int* comp) {
    const int c = g < a.n ? g / a.M : -1;
    comp[t] = c;
    if (c < 0) {
        for (int p = 0; p < a.P; ++p) x[p][t] = 0.0;
        return 0.0;
    }
    const double* gp = a.grid + (int64_t)(g - c * a.M) * a.P;
    const double* ls = hb + 1 + a.m + c * a.P;
    for (int p = 0; p < a.P; ++p) x[p][t] = gp[p] / ls[p];
    return hb[1 + c];
}

__global__ __launch_bounds__(256) void k_emu_grad(const sf_emu_grad_args a) {
    __shared__ double xr[SF_EG_PMAX][SF_LEAF];  // scaled coordinates of the block row's rows
    __shared__ double xc[SF_EG_PMAX][SF_LEAF];  // ... and of the pair's columns
    __shared__ double vr[SF_LEAF];              // variance of each row's component
    __shared__ int cr[SF_LEAF], cc[SF_LEAF];    // component of each row / column, -1: padding
    __shared__ double s_sum[SF_EG_SUMS];
    __shared__ double s_red[4 * SF_EG_NQ];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int n = a.n, M = a.M, P = a.P;
    int b, I;
    if (!sf_grad_block(a.o, b, I)) return;
    const double* __restrict__ hb = a.hyper + (int64_t)b * a.hyper_stride;
    const double* __restrict__ al = a.alpha + (int64_t)b * a.ld_alpha;
    const sf_cinv_src src = sf_cinv_source(a.L, a.npad, a.lda, a.stride, a.winv, b);
    const int R0 = I * SF_LEAF, ci0 = R0 / M, ci1 = min(R0 + SF_LEAF - 1, n - 1) / M;
    const int nq = 1 + P, nsum = 1 + (ci1 - ci0 + 1) * nq;  // (at most 64 components in 64 rows: nsum <= SF_EG_SUMS)
    for (int q = tid; q < nsum; q += 256) s_sum[q] = 0.0;
    // the rows are the same for every pair of the block row: staged once
    if (tid < SF_LEAF) vr[tid] = sf_emu_grad_stage(a, hb, R0 + tid, tid, xr, cr);
    double a_r[4];
    bool ok_r[4];
    sf_grad_rows(al, R0, n, w, lq, a_r, ok_r);
    for (int J = 0; J <= I; ++J) {
        const int C0 = J * SF_LEAF;
        const int cj0 = C0 / M, cj1 = min(C0 + SF_LEAF - 1, n - 1) / M;
        const bool rbf = ci0 <= cj1 && cj0 <= ci1;  // the component ranges of rows and columns meet
        __syncthreads();  // the last pair's columns are read; the rows and s_sum are in place
        if (rbf && tid < SF_LEAF) sf_emu_grad_stage(a, hb, C0 + tid, tid, xc, cc);
        const double wgt = sf_grad_weight(I, J);
        sf_d4 A[4];
        bool ok_c[4];
        sf_grad_tile(src, al, n, I, J, w, l15, lq, a_r, ok_r, A, ok_c);
        double v = 0.0;  // the lambda_xi slot
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t at = (int64_t)(R0 + 16 * w + lq + 4 * r) * n + C0 + 16 * t + l15;
                const double ip = ok_r[r] && ok_c[t] ? a.iphiphi[at] : 0.0;
                v = v + A[t][r] * ip;
            }
        sf_grad_put(v, s_red + w * SF_EG_NQ, lane);
        sf_grad_flush(1, wgt, s_red, SF_EG_NQ, s_sum, tid);  // (its first barrier also publishes the staged columns)
        if (!rbf) continue;  // (the same in every thread)
        // A_ij K_c[g,h] where row and column belong to one component, zero elsewhere: one exp per entry
        int c_r[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) c_r[r] = cr[16 * w + lq + 4 * r];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = 16 * t + l15, c_c = cc[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * w + lq + 4 * r;
                double k = 0.0;
                if (c_r[r] >= 0 && c_r[r] == c_c) {
                    double d2 = 0.0;
                    for (int p = 0; p < P; ++p) {
                        const double d = xr[p][row] - xc[p][col];
                        d2 = d2 + d * d;
                    }
                    k = A[t][r] * (vr[row] * exp(-0.5 * d2));
                }
                A[t][r] = k;
            }
        }
        for (int c = max(ci0, cj0); c <= min(ci1, cj1); ++c) {
            for (int q = 0; q < nq; ++q) {  // q = 0: the variance; q > 0: grid axis q - 1
                double s = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (c_r[r] != c) continue;  // (entries whose column belongs to another component are zero already)
                    const int row = 16 * w + lq + 4 * r;
                    const double x = q ? xr[q - 1][row] : 0.0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const double d = q ? x - xc[q - 1][16 * t + l15] : 1.0;
                        s = s + A[t][r] * (d * d);
                    }
                }
                sf_grad_put(s, s_red + w * SF_EG_NQ + q, lane);
            }
            sf_grad_flush(nq, wgt, s_red, SF_EG_NQ, s_sum + 1 + (c - ci0) * nq, tid);
        }
    }
    __syncthreads();
    // slots in the order of the raw row: lambda_xi, variances[m], lengthscales[m][P]
    double* part = sf_grad_part(a.o, b, I);
    for (int q = tid; q < a.o.nslots; q += 256) {
        double s;
        if (q == 0) {
            s = -s_sum[0] / hb[0];
        } else {
            const int c = q <= a.m ? q - 1 : (q - 1 - a.m) / P, k = q <= a.m ? 0 : 1 + (q - 1 - a.m) % P;
            s = c >= ci0 && c <= ci1 ? s_sum[1 + (c - ci0) * nq + k] : 0.0;
        }
        part[q] = s;
    }
}

size_t sf_emu_grad_work_doubles(int M, int P, int m, int batch) {
    if (M <= 0 || P <= 0 || m <= 0 || batch <= 0) return 0;
    return sf_grad_part_doubles((size_t)m * M, sf_emu_grad_slots(m, P), batch);
}
// every argument is the caller's to check (sf_emulator_loglike_grad_batch does, before its first launch)
int sf_launch_emu_grad(const double* grid, int M, int P, int m, const double* hyper, int hyper_stride, int batch,
                       const double* iphiphi, const double* L, int npad, int lda, int64_t stride, const double* winv,
                       const double* alpha, int ld_alpha, const int* info, double* part, double* grad, int grad_stride,
                       hipStream_t s) {
    sf_emu_grad_args a;
    a.grid = grid, a.M = M, a.P = P, a.m = m, a.n = m * M, a.hyper = hyper, a.hyper_stride = hyper_stride, a.iphiphi = iphiphi;
    a.L = L, a.npad = npad, a.lda = lda, a.stride = stride, a.winv = winv, a.alpha = alpha, a.ld_alpha = ld_alpha;
    a.o = sf_grad_out{info, part, (a.n + SF_LEAF - 1) / SF_LEAF, sf_emu_grad_slots(m, P), batch, grad, grad_stride};
    if (M <= 0 || m <= 0 || P < 1 || P > SF_EG_PMAX || npad % SF_LEAF != 0 || npad < a.n || lda < npad || ld_alpha < a.n ||
        grad_stride < a.o.nslots || hyper_stride < a.o.nslots || batch < 1 || batch > 65535) {
        sf_set_error("emu grad: P in 1 .. %d, npad a multiple of %d >= m M, grad_stride and hyper_stride >= 1 + m + m P, "
                     "ld_alpha >= m M, batch in 1 .. 65535", SF_EG_PMAX, SF_LEAF);
        return SF_EINVAL;
    }
    return sf_launch_grad(k_emu_grad, a, a.o, s);
}
