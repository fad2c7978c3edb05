// Residual diagnostics on the band solver (sf_diagnose_banded_batch): what the gradient's sequence lacks.
//
//   stage      k_band_diag_stage: the sweep's rows [R; Y] for caller right-hand sides R (the rows of Y behind them, so that the
//              Gram matrix holds G_YY and G_Y,R and the backward sweep gives T = Bd^-1 [R^T, Y^T]).  The mix for k right-hand
//              sides is k_band_mix_matrix / k_band_mix of sf_band_solve.h, Vs is k_band_vs_matrix of sf_band_selinv.h
//   read-out   k_band_cinv_diag: diag(C^-1) = diag(Sigma) - rowsum(Vs^2) from the selected inversion's band and Vs;
//              k_band_cov_diag: diag(C) = diag(Bd) + colsum(Y^2), diag(Bd) being the first column of the filled band (the
//              keeping sweep does not modify the band)
// One thread per pixel, coalesced over the pixels of a row; every sum has one order; rows >= n are neither read nor written.
#pragma once
#include "sf_band_solve.h"

__global__ __launch_bounds__(256) void k_band_diag_stage(const double* __restrict__ rhs, int ldr, int64_t rhs_stride,
                                                         const double* __restrict__ Y, int64_t sy, int n, int npad, int kr,
                                                         double* __restrict__ buf) {
    const int r = blockIdx.y, b = blockIdx.z, nin = gridDim.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double v = 0.0;
    if (r >= kr) v = Y[(int64_t)b * sy + (int64_t)(r - kr) * npad + i];
    else if (i < n) v = rhs[(int64_t)b * rhs_stride + (int64_t)r * ldr + i];
    buf[((int64_t)b * nin + r) * npad + i] = v;
}
int sf_launch_band_diag_stage(const double* rhs, int ldr, int64_t rhs_stride, const double* Y, int64_t sy, int n, int npad, int kr,
                              int m, int batch, double* buf, hipStream_t s) {
    if (!rhs || !Y || !buf || n <= 0 || npad < n || ldr < n || kr < 1 || m < 1 || kr + m > SFB_MIX_MAX || batch <= 0 || batch > 65535) {
        sf_set_error("band_diag_stage: bad arguments (n=%d npad=%d ldr=%d, %d + %d rows, batch=%d)", n, npad, ldr, kr, m, batch);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_band_diag_stage, dim3((npad + 255) / 256, kr + m, batch), dim3(256), 0, s, rhs, ldr, rhs_stride, Y, sy, n, npad,
                       kr, buf);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// cinv_diag[b][i] = Sigma_ii - sum_c Vs_ic^2, c ascending
__global__ __launch_bounds__(256) void k_band_cinv_diag(const double* __restrict__ sigma, int lds, int64_t ssigma,
                                                        const double* __restrict__ vs, int ldv, int64_t svs, int m,
                                                        const int* __restrict__ info, int n, double* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = __builtin_nan("");
    if (info[b] == 0) {
        const double* vb = vs + (int64_t)b * svs + i;
        double sum = 0.0;
        for (int c = 0; c < m; ++c) {
            const double t = vb[(int64_t)c * ldv];
            sum += t * t;
        }
        v = sigma[(int64_t)b * ssigma + (int64_t)i * lds] - sum;
    }
    out[(int64_t)b * n + i] = v;
}
int sf_launch_band_cinv_diag(const double* sigma, int lds, int64_t ssigma, const double* vs, int ldv, int64_t svs, int m,
                             const int* info, int n, int batch, double* cinv_diag, hipStream_t s) {
    if (!sigma || !vs || !info || !cinv_diag || n <= 0 || ldv < n || lds < 1 || m < 1 || batch <= 0 || batch > 65535) {
        sf_set_error("band_cinv_diag: bad arguments (n=%d ldv=%d lds=%d m=%d batch=%d)", n, ldv, lds, m, batch);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_band_cinv_diag, dim3((n + 255) / 256, batch), dim3(256), 0, s, sigma, lds, ssigma, vs, ldv, svs, m, info, n,
                       cinv_diag);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// cov_diag[b][i] = band[b][i][0] + sum_j Y_ji^2, j ascending: the diagonal of C = Bd + Y^T Y as it is factorised, jitter included
__global__ __launch_bounds__(256) void k_band_cov_diag(const double* __restrict__ band, int ldb, int64_t sband,
                                                       const double* __restrict__ Y, int ldy, int64_t sy, int m,
                                                       const int* __restrict__ info, int n, double* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = __builtin_nan("");
    if (info[b] == 0) {
        const double* yb = Y + (int64_t)b * sy + i;
        double sum = 0.0;
        for (int j = 0; j < m; ++j) {
            const double t = yb[(int64_t)j * ldy];
            sum += t * t;
        }
        v = band[(int64_t)b * sband + (int64_t)i * ldb] + sum;
    }
    out[(int64_t)b * n + i] = v;
}
int sf_launch_band_cov_diag(const double* band, int ldb, int64_t sband, const double* Y, int ldy, int64_t sy, int m, const int* info,
                            int n, int batch, double* cov_diag, hipStream_t s) {
    if (!band || !Y || !info || !cov_diag || n <= 0 || ldb < 1 || ldy < n || m < 1 || batch <= 0 || batch > 65535) {
        sf_set_error("band_cov_diag: bad arguments (n=%d ldb=%d ldy=%d m=%d batch=%d)", n, ldb, ldy, m, batch);
        return SF_EINVAL;
    }
    hipLaunchKernelGGL(k_band_cov_diag, dim3((n + 255) / 256, batch), dim3(256), 0, s, band, ldb, sband, Y, ldy, sy, m, info, n,
                       cov_diag);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
