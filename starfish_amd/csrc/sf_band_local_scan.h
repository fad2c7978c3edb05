// The score scan for a new local kernel (sf_local_scan.h) on the band + Woodbury solver: with C = Bd + Y^T Y, Sigma = Bd^-1 and
// Vs = Bd^-1 Y^T L_S^-T, W = C^-1 = Sigma - Vs Vs^T.  A candidate needs W on its patch only, so Sigma_ij for |i - j| <= hi - lo:
// the selected inversion is exact on whatever band it is run at (a band wider than the kernels' support holds zeros), so the
// head runs at the widest half-width the LDS window takes, wmax, and every patch of at most wmax + 1 pixels is served exactly.
//
//   k_ls_wband_banded   one 4-wave workgroup per (walker, tile pair I >= J, I - J <= reach): the 64 x 64 tile (I, J) of W in
//                       the layout k_ls_cand reads (sf_ls_tile), with its mirror image.  Entry (i, j), i, j < n, |i - j| <= wmax,
//                       is Sigma[max(i, j)][|i - j|] - sum_c Vs_ci Vs_cj; every other entry of a stored tile is exactly 0.0,
//                       padding rows and columns included.  The rank-m product runs on v_mfma_f64_16x16x4_f64, c ascending in
//                       steps of four, m padded to a multiple of 4 by zero columns; wave w holds rows 16 w .. 16 w + 15.  The
//                       tile passes through LDS (row stride 65: rows and columns both read without bank conflicts) so that
//                       Sigma is read and both images are written in whole rows: 512 contiguous bytes per wave and
//                       instruction -- the direct store of the accumulator layout would scatter the mirror image over 64 rows.
//                       A diagonal tile is formed from its lower triangle, so it is bit-symmetric.  No atomics, one order for
//                       every sum; a walker with info != 0 is neither read nor written.
// Behind it k_ls_patch with the patch limit wmax + 1 (a wider patch would address tiles beyond reach) and k_ls_cand as it is.
#pragma once

#define SF_LSB_REACH 3   // blocks beyond its first that a patch of sf_band_max_halfwidth(2) + 1 = 145 pixels can span
#define SF_LSB_LDT 65    // row stride of the tile in LDS

size_t sf_local_scan_banded_doubles(int n, int batch) {
    const size_t nbr = (size_t)(n + SF_LEAF - 1) / SF_LEAF;
    const size_t reach = nbr - 1 < SF_LSB_REACH ? nbr - 1 : SF_LSB_REACH;
    return (size_t)batch * nbr * (2 * reach + 1) * (SF_LEAF * SF_LEAF);
}

struct sf_lsb_args {
    const double* sigma;  // sigma[b * ssigma + i * lds + d] = Sigma[i][i - d], 0 <= d <= min(i, wmax)
    int64_t ssigma;
    int lds, wmax;
    const double* vs;     // vs[b * svs + c * ldv + i] = Vs_ci, c < m
    int64_t svs;
    int ldv, m;
};

__global__ __launch_bounds__(256) void k_ls_wband_banded(const sf_ls_args a, const sf_lsb_args g) {
    __shared__ double s_t[SF_LEAF * SF_LSB_LDT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l15 = lane & 15, lq = lane >> 4;
    const int b = blockIdx.x % a.batch, id = blockIdx.x / a.batch;
    const int I = id / (a.reach + 1), J = I - id % (a.reach + 1);
    if (J < 0 || a.info[b] != 0) return;  // (the same in every thread)
    const int n = a.f.n;
    // sum_c Vs_ci Vs_cj: lane (lq, l15) holds c = 4 s + lq of row 16 w + l15 of block I and of columns 16 t + l15 of block J
    // (ldv >= 64 nbr: the padding pixels are read, their products masked below)
    const double* vb = g.vs + (int64_t)b * g.svs;
    sf_d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = sf_d4{0.0, 0.0, 0.0, 0.0};
    for (int c0 = 0; c0 < g.m; c0 += 4) {
        const int c = c0 + lq;
        const double* vc = vb + (int64_t)c * g.ldv;
        double vi = 0.0, vj[4] = {0.0, 0.0, 0.0, 0.0};
        if (c < g.m) {
            vi = vc[I * SF_LEAF + 16 * w + l15];
#pragma unroll
            for (int t = 0; t < 4; ++t) vj[t] = vc[J * SF_LEAF + 16 * t + l15];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(vi, vj[t], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_t[(16 * w + lq + 4 * r) * SF_LSB_LDT + 16 * t + l15] = acc[t][r];
    __syncthreads();
    // W = Sigma - the sum, row by row; a diagonal tile from its lower triangle (the thread of (jj, ii) leaves both alone)
    const double* sb = g.sigma + (int64_t)b * g.ssigma;
    for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256) {
        const int ii = e >> 6, jj = e & 63, i = I * SF_LEAF + ii, j = J * SF_LEAF + jj;
        if (I == J && jj > ii) continue;
        double v = 0.0;
        if (i < n && j < n && i - j <= g.wmax) v = sb[(int64_t)i * g.lds + (i - j)] - s_t[ii * SF_LSB_LDT + jj];
        s_t[ii * SF_LSB_LDT + jj] = v;
        if (I == J) s_t[jj * SF_LSB_LDT + ii] = v;
    }
    __syncthreads();
    double* dst = sf_ls_tile(a, b, I, J);
    for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256) dst[e] = s_t[(e >> 6) * SF_LSB_LDT + (e & 63)];
    if (J < I) {  // the mirror image: (column, row)
        double* mir = sf_ls_tile(a, b, J, I);
        for (int e = tid; e < SF_LEAF * SF_LEAF; e += 256) mir[e] = s_t[(e & 63) * SF_LSB_LDT + (e >> 6)];
    }
}

// the launches behind the selected inversion: the band of W, the patches (at most wmax + 1 pixels), the candidates
int sf_launch_local_scan_banded(const sf_fill_args& f, int batch, const double* sigma, int lds, int64_t ssigma, int wmax,
                                const double* vs, int ldv, int64_t svs, int m, const double* alpha, int ld_alpha, const int* info,
                                const double* cand, int ncand, int* patch, double* wband, double* out, hipStream_t s) {
    sf_ls_args a;
    a.f = f;
    a.winv = nullptr, a.alpha = alpha, a.ld_alpha = ld_alpha, a.info = info, a.cand = cand, a.ncand = ncand, a.batch = batch;
    a.nbr = (f.n + SF_LEAF - 1) / SF_LEAF, a.reach = a.nbr - 1 < SF_LSB_REACH ? a.nbr - 1 : SF_LSB_REACH;
    a.patch = patch, a.wband = wband, a.out = out;
    a.max_patch = wmax + 1;
    const sf_lsb_args g = {sigma, ssigma, lds, wmax, vs, svs, ldv, m};
    if (f.n <= 0 || !f.monotonic || ld_alpha < f.n || ldv < a.nbr * SF_LEAF || lds < wmax + 1 || wmax < 0 || m < 1 ||
        (a.max_patch + SF_LEAF - 2) / SF_LEAF > SF_LSB_REACH || a.max_patch > SF_LS_MAXP || batch < 1 || batch > 65535 || ncand < 1 ||
        ncand > 65535) {
        sf_set_error("local scan on the band: n > 0 on a monotonic grid, rows of Vs of at least %d doubles, a half-width in 0 .. %d, "
                     "batch and ncand in 1 .. 65535", a.nbr * SF_LEAF, SF_LSB_REACH * SF_LEAF);
        return SF_EINVAL;
    }
    const long long tiles = (long long)batch * a.nbr * (a.reach + 1);
    SF_CHECK(sf_check_fill_grid(tiles));
    hipLaunchKernelGGL(k_ls_wband_banded, dim3((unsigned)tiles), dim3(256), 0, s, a, g);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ls_patch, dim3(ncand), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ls_cand, dim3(ncand, batch), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
