// Band layer of the covariance fill: the per-diagonal table of the global kernel and the band-storage fill of the
// structure-exploiting solver (sf_band.hip).
#pragma once

// Band storage of Bd = diag(sigma^2) + K_global + sum K_local + jitter for the structure-exploiting
// solver (sf_band.hip): band[i*ldb + d] = Bd[i][i-d], d in [0, ws).  The element formulas and their
// order of additions are those of k_fill_tiles.  Diagonals d > hw (the caller's half-width) are stored as
// zeros; the thread on diagonal hw also probes diagonal hw + 1: a non-zero there means the caller's
// half-width is too small for this walker -> info = SF_INFO_BANDWIDTH (the result would silently drop
// covariance otherwise) -- independently of how many diagonals the storage happens to hold.
// The element formulas are those of sf_matern_elem / sf_local_elem with the per-walker divisions
// hoisted into reciprocals and cos(pi x) evaluated as cospi(x) (differences ~1e-16 relative, far inside
// the 1e-10 covariance tolerance; the dense fill keeps the reference's exact operation order).  k_band_fill and
// k_band_gtab each keep their OWN spelling (r * (1 / r0) here, r / r0 in the table): they differ from the dense formulas
// and from each other in the last bit, on purpose -- not to be merged with sf_matern_elem / sf_local_elem or each other.
// On a log-uniform wavelength grid (lambda_i = lambda_0 e^(i delta): every synthetic order, rectified
// spectra) the metric of the global kernel depends on the offset only, (l_i - l_j)/(l_i + l_j) =
// tanh((i-j) delta/2), so K_global is one value per diagonal: tabulated here per walker from a pair in
// the middle of the order (gtab[b][d], d <= ws; the extra entry feeds the bandwidth probe).  Differences
// to the per-entry evaluation are at the level of the rounding of the grid itself (~3e-11 relative in r).
__global__ __launch_bounds__(256) void k_band_gtab(sf_fill_args a, double* __restrict__ gtab, int ws) {
    const int b = blockIdx.y, d = blockIdx.x * 256 + threadIdx.x;
    if (d > ws) return;
    const double* __restrict__ P = a.params + (int64_t)b * a.pstride;
    const double amp = exp(P[a.off_global]), ls = exp(P[a.off_global + 1]);
    const int i = min(a.n - 1, a.n / 2 + d / 2), j = i - d;
    double v = 0.0;
    if (j >= 0) {
        const double r0 = 6 * ls;
        const double r = SF_C_KMS / 2 * fabs((a.wave[j] - a.wave[i]) / (a.wave[j] + a.wave[i]));
        if (r <= r0) {
            const double t = 1.7320508075688772 / ls * r;
            v = (0.5 + 0.5 * cospi(r / r0)) * amp * (1 + t) * exp(-t);
        }
    }
    gtab[(int64_t)b * (ws + 1) + d] = v;
}

#define SF_BF_ROWS 32
// tile_wt < 0: compact band storage band[i * ldb + d].  tile_wt >= 0: the same values straight into the lower
// 128 x 128 tiles of a dense-strided array (row stride ldb) that meet the band -- element (i, i - d), d < ws =
// 128 (tile_wt + 1), as far left as the first tile column (i / 128 - tile_wt) of the row (sf_launch_potrf_band).
__global__ __launch_bounds__(256) void k_band_fill(sf_fill_args a, double* __restrict__ band, int ws, int hw, int ldb,
                                                   int64_t sband, int* __restrict__ info,
                                                   const double* __restrict__ gtab, int tile_wt) {
    // per-walker constants once per block: exp() of the hyper-parameters (spectrum_model.py:343-357)
    __shared__ double s_glob[4];                 // amp, r0, 1/r0, sqrt(3)/ls
    __shared__ double s_loc[SF_MAX_LOCAL][6];    // mu, amp, r0, 1/r0, -0.5/sigma^2, c/mu
    const int b = blockIdx.y, tid = threadIdx.x;
    const double* __restrict__ P = a.params + (int64_t)b * a.pstride;
    if (tid == 0 && a.has_global) {
        const double amp = exp(P[a.off_global]), ls = exp(P[a.off_global + 1]);
        s_glob[0] = amp;
        s_glob[1] = 6 * ls;
        s_glob[2] = 1.0 / (6 * ls);
        s_glob[3] = 1.7320508075688772 / ls;
    }
    if (tid >= 64 && tid < 64 + a.n_local) {
        const int k = tid - 64;
        const double sig = exp(P[a.off_local + 3 * k + 2]);
        s_loc[k][0] = P[a.off_local + 3 * k];
        s_loc[k][1] = exp(P[a.off_local + 3 * k + 1]);
        s_loc[k][2] = 4 * sig;
        s_loc[k][3] = 1.0 / (4 * sig);
        s_loc[k][4] = -0.5 / (sig * sig);
        s_loc[k][5] = SF_C_KMS / s_loc[k][0];
    }
    __syncthreads();
    // SF_BF_ROWS rows per block (the exp() prologue is amortised), one wave per row at a time, 64 lanes
    // along the diagonals of the row (coalesced stores, no index division)
    const int lane = tid & 63;
    const double* __restrict__ gt = gtab ? gtab + (int64_t)b * (ws + 1) : nullptr;
    for (int i = blockIdx.x * SF_BF_ROWS + (tid >> 6); i < min(a.npad, (int)(blockIdx.x + 1) * SF_BF_ROWS); i += 4) {
        const bool tiled = tile_wt >= 0;
        double* __restrict__ dst = band + (int64_t)b * sband + (int64_t)i * ldb + (tiled ? i : 0);
        const int dmax = tiled ? i - max((i >> 7) - tile_wt, 0) * 128 : ws - 1;  // last stored diagonal of this row
        const int dstep = tiled ? -1 : 1;
        if (i >= a.n) {
            for (int d = lane; d <= min(dmax, ws - 1); d += 64) dst[dstep * d] = (d == 0) ? 1.0 : 0.0;  // identity padding
            continue;
        }
        const double w_row = a.wave[i];
        auto structured = [&](int col, bool& any) {
            const double w_col = a.wave[col];
            double acc = 0.0;
            if (a.has_global && gt) {
                acc = gt[i - col];
                any = any || acc != 0.0;
            } else if (a.has_global) {
                const double r = SF_C_KMS / 2 * fabs((w_col - w_row) / (w_col + w_row));
                if (r <= s_glob[1]) {
                    const double t = s_glob[3] * r;
                    acc = (0.5 + 0.5 * cospi(r * s_glob[2])) * s_glob[0] * (1 + t) * exp(-t);
                    any = true;
                }
            }
            for (int k = 0; k < a.n_local; ++k) {
                const double mu = s_loc[k][0], cm = s_loc[k][5];
                const double d_row = cm * fabs(w_row - mu), d_col = cm * fabs(w_col - mu);
                const double r_tap = fmax(d_row, d_col);
                if (r_tap <= s_loc[k][2]) {
                    acc += (0.5 + 0.5 * cospi(r_tap * s_loc[k][3])) * s_loc[k][1] *
                           exp((d_col * d_col + d_row * d_row) * s_loc[k][4]);
                    any = true;
                }
            }
            return acc;
        };
        for (int d = lane; d <= min(dmax, ws - 1); d += 64) {
            const int j = i - d;
            double v = 0.0;
            if (j >= 0 && d <= hw) {  // diagonals past the caller's half-width are stored as zeros, never as data
                bool any = false;
                const double k = structured(j, any);
                if (d == 0) {
                    const double sg = a.sigma[i];
                    v = sg * sg;
                    v = v + k;
                    if (a.add_jitter) v = v + SF_JITTER;
                } else {
                    v = k;
                }
                if (d == hw && j >= 1) {
                    // first diagonal past the caller's half-width (whatever the storage width): non-zero -> too small
                    bool outside = false;
                    (void)structured(j - 1, outside);
                    if (outside) atomicCAS(info + b, 0, SF_INFO_BANDWIDTH);
                }
            }
            dst[dstep * d] = v;
        }
    }
}

int sf_launch_band_fill(const sf_fill_args& a, int B, double* band, int ws, int halfwidth, int ldb, int64_t sband,
                        int* info, double* gtab, hipStream_t s, int tile_wt) {
    if (halfwidth < 0 || halfwidth >= ws) {
        sf_set_error("band fill: half-width %d does not fit the %d stored diagonals", halfwidth, ws);
        return SF_EINVAL;
    }
    SF_CHECK(sf_check_n_local(a));
    if (!a.monotonic) {
        sf_set_error("the banded solver needs a strictly increasing wavelength grid");
        return SF_EINVAL;
    }
    const bool table = gtab && a.has_global && a.loguniform && 2 * ws < a.n;
    if (table) {
        hipLaunchKernelGGL(k_band_gtab, dim3((ws + 256) / 256, B), dim3(256), 0, s, a, gtab, ws);
        SF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_band_fill, dim3((unsigned)((a.npad + SF_BF_ROWS - 1) / SF_BF_ROWS), B), dim3(256), 0, s, a, band, ws, halfwidth, ldb, sband,
                       info, table ? (const double*)gtab : nullptr, tile_wt);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
