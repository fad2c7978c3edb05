// Element layer of the covariance fill: the two structured element formulas, the hyper-parameter read-out of a walker, the
// support test every culling decision goes through, and the host-side checks the fill's launchers share.
#pragma once

// kernels.py:27-40 with wx = wave[col], wy = wave[row]
__device__ __forceinline__ double sf_matern_elem(double w_row, double w_col, double amp, double ls,
                                                 double r0) {
    const double r = SF_C_KMS / 2 * fabs((w_col - w_row) / (w_col + w_row));
    if (!(r <= r0)) return 0.0;
    const double taper = 0.5 + 0.5 * cos(M_PI * r / r0);
    const double s3 = 1.7320508075688772;  // numpy.sqrt(3)
    return taper * amp * (1 + s3 * r / ls) * exp(-s3 * r / ls);
}

// kernels.py:68-80 with x = met[col], y = met[row]
__device__ __forceinline__ double sf_local_elem(double d_row, double d_col, double amp, double sigma,
                                                double r0) {
    const double r_tap = fmax(d_col, d_row);
    if (!(r_tap <= r0)) return 0.0;
    const double r2 = d_col * d_col + d_row * d_row;
    const double taper = 0.5 + 0.5 * cos(M_PI * r_tap / r0);
    return taper * amp * exp(-0.5 * r2 / (sigma * sigma));
}

__device__ __forceinline__ double sf_local_metric(double w, double mu) {
    return SF_C_KMS / mu * fabs(w - mu);  // kernels.py:69
}
// The tile bodies inline both element formulas, 16 entries per lane: 66-70 KB of straight-line code per structured tile.
// As real calls the kernels were 15 KB with 143 instead of 163 VGPRs, the same bits, and no faster (round 6:
// profiles/r06_d_fill_called_elements_ab.txt): the kernel is bound by the latency of its fp64 chains.

// The hyper-parameters of walker P (= params + b * pstride), read in ONE place: an entry the matvec multiplies has the
// bits of the entry the fill adds only while both get these operands.  (k_band_fill / k_band_gtab keep their own
// reciprocal spellings, see sf_fill_band.h.)
struct sf_global_hyper {
    double amp, ls, r0;
};
__device__ __forceinline__ sf_global_hyper sf_load_global(const sf_fill_args& a, const double* __restrict__ P) {
    sf_global_hyper g;
    g.amp = exp(P[a.off_global]);     // spectrum_model.py:343
    g.ls = exp(P[a.off_global + 1]);  // spectrum_model.py:344
    g.r0 = 6 * g.ls;                  // kernels.py:29
    return g;
}
struct sf_local_hyper {
    double mu, amp, sig;  // cut-off radius: 4 sig (kernels.py:73)
};
__device__ __forceinline__ sf_local_hyper sf_load_local(const sf_fill_args& a, const double* __restrict__ P, int k) {
    sf_local_hyper l;
    l.mu = P[a.off_local + 3 * k];
    l.amp = exp(P[a.off_local + 3 * k + 1]);  // spectrum_model.py:356
    l.sig = exp(P[a.off_local + 3 * k + 2]);  // spectrum_model.py:357
    return l;
}

// Which structured kernels can reach the block rows [rlo, rhi] x columns [clo, chi] (indices < n)?  Conservative: the
// closest (row, column) pair in wavelength against the kernel's cut-off radius (kernels.py:29,73), with a 1e-9 margin.
// `g_r0` = 6 exp(log_ls) of the global kernel (unused without one).  The ONE support test: the 128 x 128 tile map of the
// factorisation, the fill tiles (32 x 32 wave sub-tiles), the 64 x 64 support map of the dense fill and the matvec's
// column blocks -- a tile a map leaves out has no sub-tile that is reached.
__device__ __forceinline__ void sf_block_support(const sf_fill_args& a, const double* __restrict__ P, int rlo, int rhi,
                                                 int clo, int chi, double g_r0, bool& do_glob, unsigned& lmask) {
    const bool on_diag = !(rlo > chi || clo > rhi);
    do_glob = false;
    lmask = 0;
    if (a.has_global) {
        do_glob = true;
        if (a.monotonic && !on_diag) {
            // closest (row, col) pair of the block in wavelength
            double wr, wc;
            if (rlo > chi) { wr = a.wave[rlo]; wc = a.wave[chi]; }
            else { wr = a.wave[rhi]; wc = a.wave[clo]; }
            const double rmin = SF_C_KMS / 2 * fabs((wc - wr) / (wc + wr));
            do_glob = rmin <= g_r0 * (1 + 1e-9);
        }
    }
    for (int k = 0; k < a.n_local; ++k) {
        bool hit = true;
        if (a.monotonic) {
            const sf_local_hyper l = sf_load_local(a, P, k);
            const double mu = l.mu, r0 = 4 * l.sig;
            auto dmin = [&](int lo, int hi) {  // smallest metric over an index range
                const double wl = a.wave[lo], wh = a.wave[hi];
                if (wl <= mu && mu <= wh) return 0.0;
                return fmin(sf_local_metric(wl, mu), sf_local_metric(wh, mu));
            };
            hit = (dmin(rlo, rhi) <= r0 * (1 + 1e-9)) && (dmin(clo, chi) <= r0 * (1 + 1e-9));
        }
        if (hit) lmask |= 1u << k;
    }
}

static int sf_check_n_local(const sf_fill_args& a) {  // the 32-bit masks of the tiles, the per-block table of the band fill
    if (a.n_local > SF_MAX_LOCAL) {
        sf_set_error("at most %d local kernels are supported", SF_MAX_LOCAL);
        return SF_EINVAL;
    }
    return SF_OK;
}
static int sf_check_fill_grid(long long nblk) {  // one workgroup per tile (segment): a one-dimensional grid
    if (nblk > 0x7fffffffLL) {
        sf_set_error("fill grid too large");
        return SF_EINVAL;
    }
    return SF_OK;
}
