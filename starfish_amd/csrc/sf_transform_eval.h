// Per-pixel evaluation: Chebyshev correction, the extinction laws, the fused Doppler-shifted spline evaluation and
// eigenspectrum reconstruction (sf_eval_pixel, k_eval_rows), the scale factor (k_scale), residual and rank-m factor Y
// (k_resid_y), and all three in one pass (k_eval_resid_y).   transforms.py:137-304; spectrum_model.py:293-335
#pragma once
#include "sf_device.h"
#include "sf_transform.h"
#include "sf_transform_spline.h"

// numpy.polynomial.chebyshev.chebval (Clenshaw) with coefficient vector [1, c1, c2, ...]
__device__ __forceinline__ double sf_chebval(double x, const double* __restrict__ c, int nc /* incl. c0 */,
                                             double c0first) {
    auto coef = [&](int i) { return i == 0 ? c0first : c[i - 1]; };
    double a0, a1;
    if (nc == 1) { a0 = coef(0); a1 = 0.0; }
    else if (nc == 2) { a0 = coef(0); a1 = coef(1); }
    else {
        const double x2 = 2 * x;
        a0 = coef(nc - 2);
        a1 = coef(nc - 1);
        for (int i = 3; i <= nc; ++i) {
            const double tmp = a0;
            a0 = coef(nc - i) - a1;
            a1 = tmp + a1 * x2;
        }
    }
    return a0 + a1 * x;
}

// Cardelli, Clayton & Mathis (1989) extinction law A(lambda)/A(V) = a(x) + b(x)/Rv, x = 1/lambda[um]
// (their eqs. 2a-5b).  Reference call site: extinct() Starfish/transforms.py:161-206 -> third-party
// `extinction.ccm89`; PARITY UNPINNED (that package is not available), checked against the paper's
// Table 3 only.  Returns the flux multiplier 10^(-0.4 Av (a + b/Rv)).
__device__ __forceinline__ double sf_ccm89_mult(double wave_A, double Av, double Rv) {
    const double x = 1e4 / wave_A;
    double a, b;
    if (x < 1.1) {
        const double p = pow(x, 1.61);
        a = 0.574 * p;
        b = -0.527 * p;
    } else if (x <= 3.3) {
        const double y = x - 1.82;
        a = 1 + y * (0.17699 + y * (-0.50447 + y * (-0.02427 + y * (0.72085 + y * (0.01979 + y * (-0.77530 + y * 0.32999))))));
        b = y * (1.41338 + y * (2.28305 + y * (1.07233 + y * (-5.38434 + y * (-0.62251 + y * (5.30260 + y * -2.09002))))));
    } else if (x <= 8.0) {
        double fa = 0.0, fb = 0.0;
        if (x >= 5.9) {
            const double d = x - 5.9;
            fa = -0.04473 * d * d - 0.009779 * d * d * d;
            fb = 0.2130 * d * d + 0.1207 * d * d * d;
        }
        a = 1.752 - 0.316 * x - 0.104 / ((x - 4.67) * (x - 4.67) + 0.341) + fa;
        b = -3.090 + 1.825 * x + 1.206 / ((x - 4.62) * (x - 4.62) + 0.263) + fb;
    } else {
        const double d = x - 8.0;
        a = -1.073 - 0.628 * d + 0.137 * d * d - 0.070 * d * d * d;
        b = 13.670 + 4.257 * d - 0.420 * d * d + 0.374 * d * d * d;
    }
    return pow(10.0, -0.4 * (Av * (a + b / Rv)));
}

// O'Donnell (1994, ApJ 422, 158): CCM89 with re-derived optical/NIR coefficients for 1.1 <= x <= 3.3 um^-1
// (continuous with the CCM infrared branch at x = 1.1: a = 0.6689, b = -0.6126); other ranges as CCM89.
// Calzetti et al. (2000, ApJ 533, 682), eq. 4: k(lambda) = 2.659 (-1.857 + 1.040/l) + Rv for
// 0.63 um <= l <= 2.2 um and 2.659 (-2.156 + 1.509/l - 0.198/l^2 + 0.011/l^3) + Rv for 0.12 um <= l < 0.63 um,
// A_lambda = Av k / Rv (k(0.55 um) = Rv).  Outside 0.12 - 2.2 um the nearer branch is extrapolated.
// Both PARITY UNPINNED like ccm89 (literature formulas; the reference's `extinction` package is unavailable).
__device__ __forceinline__ double sf_extinct_mult(double wave_A, double Av, double Rv, int law) {
    if (law == 1) {
        const double x = 1e4 / wave_A;
        if (x >= 1.1 && x <= 3.3) {
            const double y = x - 1.82;
            const double a = 1 + y * (0.104 + y * (-0.609 + y * (0.701 + y * (1.137 + y * (-1.718 + y * (-0.827 + y * (1.647 + y * -0.505)))))));
            const double b = y * (1.952 + y * (2.908 + y * (-3.989 + y * (-7.985 + y * (11.102 + y * (5.491 + y * (-10.805 + y * 3.347)))))));
            return pow(10.0, -0.4 * (Av * (a + b / Rv)));
        }
        return sf_ccm89_mult(wave_A, Av, Rv);
    }
    if (law == 2) {
        const double l = wave_A * 1e-4;  // micron
        const double il = 1.0 / l;
        const double k = (l >= 0.63) ? 2.659 * (-1.857 + 1.040 * il) + Rv
                                     : 2.659 * (-2.156 + il * (1.509 + il * (-0.198 + il * 0.011))) + Rv;
        return pow(10.0, -0.4 * (Av * k / Rv));
    }
    return sf_ccm89_mult(wave_A, Av, Rv);
}

__global__ __launch_bounds__(256) void k_extinct_rows(const double* __restrict__ wave, int n,
                                                      const double* __restrict__ flux, int rows, double Av,
                                                      double Rv, int law, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double mlt = sf_extinct_mult(wave[i], Av, Rv, law);
    for (int r = 0; r < rows; ++r) out[(int64_t)r * n + i] = flux[(int64_t)r * n + i] * mlt;
}

int sf_launch_extinct_rows(const double* wave, int n, const double* flux, int rows, double Av, double Rv, int law,
                           double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_extinct_rows, dim3((n + 255) / 256), dim3(256), 0, s, wave, n, flux, rows, Av, Rv, law, out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Spline-based laws: Fitzpatrick (1999, PASP 111, 63) and Fitzpatrick & Massa (2007, ApJ 663, 320).  k(x) =
// E(lambda - V)/E(B - V) is a natural cubic spline through a handful of anchor points in x = 1/lambda [um^-1] up to
// 1e4/2700 and the Fitzpatrick-Massa ultraviolet parametrisation beyond; A_lambda = Av (1 + k / Rv).  The anchors,
// their second derivatives (host: sf_extinct) and the UV constants arrive in `p`:
//   p[0] = number of knots nk, p[1..7] = c1, c2, c3, c4, c5, x0^2, gamma^2, p[8] = 1 for the F99 far-UV term
//   (0.5392 y^2 + 0.05644 y^3) / 0 for FM07's y^2, then xk[nk], yk[nk], y2[nk].   PARITY UNPINNED like the others.
__global__ __launch_bounds__(256) void k_extinct_spline_rows(const double* __restrict__ wave, int n,
                                                             const double* __restrict__ flux, int rows, double Av,
                                                             double Rv, const double* __restrict__ p,
                                                             double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int nk = (int)p[0];
    const double* xk = p + 9;
    const double* yk = xk + nk;
    const double* y2 = yk + nk;
    const double x = 1e4 / wave[i];
    double k;
    if (x >= xk[nk - 2]) {  // ultraviolet: lambda <= 2700 A (the last two knots are UV points themselves)
        const double x2 = x * x;
        const double d = x2 / ((x2 - p[6]) * (x2 - p[6]) + x2 * p[7]);
        k = p[1] + p[2] * x + p[3] * d;
        if (x >= p[5]) {
            const double y = x - p[5];
            k += p[8] != 0.0 ? p[4] * (0.5392 * y * y + 0.05644 * y * y * y) : p[4] * y * y;
        }
    } else {
        int lo = 0;
        while (lo + 2 < nk && x >= xk[lo + 1]) ++lo;
        const double h = xk[lo + 1] - xk[lo];
        const double a = (xk[lo + 1] - x) / h, b = (x - xk[lo]) / h;
        k = a * yk[lo] + b * yk[lo + 1] + ((a * a * a - a) * y2[lo] + (b * b * b - b) * y2[lo + 1]) * (h * h) / 6.0;
    }
    const double mlt = pow(10.0, -0.4 * (Av * (1.0 + k / Rv)));
    for (int r = 0; r < rows; ++r) out[(int64_t)r * n + i] = flux[(int64_t)r * n + i] * mlt;
}

int sf_launch_extinct_spline_rows(const double* wave, int n, const double* flux, int rows, double Av, double Rv,
                                  const double* d_table, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_extinct_spline_rows, dim3((n + 255) / 256), dim3(256), 0, s, wave, n, flux, rows, Av, Rv, d_table, out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Fused: Doppler-scaled spline evaluation of the m+2 rows, Chebyshev multiply, reconstruction.
// the m + 2 rows at pixel i: xk[k] = eig_k * std (spectrum_model.py:312), returns the reconstruction sum_k w_k xk + mean
__device__ __forceinline__ double sf_eval_pixel(const sf_eval_args& a, int b, int i, double* xk) {
    const double* __restrict__ P = a.params + (int64_t)b * a.pstride;
    const double x = a.wave[i];
    double s = 1.0;
    if (a.has_vz) {
        const double vz = P[1];
        s = sqrt((SF_C_KMS + vz) / (SF_C_KMS - vz));  // transforms.py:157
    }
    const int ell = sf_find_interval(a.knots, s, a.nf, x);
    double h[6];
    sf_bspl6(a.knots, s, ell, x, h);
    const int rows = a.m + 2;
    const double* __restrict__ cf =
        (a.coef_batched ? a.coef + (int64_t)b * a.nf * rows : a.coef) + (int64_t)(ell - 5) * rows;
    double p = 1.0;
    if (a.n_cheb > 0) p = sf_chebval(x / a.wave_max, P + a.off_cheb, a.n_cheb + 1, 1.0);  // transforms.py:302-304
    double ext = 1.0;
    if (a.has_av) ext = sf_ccm89_mult(x, P[a.off_av], 3.1);  // spectrum_model.py:298-299 (Rv never passed)
    auto rowval = [&](int r) {
        double sp = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) sp = sp + cf[(int64_t)j * rows + r] * h[j];
        if (a.has_av) sp = sp * ext;  // extinct before the Chebyshev correction, as the reference orders them
        return a.n_cheb > 0 ? sp * p : sp;
    };
    const double mean = rowval(a.m), std = rowval(a.m + 1);
    const double* __restrict__ wmu = a.mu + (int64_t)b * a.m;
    double flux = 0.0;
    for (int k = 0; k < a.m; ++k) {
        xk[k] = rowval(k) * std;            // spectrum_model.py:312
        flux = flux + wmu[k] * xk[k];       // spectrum_model.py:313
    }
    return flux + mean;
}
// rank-m factor row at one pixel: xs (scaled X column) -> Y column, zero padded   (k_resid_y, k_eval_resid_y)
__device__ __forceinline__ void sf_y_column(const sf_resid_args& a, int b, int i, double* xs, double* __restrict__ Yb) {
    const double* __restrict__ Lw = a.Lw + (int64_t)b * a.m * a.m;
    if (!a.use_sigma_w) {
        // forward substitution Lw y = x  ->  y^T y = x^T Sigma_w^-1 x   (spectrum_model.py:334-335)
        for (int k = 0; k < a.m; ++k) {
            double v = xs[k];
            for (int j = 0; j < k; ++j) v -= Lw[k * a.m + j] * xs[j];
            xs[k] = v / Lw[k * a.m + k];
            Yb[(int64_t)k * a.ldy + i] = xs[k];
        }
    } else {
        // y = Lw^T x  ->  y^T y = x^T Sigma_w x   (the form printed in the paper / docs)
        for (int k = 0; k < a.m; ++k) {
            double v = 0.0;
            for (int j = k; j < a.m; ++j) v += Lw[j * a.m + k] * xs[j];
            Yb[(int64_t)k * a.ldy + i] = v;
        }
    }
    for (int k = a.m; k < a.mpad; ++k) Yb[(int64_t)k * a.ldy + i] = 0.0;
}

__global__ __launch_bounds__(256) void k_eval_rows(sf_eval_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.n) return;
    if (a.info && a.info[b] != 0) return;
    double xk[SF_MAX_M];
    const double flux = sf_eval_pixel(a, b, i, xk);
    double* __restrict__ Xb = a.X + (int64_t)b * a.m * a.ldx;
    for (int k = 0; k < a.m; ++k) Xb[(int64_t)k * a.ldx + i] = xk[k];
    a.flux[(int64_t)b * a.ldx + i] = flux;
}

int sf_launch_eval_rows(const sf_eval_args& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_eval_rows, dim3((a.n + 255) / 256, B), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

__device__ __forceinline__ double sf_block_sum(double v, double* red) {
    v = sf_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += red[w];
    return tot;
}

// One workgroup per walker: scale factor Omega (spectrum_model.py:316-329, transforms.py:265-268)
__global__ __launch_bounds__(256) void k_scale(sf_scale_args a) {
    __shared__ double red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ P = a.params + (int64_t)b * a.pstride;
    const double norm = P[3];
    double scale, lscale;
    if (a.has_log_scale) {
        lscale = P[2];
        scale = exp(lscale) * norm;
    } else {
        const double* __restrict__ f = a.flux + (int64_t)b * a.ldx;
        double sd = 0.0, sm = 0.0;
        for (int i = tid; i + 1 < a.n; i += 256) {
            const double d = a.wave[i + 1] - a.wave[i];
            sd += d * (a.dflux[i + 1] + a.dflux[i]) / 2.0;
            sm += d * (f[i + 1] * norm + f[i] * norm) / 2.0;
        }
        sd = sf_block_sum(sd, red);
        sm = sf_block_sum(sm, red);
        scale = sd / sm;
        lscale = log(scale);
        scale = scale * norm;
    }
    if (tid == 0) {
        a.scale[b] = scale;
        if (a.log_scale_out) a.log_scale_out[b] = lscale;
    }
}

int sf_launch_scale(const sf_scale_args& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(k_scale, dim3(B), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

static int sf_check_max_m(int m) {  // the per-thread X column of the two kernels
    if (m > SF_MAX_M) {
        sf_set_error("at most %d eigenspectra are supported", SF_MAX_M);
        return SF_EINVAL;
    }
    return SF_OK;
}

// Elementwise: rescale flux and X, residual, and Y = Lw^-1 X (or Lw^T X), zero padded.
__global__ __launch_bounds__(256) void k_resid_y(sf_resid_args a) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.ldy) return;
    double* __restrict__ Yb = a.Y ? a.Y + (int64_t)b * a.mpad * a.ldy : nullptr;
    if (i >= a.n || (a.info && a.info[b] != 0)) {
        if (Yb)
            for (int k = 0; k < a.mpad; ++k) Yb[(int64_t)k * a.ldy + i] = 0.0;
        if (i < a.ldx && a.resid) a.resid[(int64_t)b * a.ldx + i] = 0.0;
        return;
    }
    const double sc = a.scale[b];
    const double f = a.flux[(int64_t)b * a.ldx + i] * sc;  // transforms.py:231
    if (a.flux_out) a.flux_out[(int64_t)b * a.n + i] = f;
    if (a.resid) a.resid[(int64_t)b * a.ldx + i] = f - a.dflux[i];  // spectrum_model.py:402
    const double* __restrict__ Xb = a.X + (int64_t)b * a.m * a.ldx;
    double xs[SF_MAX_M];
    for (int k = 0; k < a.m; ++k) {
        xs[k] = Xb[(int64_t)k * a.ldx + i] * sc;
        if (a.X_out) a.X_out[((int64_t)b * a.m + k) * a.n + i] = xs[k];
    }
    if (!Yb) return;
    sf_y_column(a, b, i, xs, Yb);
}

int sf_launch_resid_y(const sf_resid_args& a, int B, hipStream_t s) {
    SF_CHECK(sf_check_max_m(a.m));
    hipLaunchKernelGGL(k_resid_y, dim3((a.ldy + 255) / 256, B), dim3(256), 0, s, a);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// k_eval_rows + k_scale (log_scale given) + k_resid_y in one pass over the pixels: the same operations in the same order, X and
// the unscaled flux stay in registers (banded step, B = 128: 75 + 6 + 50 us of launches -> one)
__global__ __launch_bounds__(256) void k_eval_resid_y(sf_eval_args e, sf_resid_args a, double* __restrict__ scale_out,
                                                      double* __restrict__ log_scale_out) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    const double* __restrict__ P = e.params + (int64_t)b * e.pstride;
    const double lscale = P[2], sc = exp(lscale) * P[3];  // (k_scale: scale = exp(log_scale) * norm)
    if (i == 0) {
        scale_out[b] = sc;
        if (log_scale_out) log_scale_out[b] = lscale;
    }
    if (i >= a.ldy) return;
    double* __restrict__ Yb = a.Y ? a.Y + (int64_t)b * a.mpad * a.ldy : nullptr;
    if (i >= a.n || (e.info && e.info[b] != 0)) {
        if (Yb)
            for (int k = 0; k < a.mpad; ++k) Yb[(int64_t)k * a.ldy + i] = 0.0;
        if (i < a.ldx && a.resid) a.resid[(int64_t)b * a.ldx + i] = 0.0;
        return;
    }
    double xs[SF_MAX_M];
    const double f = sf_eval_pixel(e, b, i, xs) * sc;  // transforms.py:231
    if (a.flux_out) a.flux_out[(int64_t)b * a.n + i] = f;
    if (a.resid) a.resid[(int64_t)b * a.ldx + i] = f - a.dflux[i];  // spectrum_model.py:402
    for (int k = 0; k < a.m; ++k) {
        xs[k] = xs[k] * sc;
        if (a.X_out) a.X_out[((int64_t)b * a.m + k) * a.n + i] = xs[k];
    }
    if (!Yb) return;
    sf_y_column(a, b, i, xs, Yb);
}

int sf_launch_eval_resid_y(const sf_eval_args& e, const sf_resid_args& r, double* scale_out, double* log_scale_out, int B,
                           hipStream_t s) {
    SF_CHECK(sf_check_max_m(r.m));
    hipLaunchKernelGGL(k_eval_resid_y, dim3((r.ldy + 255) / 256, B), dim3(256), 0, s, e, r, scale_out, log_scale_out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}

// Chebyshev free function
__global__ __launch_bounds__(256) void k_cheb_rows(const double* __restrict__ wave, int n, double wave_max,
                                                   const double* __restrict__ flux, int rows,
                                                   const double* __restrict__ coeffs, int ncoef,
                                                   double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double p = sf_chebval(wave[i] / wave_max, coeffs + 1, ncoef, coeffs[0]);
    for (int r = 0; r < rows; ++r) out[(int64_t)r * n + i] = flux[(int64_t)r * n + i] * p;
}

int sf_launch_cheb_rows(const double* wave, int n, double wave_max, const double* flux, int rows,
                        const double* d_coeffs, int ncoef, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_cheb_rows, dim3((n + 255) / 256), dim3(256), 0, s, wave, n, wave_max, flux, rows,
                       d_coeffs, ncoef, out);
    SF_LAUNCH_CHECK();
    return SF_OK;
}
