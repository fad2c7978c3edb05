// Host numerics of the C-ABI layer: the collocation factor of the fixed log-lambda grid and its truncated inverse, twiddles,
// grid tests, the factor of the constant v11 and the tables of the spline-based extinction laws.  Host code only prepares
// constants that the reference recomputes on every call but that do not depend on the walker.  Plain C++: no HIP.
#include <cmath>

#include "sf_hostmath.h"

// ------------------------------------------------------------------- host-side spline set-up
// FITPACK knots of an interpolating k=5 spline through x[0..n): x0 x6, x[3:-3], x[n-1] x6.
void quintic_knots(const double* x, int n, std::vector<double>& t) {
    t.resize((size_t)n + 6);
    for (int i = 0; i < 6; ++i) t[i] = x[0];
    for (int j = 3; j <= n - 4; ++j) t[j + 3] = x[j];
    for (int i = 0; i < 6; ++i) t[n + i] = x[n - 1];
}
void bspl6_host(const double* t, int ell, double x, double h[6]) {
    double hh[5];
    h[0] = 1.0;
    for (int j = 1; j <= 5; ++j) {
        for (int i = 0; i < j; ++i) hh[i] = h[i];
        h[0] = 0.0;
        for (int i = 1; i <= j; ++i) {
            const int li = ell + i, lj = li - j;
            const double f = hh[i - 1] / (t[li] - t[lj]);
            h[i - 1] = h[i - 1] + f * (t[li] - x);
            h[i] = f * (x - t[lj]);
        }
    }
}
// Band LU (no pivoting; B-spline collocation matrices are totally positive) of A[i][j] = B_j(x_i).
// Outputs, per row j: Lf[j][k-1] = L[j][j-k], Uf[j][k-1] = U[j][j+k] (k = 1..SF_KB), rdiag[j] = 1/U[j][j].
int quintic_collocation_lu(const double* x, int n, std::vector<double>& t, std::vector<double>& Lf,
                           std::vector<double>& Uf, std::vector<double>& rdiag) {
    if (n < 6) {
        sf_set_error("resample needs at least 6 points, got %d", n);
        return SF_EINVAL;
    }
    for (int i = 1; i < n; ++i)
        if (!(x[i] > x[i - 1])) {
            sf_set_error("resample: the source grid must be strictly increasing");
            return SF_EINVAL;
        }
    quintic_knots(x, n, t);
    const int W = 2 * SF_KB + 1;
    std::vector<double> ab((size_t)n * W, 0.0);  // ab[i][col - i + KB]
    int ell = 5;
    for (int i = 0; i < n; ++i) {
        while (ell < n - 1 && t[ell + 1] <= x[i]) ++ell;
        double h[6];
        bspl6_host(t.data(), ell, x[i], h);
        for (int q = 0; q < 6; ++q) {
            const int col = ell - 5 + q;
            const int d = col - i + SF_KB;
            if (h[q] != 0.0) {
                if (d < 0 || d >= W) {
                    sf_set_error("collocation bandwidth exceeded at row %d", i);
                    return SF_EINVAL;
                }
                ab[(size_t)i * W + d] = h[q];
            }
        }
    }
    for (int k = 0; k < n; ++k) {
        const double piv = ab[(size_t)k * W + SF_KB];
        if (!(std::fabs(piv) > 0.0)) {
            sf_set_error("singular spline collocation matrix at row %d", k);
            return SF_EINVAL;
        }
        const int imax = (k + SF_KB < n - 1) ? k + SF_KB : n - 1;
        for (int i = k + 1; i <= imax; ++i) {
            double& lik = ab[(size_t)i * W + (k - i + SF_KB)];
            if (lik == 0.0) continue;
            lik /= piv;
            for (int j = k + 1; j <= imax; ++j) {
                const double ukj = ab[(size_t)k * W + (j - k + SF_KB)];
                if (ukj != 0.0) ab[(size_t)i * W + (j - i + SF_KB)] -= lik * ukj;
            }
        }
    }
    Lf.assign((size_t)n * SF_KB, 0.0);
    Uf.assign((size_t)n * SF_KB, 0.0);
    rdiag.resize(n);
    for (int j = 0; j < n; ++j) {
        rdiag[j] = 1.0 / ab[(size_t)j * W + SF_KB];
        for (int k = 1; k <= SF_KB; ++k) {
            if (j - k >= 0) Lf[(size_t)j * SF_KB + k - 1] = ab[(size_t)j * W + (SF_KB - k)];
            if (j + k < n) Uf[(size_t)j * SF_KB + k - 1] = ab[(size_t)j * W + (SF_KB + k)];
        }
    }
    return SF_OK;
}

// Truncated inverse of the collocation matrix from its band LU, by windowed column solves: column j of
// A^-1 is obtained with a forward sweep over [j, j+WF] and a backward sweep over [j-WF, j+WF] (entries
// further out are < 1e-30 of the peak).  band[(j - i + SF_IW) * n + i] = Ainv[i][j] for |i - j| <= SF_IW.
void truncated_inverse_band(int n, const std::vector<double>& Lf, const std::vector<double>& Uf,
                            const std::vector<double>& rdiag, std::vector<double>& band) {
    const int W = SF_IW, WF = SF_IW + 40;
    band.assign((size_t)(2 * W + 1) * n, 0.0);
    std::vector<double> yv(WF + 1), xv(2 * WF + 1);
    for (int j = 0; j < n; ++j) {
        const int hi = (j + WF < n - 1) ? j + WF : n - 1;
        const int lo = (j - WF > 0) ? j - WF : 0;
        yv[0] = 1.0;
        for (int i = j + 1; i <= hi; ++i) {
            double v = 0.0;
            for (int k = 1; k <= SF_KB && i - k >= j; ++k) v -= Lf[(size_t)i * SF_KB + k - 1] * yv[i - k - j];
            yv[i - j] = v;
        }
        // xv index: i - lo
        for (int i = hi; i >= lo; --i) {
            double v = (i >= j) ? yv[i - j] : 0.0;
            for (int k = 1; k <= SF_KB && i + k <= hi; ++k) v -= Uf[(size_t)i * SF_KB + k - 1] * xv[i + k - lo];
            xv[i - lo] = v * rdiag[i];
        }
        const int ilo = (j - W > 0) ? j - W : 0, ihi = (j + W < n - 1) ? j + W : n - 1;
        for (int i = ilo; i <= ihi; ++i) band[(size_t)(j - i + W) * n + i] = xv[i - lo];
    }
}
// 16 x 16 coefficient blocks for the MFMA band product (k_spline_apply): output block ib uses the
// input blocks ib-4 .. ib+4
void inverse_band_blocks(int n, const std::vector<double>& band, std::vector<double>& tblk) {
    const int nfb = n / 16, nkb = 2 * (SF_IW / 16) + 1;
    tblk.assign((size_t)nfb * nkb * 256, 0.0);
    for (int ib = 0; ib < nfb; ++ib)
        for (int kb = 0; kb < nkb; ++kb)
            for (int r = 0; r < 16; ++r)
                for (int cc = 0; cc < 16; ++cc) {
                    const int i = ib * 16 + r, k = (ib - SF_IW / 16 + kb) * 16 + cc;
                    if (k < 0 || k >= n || k - i > SF_IW || i - k > SF_IW) continue;
                    tblk[(((size_t)ib * nkb + kb) * 16 + r) * 16 + cc] = band[(size_t)(k - i + SF_IW) * n + i];
                }
}

void make_twiddles(int nf, std::vector<double>& tw) {
    tw.resize((size_t)nf);  // nf/2 complex values
    for (int k = 0; k < nf / 2; ++k) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)nf;
        tw[2 * k] = (double)cosl(ang);
        tw[2 * k + 1] = (double)sinl(ang);
    }
}

double min_dv(const double* w, int n) {  // Starfish/utils.py:22
    double best = INFINITY;
    for (int i = 0; i + 1 < n; ++i) {
        const double v = (w[i + 1] - w[i]) / w[i];
        if (v < best) best = v;
    }
    return SF_C_KMS * best;
}
// log-uniform grid?  (w_i - w_{i-1}) / (w_i + w_{i-1}) = tanh(delta/2) for every i, to the
// rounding of the wavelengths themselves (relative spread ~ ulp(w)/dw, e.g. 3e-11 at 5000 A, dv = 2)
bool is_loguniform(const double* w, int n) {
    double qmin = 1e300, qmax = 0.0;
    for (int i = 1; i < n; ++i) {
        const double q = (w[i] - w[i - 1]) / (w[i] + w[i - 1]);
        qmin = q < qmin ? q : qmin;
        qmax = q > qmax ? q : qmax;
    }
    return (qmax - qmin) <= 2e-10 * qmax;
}

// Cholesky of v11 and the constants derived from it (emulator.py:387-388 solves with the constant
// v11 on every call; here the factor is built once).
int emulator_constants(const double* v11, const double* w_hat, int N, std::vector<double>& alpha,
                       std::vector<double>& Linv) {
    std::vector<double> L((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i) {
        const double* ai = v11 + (size_t)i * N;
        double* li = &L[(size_t)i * N];
        for (int j = 0; j <= i; ++j) {
            const double* lj = &L[(size_t)j * N];
            double s = ai[j];
            for (int k = 0; k < j; ++k) s -= li[k] * lj[k];
            if (i == j) {
                if (!(s > 0.0)) {
                    sf_set_error("emulator v11 is not positive definite (row %d)", i);
                    return SF_EINVAL;
                }
                li[j] = std::sqrt(s);
            } else {
                li[j] = s / lj[j];
            }
        }
    }
    // W = Linv^T (row-major W[j][i] = Linv[i][j]) so the inner products run over contiguous memory
    std::vector<double> W((size_t)N * N, 0.0);
    for (int j = 0; j < N; ++j) {
        double* wj = &W[(size_t)j * N];
        for (int i = j; i < N; ++i) {
            const double* li = &L[(size_t)i * N];
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = j; k < i; ++k) s -= li[k] * wj[k];
            wj[i] = s / li[i];
        }
    }
    Linv.assign((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) Linv[(size_t)i * N + j] = W[(size_t)j * N + i];
    // alpha = Linv^T (Linv w_hat)
    std::vector<double> y(N, 0.0);
    for (int i = 0; i < N; ++i) {
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s += Linv[(size_t)i * N + j] * w_hat[j];
        y[i] = s;
    }
    alpha.assign(N, 0.0);
    for (int j = 0; j < N; ++j) {
        double s = 0.0;
        for (int i = j; i < N; ++i) s += W[(size_t)j * N + i] * y[i];
        alpha[j] = s;
    }
    return SF_OK;
}

// Anchor points of the spline-based laws (k = E(lambda - V)/E(B - V) at x = 1/lambda [um^-1]) and the second
// derivatives of the NATURAL cubic spline through them.  fitzpatrick99: Fitzpatrick (1999) section 5 / table 4 as
// coded in his FM_UNRED: optical anchors as polynomials in Rv, infrared ones scaled by Rv/3.1, two ultraviolet
// anchors from the FM90 curve with c2 = -0.824 + 4.717/Rv, c1 = 2.030 - 3.007 c2.  fm07: Fitzpatrick & Massa (2007)
// mean curve, defined for Rv = 3.1 only.  PARITY UNPINNED (see the header).
int extinct_spline_table(int law, double Rv, std::vector<double>& tab) {
    std::vector<double> xk, yk;
    double c1, c2, c3, c4, c5, x0, gam, f99;
    auto uv = [&](double x) {
        const double x2 = x * x;
        double k = c1 + c2 * x + c3 * x2 / ((x2 - x0 * x0) * (x2 - x0 * x0) + x2 * gam * gam);
        if (x >= c5) {
            const double y = x - c5;
            k += f99 != 0.0 ? c4 * (0.5392 * y * y + 0.05644 * y * y * y) : c4 * y * y;
        }
        return k;
    };
    if (law == 3) {
        x0 = 4.596, gam = 0.99, c3 = 3.23, c4 = 0.41, c5 = 5.9, f99 = 1.0;
        c2 = -0.824 + 4.717 / Rv;
        c1 = 2.030 - 3.007 * c2;
        xk = {0.0, 1e4 / 26500.0, 1e4 / 12200.0, 1e4 / 6000.0, 1e4 / 5470.0, 1e4 / 4670.0, 1e4 / 4110.0, 1e4 / 2700.0, 1e4 / 2600.0};
        const double r2 = Rv * Rv, r3 = r2 * Rv, r4 = r3 * Rv;
        yk = {-Rv,
              0.26469 * Rv / 3.1 - Rv,
              0.82925 * Rv / 3.1 - Rv,
              -4.22809e-01 + 1.00270 * Rv + 2.13572e-04 * r2 - Rv,
              -5.13540e-02 + 1.00216 * Rv - 7.35778e-05 * r2 - Rv,
              7.00127e-01 + 1.00184 * Rv - 3.32598e-05 * r2 - Rv,
              1.19456 + 1.01707 * Rv - 5.46959e-03 * r2 + 7.97809e-04 * r3 - 4.45636e-05 * r4 - Rv,
              uv(1e4 / 2700.0),
              uv(1e4 / 2600.0)};
    } else {
        if (std::fabs(Rv - 3.1) > 1e-12) {
            sf_set_error("fm07 is defined for Rv = 3.1 only");
            return SF_EINVAL;
        }
        x0 = 4.592, gam = 0.922, c1 = -0.175, c2 = 0.807, c3 = 2.991, c4 = 0.319, c5 = 6.097, f99 = 0.0;
        xk = {0.0, 0.25, 0.50, 0.75, 1.0, 1e4 / 5530.0, 1e4 / 4000.0, 1e4 / 3300.0, 1e4 / 2700.0, 1e4 / 2600.0};
        yk.resize(xk.size());
        for (int i = 0; i < 5; ++i) yk[i] = (-0.83 + 0.63 * Rv) * std::pow(xk[i], 1.84) - Rv;
        yk[5] = 0.0;
        yk[6] = 1.322;
        yk[7] = 2.055;
        yk[8] = uv(xk[8]);
        yk[9] = uv(xk[9]);
    }
    const int nk = (int)xk.size();
    // natural cubic spline: tridiagonal system for the second derivatives (y2[0] = y2[nk-1] = 0)
    std::vector<double> y2(nk, 0.0), u(nk, 0.0);
    for (int i = 1; i < nk - 1; ++i) {
        const double sig = (xk[i] - xk[i - 1]) / (xk[i + 1] - xk[i - 1]);
        const double pp = sig * y2[i - 1] + 2.0;
        y2[i] = (sig - 1.0) / pp;
        const double dd = (yk[i + 1] - yk[i]) / (xk[i + 1] - xk[i]) - (yk[i] - yk[i - 1]) / (xk[i] - xk[i - 1]);
        u[i] = (6.0 * dd / (xk[i + 1] - xk[i - 1]) - sig * u[i - 1]) / pp;
    }
    for (int i = nk - 2; i >= 1; --i) y2[i] = y2[i] * y2[i + 1] + u[i];
    tab = {(double)nk, c1, c2, c3, c4, c5, x0 * x0, gam * gam, f99};
    tab.insert(tab.end(), xk.begin(), xk.end());
    tab.insert(tab.end(), yk.begin(), yk.end());
    tab.insert(tab.end(), y2.begin(), y2.end());
    return SF_OK;
}
