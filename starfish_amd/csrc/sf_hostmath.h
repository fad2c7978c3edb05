// Host numerics of the C-ABI layer (internal): constants the reference recomputes on every call but that do not depend
// on the walker.  Plain C++, no HIP: tests/test_hostmath.py compiles sf_hostmath.cpp on its own with the host compiler.
#pragma once
#include <vector>

#include "sf_base.h"

#pragma GCC visibility push(hidden)  // shared between the host layer's translation units, not part of the library's surface
// FITPACK knots of an interpolating k=5 spline through x[0..n): x0 x6, x[3:-3], x[n-1] x6.
void quintic_knots(const double* x, int n, std::vector<double>& t);
void bspl6_host(const double* t, int ell, double x, double h[6]);
// Band LU (no pivoting; B-spline collocation matrices are totally positive) of A[i][j] = B_j(x_i).
// Outputs, per row j: Lf[j][k-1] = L[j][j-k], Uf[j][k-1] = U[j][j+k] (k = 1..SF_KB), rdiag[j] = 1/U[j][j].
int quintic_collocation_lu(const double* x, int n, std::vector<double>& t, std::vector<double>& Lf, std::vector<double>& Uf,
                           std::vector<double>& rdiag);
// Truncated inverse of the collocation matrix from its band LU: band[(j - i + SF_IW) * n + i] = Ainv[i][j], |i - j| <= SF_IW
void truncated_inverse_band(int n, const std::vector<double>& Lf, const std::vector<double>& Uf, const std::vector<double>& rdiag,
                            std::vector<double>& band);
// ... repacked into 16 x 16 coefficient blocks for the MFMA band product (k_spline_apply); n a multiple of 16
void inverse_band_blocks(int n, const std::vector<double>& band, std::vector<double>& tblk);
void make_twiddles(int nf, std::vector<double>& tw);  // exp(-2 pi i k / nf), k < nf/2
double min_dv(const double* w, int n);                // Starfish/utils.py:22
bool is_loguniform(const double* w, int n);           // w strictly increasing, n > 2
// Cholesky of v11 -> alpha = v11^-1 w_hat and Linv = Lc^-1 (row-major, lower)
int emulator_constants(const double* v11, const double* w_hat, int N, std::vector<double>& alpha, std::vector<double>& Linv);
// Table of the spline-based extinction laws (3 fitzpatrick99, 4 fm07): nk, c1..c5, x0^2, gamma^2, f99, then x, y, y''
int extinct_spline_table(int law, double Rv, std::vector<double>& tab);
#pragma GCC visibility pop
