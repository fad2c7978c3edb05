// Argument blocks of the transform / emulator kernels (internal).
#pragma once
#include "sf_common.h"

// (SF_KB, SF_IW: sf_base.h)
#define SF_MAX_M 32  // eigenspectra handled by the per-pixel rank-m factor kernel

struct sf_broaden_args {
    const double* in;      // rows x nf real input (free functions) or NULL
    const double2* spec;   // precomputed half spectra rows x (nf/2+1) (context path) when in == NULL
    int B, rows, nf;
    const double2* tw;     // exp(-2 pi i k / nf), k < nf/2
    double dv;
    int kind;              // 0 none, 1 rotational, 2 instrumental
    const double* params;  // per-item parameter rows (NULL -> scalar_param)
    int pstride, poff;
    double scalar_param;
    double* out;
    int64_t ob, orow, oelem;  // strides of the output: item, row, element
    double2* gscratch;     // B*rows*nf complex when nf does not fit the LDS
    double* mult;          // optional B x (nf/2+1) scratch (context path): per-walker multiplier table ->
                           // half-size FFT kernel
    int* info;
};
size_t sf_fft_scratch_bytes(int rows_total, int nf);
size_t sf_fft_half_scratch_bytes(int rows_total, int nf);
int sf_launch_broaden(const sf_broaden_args& a, hipStream_t s);
int sf_launch_rfft_rows(const double* in, int rows, int nf, const double2* tw, double2* spec,
                        double2* gscratch, hipStream_t s);
int sf_launch_spline_solve(double* data, int B, int rows, int64_t bstride, int64_t rstride,
                           int64_t estride, int n, const double* Lf, const double* Uf, const double* rdiag,
                           hipStream_t s);
// c = A^-1 y with the truncated (banded) inverse: y, c laid out [B][n][rows]; band[(2*SF_IW+1)][n]
int sf_launch_spline_apply(const double* y, double* c, int B, int rows, int n, const double* band, hipStream_t s);
int sf_launch_spline_eval(const double* coef, int rows, int ncoef, const double* t, const double* xq, int nq,
                          double* out, hipStream_t s);

struct sf_eval_args {
    const double* wave;    // [n] data wavelengths
    const double* knots;   // [nf + 6]
    const double* coef;    // [B?][nf][m+2] spline coefficients, row index fastest
    int coef_batched;      // 0: one static coefficient set shared by all walkers
    const double* params;
    const double* mu;      // [B][m] emulator weights
    double* X;             // [B][m][ldx]  unscaled eig*std rows
    double* flux;          // [B][ldx]     unscaled reconstruction
    const int* info;
    int n, nf, m, ldx, pstride, has_vz, n_cheb, off_cheb;
    int has_av, off_av;
    double wave_max;
};
int sf_launch_eval_rows(const sf_eval_args& a, int B, hipStream_t s);

struct sf_scale_args {
    const double* wave;
    const double* dflux;
    const double* flux;    // [B][ldx]
    const double* params;
    double* scale;         // [B]
    double* log_scale_out; // [B] or NULL
    int n, ldx, pstride, has_log_scale;
};
int sf_launch_scale(const sf_scale_args& a, int B, hipStream_t s);

struct sf_resid_args {
    const double* dflux;
    const double* flux;    // [B][ldx] unscaled
    const double* X;       // [B][m][ldx] unscaled
    const double* scale;   // [B]
    const double* Lw;      // [B][m][m] lower Cholesky factor of Sigma_w
    const int* info;
    double* resid;         // [B][ldx] or NULL
    double* Y;             // [B][mpad][ldy] or NULL
    double* flux_out;      // [B][n] or NULL
    double* X_out;         // [B][m][n] or NULL
    int n, m, mpad, ldx, ldy, use_sigma_w;
};
int sf_launch_resid_y(const sf_resid_args& a, int B, hipStream_t s);
// eval_rows + scale (given log_scale: spectrum_model.py:316-318) + resid_y in one pass: X and the flux never go through memory
// (e.X / e.flux / r.X / r.flux / r.scale are not used; `scale_out` [B] and `log_scale_out` [B] or NULL are written)
int sf_launch_eval_resid_y(const sf_eval_args& e, const sf_resid_args& r, double* scale_out, double* log_scale_out, int B,
                           hipStream_t s);

// sf_mean_grad.h: the likelihood's gradient in the mean-flux parameters, contracted from alpha = C^-1 r and
// V = C^-1 X^T (the staging area after SF_APPLY_CINV on the 1 + m right-hand sides sf_launch_mean_stage put there)
struct sf_emu_args;
struct sf_mean_grad_args {
    const double* stage;   // [B][1 + m][npad]: alpha, V_1 .. V_m
    const double* Xs;      // [B][m][n] scaled rows (sf_resid_args::X_out)
    const double* Lw;      // [B][m][m]
    const double* mu;      // [B][m]
    const double* scale;   // [B]
    const int* info;       // [B]: != 0 -> NaN row, nothing of the walker is read
    double* fin;           // [B][sf_mean_fin_doubles(m)]: z_a, Sigma_w^-1, Q, a, H
    double* part;          // sf_mean_grad_part_doubles(n, nslots, B)
    double* grad;          // [B][grad_stride]
    double* dcoef;         // [B][nf][m + 2]: spline coefficients of the d / d vsini rows (want_vsini)
    double* kdot;          // [ng][B][m M]: d v12 per grid column asked for
    double* mudot;         // [ng][B][m]
    double* zdot;          // [ng][B][m M][m]: Linv d v12
    int n, npad, m, nslots, grad_stride, want_vz, want_vsini, ng;
    int slots[SF_MEAN_GRAD_MAX_SLOTS];  // columns of the parameter row: 0 vsini, 1 vz, 2 log_scale, grid, cheb, Av
    int gcols[SF_MEAN_GRAD_MAX_SLOTS];  // the ng grid columns among them, in their order
};
static inline __host__ __device__ size_t sf_mean_fin_doubles(int m) { return 2 * (size_t)m + 3 * (size_t)m * m; }
size_t sf_mean_grad_part_doubles(int n, int nslots, int batch);
int sf_launch_mean_stage(const double* resid, const double* Xs, const int* info, int n, int npad, int m, int batch, double* stage,
                         hipStream_t s);
// the tangents that need no solve: a.dcoef (bro: the broadening's arguments as run_transforms fills them; its ybro, mult and FFT
// scratch are used once more) and a.kdot, a.mudot, a.zdot (e: the emulator's arguments); want_zdot == false leaves a.zdot alone
int sf_launch_mean_tangents(const sf_broaden_args& bro, const double* inv_band, const sf_emu_args& e, const sf_mean_grad_args& a,
                            int B, hipStream_t s, bool want_zdot = true);
// the moments, the pixel pass, the grid slots (z: the emulator's [B][mM][m]) and the sum over the blocks; e: the evaluation's
// arguments as run_transforms fills them
int sf_launch_mean_grad(const sf_eval_args& e, const sf_mean_grad_args& a, const double* z, int mM, int batch, hipStream_t s);

// sf_fisher.h: the Fisher information of the mean-flux parameters, F = J^T C^-1 J with the tangent columns J = d f / d theta.
// The columns of a's slots into rows[b * rstride + j * npad + i] (zero on the padding and where a.info[b] != 0; a.info: the
// transform chain's status), behind sf_launch_mean_tangents; of a only Xs, mu, scale, info, dcoef, mudot and the counts are read
int sf_launch_fisher_tangents(const sf_eval_args& e, const sf_mean_grad_args& a, double* rows, int64_t rstride, int batch,
                              hipStream_t s);
// band solver: [r; Y] into the first 1 + m of the nin rows of buf[b] (the columns follow); the leading nl x nl block of the
// nin x nin Gram matrices, compact; F = G_JJ - U^T U from the Gram matrix of [r; Y; J] (info: the final status, != 0 -> NaN)
int sf_launch_fisher_rows(const double* resid, const double* Y, int64_t sy, int n, int npad, int m, int nin, int batch, double* buf,
                          hipStream_t s);
int sf_launch_fisher_lead(const double* gram, int nin, int nl, int batch, double* lead, hipStream_t s);
int sf_launch_fisher_band(const double* gram, int m, int p, int batch, const int* info, double* fisher, int64_t fstride,
                          hipStream_t s);
// dense factor: F = Z^T Z for Z = L^-1 J, [B][p][npad]; part: sf_fisher_part_doubles(n, p, B)
size_t sf_fisher_part_doubles(int n, int nslots, int batch);
int sf_launch_fisher_ztz(const double* Z, int n, int npad, int p, int batch, const int* info, double* part, double* fisher,
                         int64_t fstride, hipStream_t s);
// sf_fisher_multi.h: all orders of a multi-order call.  The compact p x p blocks sf_launch_fisher_band leaves (fstride = p^2)
// into fisher[u * fstride + a * ld + b]; and the sum of the unit matrices over the orders (sf_multi_fisher_reduce)
int sf_launch_fisher_spread(const double* comp, int p, int batch, double* fisher, int ld, int64_t fstride, hipStream_t s);
struct sf_multi_fisher_reduce_args {
    const double* unit_lnl;     // [nseg * W]
    const int* unit_info;       // [nseg * W]
    const double* unit_fisher;  // [nseg * W][fisher_stride], rows of fisher_ld
    const int* col_ptr;         // [ncols + 1]
    const int* col_src;         // [col_ptr[ncols]][2]: (segment, slot), ascending in the segment within a column
    int nseg, W, fisher_ld, ncols;
    int64_t fisher_stride, out_stride;
    double* lnl;     // [W]
    double* fisher;  // [W][out_stride], rows of ncols
    int* info;       // [W]
};
int sf_launch_multi_fisher_reduce(const sf_multi_fisher_reduce_args& a, hipStream_t s);
// sf_local_scan_multi.h: per candidate the means of z and amp over the walkers with info == 0 (sf_local_scan_mean)
int sf_launch_local_scan_mean(int B, int ncand, const double* out, const int* info, double* mean, int* count, hipStream_t s);

int sf_launch_extinct_rows(const double* wave, int n, const double* flux, int rows, double Av, double Rv, int law,
                           double* out, hipStream_t s);  // law: 0 ccm89, 1 odonnell94, 2 calzetti00
int sf_launch_extinct_spline_rows(const double* wave, int n, const double* flux, int rows, double Av, double Rv,
                                  const double* d_table, double* out, hipStream_t s);  // law 3 / 4: table built by sf_extinct
int sf_launch_cheb_rows(const double* wave, int n, double wave_max, const double* flux, int rows,
                        const double* d_coeffs, int ncoef, double* out, hipStream_t s);

struct sf_emu_args {
    const double* params;
    int pstride, off_grid;
    int m, M, P;
    const double* grid;          // [M][P]
    const double* variances;     // [m]
    const double* lengthscales;  // [m][P]
    const double* gmin;          // [P]
    const double* gmax;          // [P]
    const double* alpha;         // [mM]   v11^-1 w_hat
    const double* LinvT;         // [mM][mM] TRANSPOSE of the inverse of the lower Cholesky factor of v11
    double* zscratch;            // [B][mM][m]
    double* kbuf;                // [B][mM] v12 blocks of every walker
    double* mu;                  // [B][m]
    double* cov;                 // [B][m][m] or NULL
    double* Lw;                  // [B][m][m] or NULL
    int* info;
};
int sf_launch_emulator(const sf_emu_args& a, int B, hipStream_t s);
int sf_launch_emu_joint(const sf_emu_args& a, int B, const double* mu_pts, double* mu, double* cov, hipStream_t s);
int sf_launch_finish(int B, const double* logdet, const double* sqmah, const int* info, const int* info2,
                     double* lnl, int* info_out, hipStream_t s);
int sf_launch_v11_build(const double* grid, int M, int P, int m, const double* hyper, const double* iphiphi, double* A, int npad,
                        int lda, hipStream_t s);
int sf_launch_v11_build_batch(const double* grid, int M, int P, int m, const double* hyper, int hyper_stride, int B,
                              const double* iphiphi, double* A, int npad, int lda, int64_t stride, int lower_only,
                              const double* w_hat, double* R, int ldr, hipStream_t s);
