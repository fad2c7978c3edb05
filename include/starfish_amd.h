/*
 * starfish_amd.h -- C-ABI of the MI355X (gfx950) implementation of the Starfish per-MCMC-step
 * log-likelihood path.
 *
 * The reference (Starfish-develop/Starfish v0.4.2) is pure Python and has NO FFI / plugin layer
 * for this path: its boundary is the Python object API (SpectrumModel / Emulator and the free
 * functions of Starfish.transforms / Starfish.models.kernels).  This header is therefore the
 * boundary a maintainer would bind with ctypes; every entry point cites the
 * reference function it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C, extern "C"; no torch / C++ types in any signature;
 *   - every `d_*` argument is a DEVICE pointer to C-contiguous fp64 (or int32) owned by the
 *     caller (e.g. torch.Tensor.data_ptr()); `h_*` arguments are HOST pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only ENQUEUE work,
 *     they never synchronise -- the caller synchronises the stream before reading results;
 *   - no allocation inside hot calls: scratch comes from the caller through the *_workspace_bytes
 *     queries;
 *   - return value: 0 = ok, <0 = SF_E* (bad argument / HIP failure).  Per-item numerical status is
 *     reported LAPACK-style in `d_info[b]`: 0 ok, k>0 = order of the first non-positive pivot,
 *     <0 = SF_INFO_* (parameter outside the emulator grid, non-positive vsini, ...).
 *   - all matrices are row-major; the Cholesky factor is the LOWER triangle (A = L L^T), the strict
 *     upper triangle is not referenced.
 *   - the batched Cholesky forks part of its launches onto side streams (lookahead, slab groups) and
 *     joins them back to `stream` with events before returning: from the caller's point of view all
 *     work is ordered on `stream`.  Those streams and their event pool belong to the CONTEXT (to the
 *     calling thread for the context-free entry points): different contexts may be driven from
 *     different host threads, and live on different devices, concurrently; ONE context is not
 *     re-entrant (like the reference's model object).  Every context call makes the context's device
 *     current for the calling thread.  Only the bench timing hooks (sf_profile_*) are process-global
 *     (mutex-protected).
 *   - the library reads NO environment variable.  (The test and tracing switches named in starfish_amd/csrc --
 *     SF_DF_* fault and trace aids, SF_TRANSFORM_UNFUSED, SF_BAND_TILES_POISON, SF_WIDE_STAMPS, SF_DIAG_STAMPS -- exist
 *     only in the separate development build `make -C starfish_amd/csrc TUNING=1` (-DSF_TUNING ->
 *     libstarfish_amd_tuning.so), which tools/ and two GPU tests load on purpose; the shipped libstarfish_amd.so
 *     contains no getenv and none of their names: tests/test_host_logic.py checks the binary.)
 */
#ifndef STARFISH_AMD_H
#define STARFISH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_OK 0
#define SF_EINVAL (-1)  /* bad argument */
#define SF_ENOMEM (-2)  /* workspace too small / allocation failure */
#define SF_EHIP (-3)    /* a HIP runtime call failed (sf_last_error() has the text) */
#define SF_ENODEV (-4)  /* no gfx950 device visible */

/* per-item d_info codes (<0) */
#define SF_INFO_OUT_OF_GRID (-1) /* emulator queried outside its grid: emulator.py:377-378 */
#define SF_INFO_BAD_VSINI (-2)   /* vsini <= 0: transforms.py:121-122 */
#define SF_INFO_BAD_WEIGHT_COV (-3) /* Sigma_w not positive definite: spectrum_model.py:334 */
#define SF_INFO_BANDWIDTH (-4)   /* banded solver only: covariance support wider than the given half-width */
#define SF_INFO_INTERNAL (-5)    /* a bounded wait between workgroups / waves of ONE launch gave up: the banded sweep's wave
                                    synchronisation, or the persistent-kernel Cholesky (the default sequence of small batches)
                                    -- there EVERY matrix of the call carries the code and no result of the call is valid.
                                    Never seen on a device the process has to itself (the schedule is live by construction);
                                    on a device SHARED with other processes the launch stalls when workgroups that hold claimed
                                    tasks are kept from running, and is given up after 25 ms without a single completed task
                                    (or 4 s in any one wait): see sf_persistent_potrf / sf_persistent_potrf_status.  Callers
                                    recover by sf_persistent_potrf(0) and re-running the batch (starfish_amd/_runtime.py does,
                                    with a warning); it is never to be treated as a rejected walker */

#define SF_INFO_NAN (-6)         /* the likelihood came out NaN although every stage reported success: lnl = -inf, but
                                    distinguishable from a legitimately rejected walker */

#define SF_JITTER 1e-10 /* spectrum_model.py:399 */

const char* sf_version(void);
const char* sf_last_error(void);
/* number of visible HIP devices (0 when none); never fails */
int sf_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Stand-alone stage entry points (used by the drop-in free functions and stage parity tests)
 * ---------------------------------------------------------------------------------------- */

/* Starfish/models/kernels.py:7-41  global_covariance_matrix(wave, amplitude, lengthscale)
 * d_out[n*n] = Hann-tapered Matern-3/2 in velocity distance (overwritten, full matrix). */
int sf_global_cov(const double* d_wave, int n, double amplitude, double lengthscale,
                  double* d_out, void* stream);

/* Starfish/models/kernels.py:44-81  local_covariance_matrix(wave, amplitude, mu, sigma)
 * accumulate != 0 adds into d_out (the sum over kernels of spectrum_model.py:353-360). */
int sf_local_cov(const double* d_wave, int n, double amplitude, double mu, double sigma,
                 int accumulate, double* d_out, void* stream);

/* Starfish/transforms.py:93-134  rotational_broaden(wave, flux, vsini); dv = calculate_dv(wave)
 * (Starfish/utils.py:8-22).  d_flux / d_out: rows x nf, nf a power of two.
 * d_work: sf_fft_workspace_bytes(rows, nf). */
int sf_rotational_broaden(const double* d_flux, int rows, int nf, double dv, double vsini,
                          double* d_out, void* d_work, size_t work_bytes, void* stream);

/* Starfish/transforms.py:45-90  instrumental_broaden(wave, flux, fwhm) */
int sf_instrumental_broaden(const double* d_flux, int rows, int nf, double dv, double fwhm,
                            double* d_out, void* d_work, size_t work_bytes, void* stream);

size_t sf_fft_workspace_bytes(int rows, int nf);

/* Starfish/transforms.py:11-42  resample(wave, flux, new_wave): interpolating k=5 spline
 * (FITPACK knots x[0]x6, x[3:-3], x[-1]x6) per row, evaluated at new_wave.
 * h_wave[n] is a HOST pointer (the collocation factor is built on the host once per grid);
 * d_flux rows x n, d_new_wave[nq], d_out rows x nq (nq = 0: both may be null).  d_work: sf_resample_workspace_bytes. */
int sf_resample(const double* h_wave, int n, const double* d_flux, int rows,
                const double* d_new_wave, int nq, double* d_out, void* d_work,
                size_t work_bytes, void* stream);
size_t sf_resample_workspace_bytes(int n, int rows);

/* Starfish/transforms.py:271-304  chebyshev_correct(wave, flux, coeffs): flux * chebval(
 * wave / wave_max, coeffs); h_coeffs[ncoef] is a HOST pointer (c0 must be 1 for 1-D use). */
int sf_chebyshev_correct(const double* d_wave, int n, double wave_max, const double* d_flux,
                         int rows, const double* h_coeffs, int ncoef, double* d_out,
                         void* stream);

/* Starfish/transforms.py:161-206  extinct(wave, flux, Av, Rv, law="ccm89"): flux * 10^(-0.4 A_lambda),
 * A_lambda = Av (a(x) + b(x)/Rv) from Cardelli, Clayton & Mathis (1989).  PARITY UNPINNED (the
 * reference calls the third-party `extinction` package); only the default law is provided. */
int sf_extinct_ccm89(const double* d_wave, int n, const double* d_flux, int rows, double Av, double Rv,
                     double* d_out, void* stream);
/* same with a choice of law: 0 = ccm89, 1 = odonnell94 (O'Donnell 1994: CCM89 with new optical/NIR
 * coefficients), 2 = calzetti00 (Calzetti et al. 2000, eq. 4), 3 = fitzpatrick99 (Fitzpatrick 1999: natural cubic
 * spline through Rv-dependent anchors + FM90 ultraviolet curve), 4 = fm07 (Fitzpatrick & Massa 2007, Rv = 3.1 only).
 * All PARITY UNPINNED (literature formulas).  Laws 3 and 4 synchronise the stream (a small table is uploaded). */
int sf_extinct(const double* d_wave, int n, const double* d_flux, int rows, double Av, double Rv, int law,
               double* d_out, void* stream);

/* scipy.linalg.cho_factor call site Starfish/models/spectrum_model.py:400 (LAPACK dpotrf).
 * In-place batched lower Cholesky of `batch` matrices, matrix b at d_A + b*stride (doubles),
 * n must be a multiple of 64 (callers pad with an identity block), row stride lda.
 * Layout contract: d_A 16-byte aligned, lda >= n and even, stride even (every matrix base is then 16-byte aligned: the
 * panel kernels fetch 16-byte granules) and stride >= (n - 1) lda + n (the matrices are factorised concurrently in place,
 * so no two may share an element; stride = n lda is the usual choice, a larger one leaves a gap).  Only the lower triangle
 * (diagonal included) is read; the strict upper triangle is undefined afterwards; the columns n .. lda of a row, the gaps
 * between matrices and everything outside [d_A, d_A + (batch - 1) stride + (n - 1) lda + n) are neither read into a result
 * nor written.  The workspace needs no initialisation and may be reused from call to call.
 * d_work: sf_potrf_workspace_bytes(n, batch).  d_info[batch]: 0, or the 1-based index of the first non-positive pivot; the
 * factor's columns left of that pivot are those of the successful factorisation.
 * SF_EINVAL before anything is enqueued: a null d_A, d_info or d_work, n not a positive multiple of 64, lda < n or odd,
 * batch < 1, stride odd or below (n - 1) lda + n, work_bytes below sf_potrf_workspace_bytes(n, batch). */
int sf_potrf_batch(double* d_A, int n, int lda, int64_t stride, int batch, int* d_info,
                   void* d_work, size_t work_bytes, void* stream);
size_t sf_potrf_workspace_bytes(int n, int batch);

/* Starfish/models/spectrum_model.py:401-404: logdet = 2 sum log L_ii and sqmah = R^T C^-1 R
 * = |L^-1 R|^2 (one forward substitution; the reference's cho_solve does two).
 * d_L as left by sf_potrf_batch; d_R: batch x ldr (ldr >= n, padded entries zero);
 * d_work: sf_potrf_workspace_bytes(n, batch) (only touched when n*8 bytes exceed the LDS: from n = 16256 on, where a
 * missing or short workspace is refused with SF_ENOMEM; below that d_work may be NULL).  Only the lower triangle of d_L is
 * read.  SF_EINVAL before anything is enqueued: a null d_L, d_R, d_logdet or d_sqmah, n not a multiple of 64, batch < 1,
 * ldr < n. */
int sf_logdet_sqmah_batch(const double* d_L, int n, int lda, int64_t stride, int batch,
                          const double* d_R, int ldr, void* d_work, size_t work_bytes,
                          double* d_logdet, double* d_sqmah, void* stream);

/* scipy.linalg.cho_solve call site Starfish/models/spectrum_model.py:404 (LAPACK dpotrs), and the factor on its own:
 * applies the L left by sf_potrf_batch (same n, lda, stride; only the lower triangle is read) to nrhs right-hand sides
 * per matrix.  op: */
#define SF_APPLY_L 0     /* L Z                                        */
#define SF_APPLY_LINV 1  /* L^-1 B  (forward substitution)             */
#define SF_APPLY_LINVT 2 /* L^-T B  (back substitution)                */
#define SF_APPLY_CINV 3  /* L^-T L^-1 B = (L L^T)^-1 B  (cho_solve)    */
/* Right-hand side r of matrix b: d_rhs + b*rhs_stride + r*ldr, its n rows contiguous (the layout of
 * sf_band_logdet_gram_batch's d_rhs); rhs_stride == 0: one block of right-hand sides shared by every matrix.  Results in
 * the same layout at d_out (ldo, out_stride).  d_out may be d_rhs when rhs_stride != 0, ldo == ldr and out_stride ==
 * rhs_stride; any other overlap is the caller's error.  No workspace.  SF_EINVAL before anything is enqueued: n not a
 * positive multiple of 64, lda < n, ldr < n, ldo < n, nrhs < 1, batch < 1, unknown op, null pointers, d_out == d_rhs with
 * rhs_stride == 0 or differing strides.  Componentwise backward stable (Higham, Accuracy and Stability of Numerical
 * Algorithms, Thms 8.5 and 10.4 with gamma_n). */
int sf_potrs_batch(const double* d_L, int n, int lda, int64_t stride, int batch, int op, const double* d_rhs, int nrhs,
                   int ldr, int64_t rhs_stride, double* d_out, int ldo, int64_t out_stride, void* stream);

/* The diagonal of the inverse from the factor (LAPACK dpotri, of which only the diagonal is formed): d_out[b*out_stride + j]
 * = (C_b^-1)_jj = sum_{i >= j} (L_b^-1)_ij^2 for the L left by sf_potrf_batch (same n, lda, stride).  With alpha = C^-1 r
 * (sf_potrs_batch, SF_APPLY_CINV) this is the leave-one-out predictive of a Gaussian process (Rasmussen & Williams, Gaussian
 * Processes for Machine Learning, 5.4.2): mean r_j - alpha_j / d_j, variance 1 / d_j.  The lower triangle of d_L is read and
 * left bit-identical; the strict upper triangle is scratch (nothing in it is read before it has been written) and is
 * undefined afterwards.  Every sum has a fixed order: a repeated call gives the same bits.  d_work:
 * sf_potri_diag_workspace_bytes(n, batch) (0 for bad arguments): the inverses of the 64 x 64 diagonal blocks.  SF_EINVAL
 * before anything is enqueued: n not a positive multiple of 64, lda < n, batch < 1, out_stride < n, null pointers, workspace
 * too small.  Componentwise |d^ - d| <= 2 gamma_2n diag(|X|^T |X||L||X|) + gamma_{n+1} d with X = L^-1 (Higham, Accuracy and
 * Stability of Numerical Algorithms, ch. 14). */
size_t sf_potri_diag_workspace_bytes(int n, int batch);
int sf_potri_diag_batch(double* d_L, int n, int lda, int64_t stride, int batch, double* d_out, int64_t out_stride, void* d_work,
                        size_t work_bytes, void* stream);

/* Selected 64 x 64 blocks of the inverse from the factor (the blocks of LAPACK dpotri's result that a caller names):
 * d_out[((b*npairs + p)*64 + r)*64 + c] = (C_b^-1)[64 I_p + r][64 J_p + c] for the L left by sf_potrf_batch (same n, lda,
 * stride).  d_pairs: device array of npairs x (I, J) int32 with 0 <= J <= I < n / 64; a pair may be listed more than once; a
 * pair outside that range gives a block of NaN and reads nothing.  Runs the two launches of sf_potri_diag_batch (X = L^-1 into
 * the strict upper triangle, which is scratch and undefined afterwards; the lower triangle is read and left bit-identical),
 * then G_IJ = sum_{K >= I} X_KI^T X_KJ on the matrix cores.  Every sum has a fixed order: a repeated call gives the same bits.
 * d_work: sf_potri_blocks_workspace_bytes(n, batch) (0 for bad arguments).  SF_EINVAL before anything is enqueued: n not a
 * positive multiple of 64, lda < n, batch < 1, npairs < 1, null pointers, workspace too small.  Entrywise |G^ - G| <=
 * gamma_2n (E + E^T) + gamma_{n+1} |X|^T |X| with E = |X|^T |X||L||X|. */
size_t sf_potri_blocks_workspace_bytes(int n, int batch);
int sf_potri_blocks_batch(double* d_L, int n, int lda, int64_t stride, int batch, const int* d_pairs, int npairs, double* d_out,
                          void* d_work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-order context: static data resident in HBM for the whole chain
 * ---------------------------------------------------------------------------------------- */
typedef struct sf_ctx sf_ctx;

/* All pointers are HOST pointers; everything is copied.  Mirrors what
 * SpectrumModel.__init__ (Starfish/models/spectrum_model.py:126-181) and Emulator.__init__
 * (Starfish/emulator/emulator.py:69-131) hold. */
typedef struct sf_order_desc {
    int32_t n;       /* masked data pixels N                     (spectrum.py:41-58)        */
    int32_t nf;      /* length of min_dv_wave, a power of two    (utils.py:79-84)           */
    int32_t m;       /* eigenspectra                             (emulator.py:104)          */
    int32_t n_grid;  /* emulator parameter dimensions                                       */
    int32_t M;       /* library grid points                                                  */
    int32_t reserved;
    const double* wave;         /* [n]   data.wave                                           */
    const double* flux;         /* [n]   data.flux                                           */
    const double* sigma;        /* [n]   data.sigma                                          */
    const double* min_dv_wave;  /* [nf]  spectrum_model.py:151-153                           */
    const double* bulk_fluxes;  /* [(m+2)*nf] eigenspectra; flux_mean; flux_std resampled on
                                   min_dv_wave (spectrum_model.py:154-156)                   */
    const double* grid_points;  /* [M*n_grid]                                                */
    const double* variances;    /* [m]                                                       */
    const double* lengthscales; /* [m*n_grid]                                                */
    const double* v11;          /* [(m*M)^2]  emulator.py:123-128                            */
    const double* w_hat;        /* [m*M]      component-major (emulator/_utils.py:19-21)     */
    /* optional (both or neither): the factor of the constant v11, so that callers holding many orders of
     * one emulator factor it once (LAPACK) instead of once per context.  linv = inverse of the LOWER
     * Cholesky factor of v11, row-major with zeros above the diagonal; alpha = v11^-1 w_hat.
     * NULL: computed by sf_ctx_create on the host (scalar code: fine up to m*M of a few hundred). */
    const double* linv;         /* [(m*M)^2] or NULL                                         */
    const double* alpha;        /* [m*M] or NULL                                             */
} sf_order_desc;

sf_ctx* sf_ctx_create(const sf_order_desc* desc, int device, int* err);
void sf_ctx_destroy(sf_ctx* ctx);
int sf_ctx_npad(const sf_ctx* ctx); /* N rounded up to the Cholesky leaf (64)              */
int sf_ctx_lda(const sf_ctx* ctx);  /* row stride used for the covariance matrices          */

/* Which optional parameters the model carries (the `"x" in self.params` tests of
 * SpectrumModel.__call__, spectrum_model.py:290-363) and the layout of one parameter row:
 *   [0] vsini  [1] vz  [2] log_scale  [3] norm factor (1 unless norm=True)
 *   [4] global log_amp  [5] global log_ls
 *   [6 .. 6+n_grid)             emulator grid parameters
 *   [.. +n_cheb)                c1, c2, ...   (c0 == 1, spectrum_model.py:301-304)
 *   [.. +3*n_local)             (mu, log_amp, log_sigma) per local kernel
 *   [.. +1)                     Av, only when has_av (extinct(), Starfish/transforms.py:161-206 as
 *                               called at spectrum_model.py:298-299: law ccm89, Rv = 3.1)
 * Unused slots are ignored.  Row stride = sf_param_stride(). */
typedef struct sf_model_desc {
    int32_t has_vsini;     /* needs 16 <= nf <= 65536: every call refuses other orders with SF_EINVAL up front */
    int32_t has_vz;
    int32_t has_log_scale; /* 0: renormalise by the integrated-flux ratio (spectrum_model.py:322-326) */
    int32_t has_global;
    int32_t n_local;
    int32_t n_cheb;
    int32_t use_sigma_w; /* 0 (default, parity): C_emu = X^T Sigma_w^-1 X as the code does
                            (spectrum_model.py:334-335); 1: X^T Sigma_w X as the paper says  */
    int32_t has_av;      /* 1: multiply every row by 10^(-0.4 A_lambda), A_lambda from the published
                            CCM89 law (Cardelli, Clayton & Mathis 1989) with Rv = 3.1.  PARITY
                            UNPINNED: the reference delegates this to the third-party `extinction`
                            C extension, which is not available to generate vectors from.          */
} sf_model_desc;

int sf_param_stride(const sf_ctx* ctx, const sf_model_desc* model);

/* scratch needed by the batched calls below for B walkers (covariance matrices included) */
size_t sf_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B);

/* Emulator.__call__ (Starfish/emulator/emulator.py:330-394) for B parameter rows:
 * d_mu[B*m], d_cov[B*m*m].  d_params: B x stride rows laid out as above. */
int sf_emulator_query_batch(sf_ctx* ctx, const sf_model_desc* model, int B,
                            const double* d_params, double* d_mu, double* d_cov, int* d_info,
                            void* d_work, size_t work_bytes, void* stream);

/* Emulator.__call__ with several parameter rows (emulator.py:382-389): the JOINT conditional of the
 * B*m weights, component-major (index i*B + b): d_mu[B*m], d_cov[(B*m)^2]. */
int sf_emulator_joint_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params,
                            double* d_mu, double* d_cov, int* d_info, void* d_work,
                            size_t work_bytes, void* stream);

/* Transform chain of SpectrumModel.__call__ (spectrum_model.py:287-332): rotational_broaden,
 * doppler_shift, resample, chebyshev_correct, eigenspectrum reconstruction and (re)scaling.
 * Outputs: d_flux[B*n] scaled model flux, d_X[B*m*n] scaled eig*std rows, d_resid[B*n] =
 * flux - data.flux, d_log_scale[B] (the `_log_scale` attribute).  Any output may be NULL. */
int sf_transform_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params,
                       double* d_flux, double* d_X, double* d_resid, double* d_log_scale,
                       int* d_info, void* d_work, size_t work_bytes, void* stream);

/* SpectrumModel.__call__ (spectrum_model.py:277-365): d_flux[B*n], d_cov[B*n*n] (full symmetric
 * matrices, WITHOUT the 1e-10 jitter, exactly what the reference returns). */
int sf_forward_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params,
                     double* d_flux, double* d_cov, double* d_log_scale, int* d_info,
                     void* d_work, size_t work_bytes, void* stream);

/* The fused covariance fill on its own: C = X^T Sigma_w^-1 X (spectrum_model.py:334-338) + sigma^2 on
 * the diagonal (:338) + global Matern-3/2 kernel + local Gaussian kernels (models/kernels.py:7-81), and -- with
 * add_jitter -- the 1e-10 the likelihood adds before factorising (spectrum_model.py:399), in the reference's order of
 * additions, written in ONE pass into the caller's array: matrix b at d_cov + b * stride, row stride ld >= n.
 * lower_only: tiles above the diagonal are skipped (entries above the diagonal INSIDE a diagonal tile may be written; a
 * factorisation never reads them).  (sf_forward_batch = this with ld = n, both triangles, no
 * jitter, plus the flux; the likelihood entry points run the same kernel on the workspace matrices.) */
int sf_cov_fill_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, double* d_cov, int ld,
                      int64_t stride, int lower_only, int add_jitter, int* d_info, void* d_work, size_t work_bytes,
                      void* stream);

/* SpectrumModel.log_likelihood without the prior term (spectrum_model.py:397-405):
 * d_lnl[B] = -(logdet + sqmah)/2; optional d_logdet[B], d_sqmah[B], d_resid[B*n],
 * d_log_scale[B].  Items with d_info[b] != 0 get lnl = -inf. */
int sf_loglike_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params,
                     double* d_lnl, double* d_logdet, double* d_sqmah, double* d_resid,
                     double* d_log_scale, int* d_info, void* d_work, size_t work_bytes,
                     void* stream);

/* The Cholesky factor of the walkers' covariance matrices applied to right-hand sides: the same transform chain, fill
 * (lower triangle, 1e-10 jitter) and dense factorisation as sf_loglike_batch, then sf_potrs_batch's `op` (SF_APPLY_*):
 * C^-1 rhs (cho_solve, spectrum_model.py:404), whitened vectors L^-1 rhs, noise draws L z.  The structure-exploiting
 * solver is not involved.  d_rhs: right-hand side r of walker b at d_rhs + b*rhs_stride + r*ldr, n = data pixels
 * contiguous rows, ldr >= n; rhs_stride == 0: one block shared by all walkers; d_rhs == NULL: each walker's own residual
 * flux - data.flux (nrhs must be 1).  d_out[B*nrhs*n] (must not overlap d_rhs); d_flux[B*n] (model flux) and d_info[B]
 * may be NULL.  Walkers with d_info[b] != 0 (the codes of sf_loglike_batch) get NaN in d_out.
 * d_work: sf_apply_workspace_bytes(ctx, model, B, nrhs) (0 for bad arguments). */
size_t sf_apply_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int nrhs);
int sf_apply_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, int op, const double* d_rhs,
                   int nrhs, int ldr, int64_t rhs_stride, double* d_out, double* d_flux, int* d_info, void* d_work,
                   size_t work_bytes, void* stream);

/* The residual split by covariance component: alpha = C^-1 rhs by the sequence of sf_apply_batch with SF_APPLY_CINV (same
 * transform chain, fill, factorisation: the same bits), then the conditional mean of every term of
 *     C = Y^T Y (emulator) + diag(sigma^2 + 1e-10) (noise, the likelihood's jitter) + K_global + sum_j K_local,j
 * given rhs, mu_k = K_k alpha, without materialising a matrix.  Component order: 0 emulator, 1 noise, 2 global (zeros for
 * a model without has_global), 3 + j local kernel j: ncomp = 3 + n_local, d_comp[B][ncomp][nrhs][n].  The components add
 * up to C alpha = rhs to rounding.  The structured entries are evaluated by the element formulas of the fill on the same
 * operands; every sum has a fixed order (a repeated call gives the same bits); rows beyond n are never written.
 * d_rhs, nrhs, ldr, rhs_stride: as sf_apply_batch (NULL: each walker's own residual, nrhs must be 1; rhs_stride == 0:
 * one block shared by all walkers).  d_alpha[B*nrhs*n], d_flux[B*n] and d_info[B] may be NULL.  Walkers with
 * d_info[b] != 0 (the codes of sf_loglike_batch) get NaN in every row of d_comp and d_alpha.  SF_EINVAL before anything is
 * enqueued: B or nrhs outside 1 .. 65535, null d_params or d_comp, rhs_stride < 0, nrhs != 1 without d_rhs, a bad context
 * or model, ldr < n.  d_work: sf_decompose_workspace_bytes(ctx, model, B, nrhs) (0 for bad arguments): the workspace of
 * sf_apply_batch plus m doubles per right-hand side. */
size_t sf_decompose_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int nrhs);
int sf_decompose_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const double* d_rhs, int nrhs,
                       int ldr, int64_t rhs_stride, double* d_comp, double* d_alpha, double* d_flux, int* d_info,
                       void* d_work, size_t work_bytes, void* stream);
/* Timing aid (tools/bench_decompose.py): the last step of sf_decompose_batch alone, K_k alpha -> d_comp, on the workspace
 * that a call of sf_decompose_batch with the same ctx, model, B, nrhs and d_params left behind. */
int sf_debug_decompose_matvec(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, int nrhs,
                              double* d_comp, void* d_work, size_t work_bytes, void* stream);

/* Per-pixel leave-one-out diagnostics: alpha = C^-1 rhs by the sequence of sf_apply_batch with SF_APPLY_CINV (same transform
 * chain, fill, factorisation: the same bits), then sf_potri_diag_batch on the workspace matrices: d_cinv_diag[B][n] =
 * diag(C_b^-1).  Pixel i predicted from all the others has mean rhs_i - alpha_i / d_i and variance 1 / d_i.
 * d_cov_diag[B][n] (may be NULL): the diagonal of the matrix that is factorised, the 1e-10 jitter included, copied out
 * between fill and factorisation (the marginal variances).  d_rhs, nrhs, ldr, rhs_stride: as sf_apply_batch (NULL: each
 * walker's own residual, nrhs must be 1; rhs_stride == 0: one block shared by all walkers).  d_alpha[B*nrhs*n] and
 * d_cinv_diag are required; d_flux[B*n] and d_info[B] may be NULL.  Walkers with d_info[b] != 0 (the codes of
 * sf_loglike_batch) get NaN in every row of d_alpha, d_cinv_diag and d_cov_diag.  SF_EINVAL before anything is enqueued: B
 * or nrhs outside 1 .. 65535, null d_params, d_alpha or d_cinv_diag, rhs_stride < 0, nrhs != 1 without d_rhs, a bad context
 * or model, ldr < n.  d_work: sf_pointwise_workspace_bytes(ctx, model, B, nrhs) (0 for bad arguments): the workspace of
 * sf_apply_batch, two rows of npad doubles per walker and the workspace of sf_potri_diag_batch. */
size_t sf_pointwise_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int nrhs);
int sf_pointwise_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const double* d_rhs, int nrhs,
                       int ldr, int64_t rhs_stride, double* d_alpha, double* d_cinv_diag, double* d_cov_diag, double* d_flux,
                       int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The likelihood and its gradient in the covariance hyper-parameters: d lnL / d theta = 1/2 sum_ij (alpha_i alpha_j -
 * (C^-1)_ij) (dC / d theta)_ij (Rasmussen & Williams, Gaussian Processes for Machine Learning, eq. 5.9) with alpha = C^-1 r by
 * the sequence of sf_apply_batch with SF_APPLY_CINV on each walker's own residual (same transform chain, fill, factorisation
 * and finish: d_lnl and d_info have sf_loglike_batch's bits), the blocks of C^-1 on the kernels' support as
 * sf_potri_blocks_batch forms them, and the analytic entry derivatives.  d_grad[b*grad_stride + s], slots in parameter-row
 * order: log_amp, log_ls of the global kernel if the model has one, then mu, log_amp, log_sigma of every local kernel.  In mu
 * the likelihood has a kink wherever two pixels of a patch are equidistant from mu; the derivative is the almost-everywhere
 * one.  The matrix is the one that is factorised (jitter included).  d_flux[B*n] and d_info[B] may be NULL.  Walkers with
 * d_info[b] != 0 get NaN in every slot.  Every sum has a fixed order: a repeated call gives the same bits.  SF_EINVAL before
 * anything is enqueued: B outside 1 .. 65535, null d_params, d_lnl or d_grad, a model without global and local kernels
 * ("nothing to differentiate"), grad_stride below the number of slots, a bad context or model.  d_work:
 * sf_loglike_grad_workspace_bytes(ctx, model, B) (0 for bad arguments): the workspace of sf_apply_batch with one right-hand
 * side, a row of npad doubles per walker, the workspace of sf_potri_diag_batch and one double per (walker, 64-row block,
 * slot). */
size_t sf_loglike_grad_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B);
int sf_loglike_grad_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, double* d_lnl, double* d_grad,
                          int grad_stride, double* d_flux, int* d_info, void* d_work, size_t work_bytes, void* stream);
/* Timing aid (tools/bench_gradient.py): the contraction launches of sf_loglike_grad_batch alone, on the workspace that a
 * call of sf_loglike_grad_batch with the same ctx, model, B and d_params left behind. */
int sf_debug_loglike_grad_contract(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, double* d_grad,
                                   int grad_stride, void* d_work, size_t work_bytes, void* stream);

/* The Fisher information of the covariance hyper-parameters,
 *     F_ij = 1/2 tr(C^-1 dC/dtheta_i C^-1 dC/dtheta_j),
 * in the slots of sf_loglike_grad_batch (s = 2 with a global kernel + 3 per local kernel, same order): its inverse is the
 * Laplace covariance of the fitted noise model.  The head is sf_loglike_grad_batch's (factor and inverse factor on the
 * walker's own residual: d_lnl and d_info, both may be NULL, have sf_loglike_batch's bits).  Then every 64 x 64 tile of
 * W = C^-1 is formed once per walker, and per slot j the product T_j = W dC_j (the derivative tiles generated from the entry
 * formulas on the kernel's support), the tiles of S_j = T_j W on the kernels' support, both on the fp64 matrix cores, and the
 * block-row contraction F_ij = 1/2 sum (dC_i)_ab (S_j)_ab for i >= j.  d_fisher[b*fisher_stride + i*s + j], fisher_stride >=
 * s*s; the upper triangle is the mirror image: F_ij and F_ji are the same bits.  The matrix is the one that is factorised
 * (jitter included); the derivative in mu is the almost-everywhere one.  A walker with d_info[b] != 0 gets a NaN matrix.
 * Every sum has a fixed order that does not depend on the batch: a repeated call and a call on a sub-batch give the same
 * bits.  Dense factor only (the band of Bd^-1 does not hold C^-1 dC_i C^-1 off the band).  SF_EINVAL, the message starting
 * with the call's name, before anything is enqueued and before the context is looked at: B outside 1 .. 65535, null
 * d_params or d_fisher, a model without global and local kernels ("nothing to differentiate"), fisher_stride < s*s; then a
 * bad context or model.  d_work: sf_fisher_cov_workspace_bytes(ctx, model, B) (0 for what the call refuses): the workspace
 * of sf_loglike_grad_batch plus, per walker, two matrices of ld x ld doubles, ld = 64 ceil(n / 64) (all of W; one T_j): the
 * slots are worked through one at a time, so the size does not grow with s.  Never synchronises. */
size_t sf_fisher_cov_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B);
int sf_fisher_cov_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, double* d_lnl, double* d_fisher,
                        int fisher_stride, int* d_info, void* d_work, size_t work_bytes, void* stream);
/* Timing aid (tools/bench_cov_fisher.py): the launches of sf_fisher_cov_batch behind the inverse alone, on the workspace that
 * a call of sf_fisher_cov_batch with the same ctx, model, B and d_params left behind. */
int sf_debug_fisher_cov_contract(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, double* d_fisher,
                                 int fisher_stride, void* d_work, size_t work_bytes, void* stream);

/* The score (Lagrange-multiplier) scan for a NEW local kernel: where does one belong, and how wide?  For every candidate (mu,
 * sigma in km/s) and every walker, with k(mu, sigma) the matrix the fill would add for a local kernel of that centre and width
 * at amplitude 1 (the reference's local_covariance_matrix, cut off at 4 sigma), alpha = C^-1 r and W = C^-1 of the walker's
 * covariance as it stands (every kernel the model has included),
 *     quad = alpha^T k alpha,    trace = tr(W k),    fisher = 1/2 tr(W k W k),
 * d_out[(b*ncand + q)*3 + 0 .. 2].  The derivative of lnL in the new kernel's amplitude A at A = 0 is U = 1/2 (quad - trace), its
 * information is fisher: z = U / sqrt(fisher) is the score statistic and U / fisher one Newton step in A.  d_cand[q*2 + 0 .. 1] =
 * mu, sigma is shared by the batch.  The head is sf_pointwise_batch's (factor and inverse factor on the walker's own residual:
 * d_lnl and d_info, both may be NULL, have sf_loglike_batch's bits).  k lives on the pixels within 4 sigma (1 + 1e-9) of mu, a
 * contiguous patch of the grid, so only the 64 x 64 tiles of W within 4 blocks of the diagonal are formed (once per walker, with
 * their mirror images); per (walker, candidate) one workgroup generates the tiles of k from the fill's element formulas and
 * forms the products W k on the fp64 matrix cores.  A candidate's numbers do not depend on the other candidates, the batch or
 * the chunk (same bits).  A candidate with no pixel in reach gets exactly 0, 0, 0; one whose patch is wider than
 * SF_LOCAL_SCAN_MAX_PATCH pixels, or whose mu or sigma is not positive and finite, gets NaN in all three for every walker; a
 * walker with d_info[b] != 0 gets NaN rows.  The model may have no global and no local kernel at all.  Dense factor only.
 * SF_EINVAL, the message starting with the call's name, before anything is enqueued: B or ncand outside 1 .. 65535, null
 * d_params, d_cand or d_out; then a bad context or model; then a wavelength grid that is not monotonic.  d_work:
 * sf_local_scan_workspace_bytes(ctx, model, B, ncand) (0 for what the call refuses): the workspace of sf_pointwise_batch's
 * inverse, two ints per candidate and, per walker, ceil(n / 64) * 9 tiles of 64 x 64 doubles -- linear in n.  Never synchronises. */
#define SF_LOCAL_SCAN_MAX_PATCH 256
size_t sf_local_scan_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int ncand);
int sf_local_scan_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const double* d_cand, int ncand,
                        double* d_out, double* d_lnl, int* d_info, void* d_work, size_t work_bytes, void* stream);
/* Timing aid (tools/bench_local_scan.py): the launches of sf_local_scan_batch behind the inverse alone, on the workspace that
 * a call of sf_local_scan_batch with the same ctx, model, B, d_params and ncand left behind. */
int sf_debug_local_scan_contract(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const double* d_cand,
                                 int ncand, double* d_out, void* d_work, size_t work_bytes, void* stream);
/* The same scan on the band + Woodbury solver: no N x N matrix anywhere.  With C = Bd + Y^T Y, Sigma = Bd^-1 and Vs = Bd^-1 Y^T
 * L_S^-T, W = C^-1 = Sigma - Vs Vs^T.  The head is the one sf_diagnose_banded_batch runs for the walker's own residual with
 * d_cinv_diag (band filled entry by entry, keeping sweep, capacitance step, backward sweep, alpha, the selected inversion, Vs),
 * run at the widest half-width the LDS window takes for the 1 + m rows, wmax = 144 / 128 / 112 for m <= 15 / 31 / 32, WHATEVER
 * the model's own support is: the selected inversion is exact on the band it is run at and a band wider than the kernels' support
 * holds zeros, so every patch of at most sf_local_scan_banded_max_patch = wmax + 1 pixels is served exactly, and a candidate's
 * numbers depend on m alone -- not on the other candidates, the batch, the chunk or a group of walkers (same bits).  Behind the
 * head the 64 x 64 tiles of W within 3 blocks of the diagonal are formed from the band of Sigma and the rank-m product on the fp64
 * matrix cores, then the candidates run as in sf_local_scan_batch.  d_out as there (values agree to rounding, not bit for bit);
 * d_lnl and d_info (both may be NULL) as the banded head leaves them: a walker whose covariance support exceeds wmax gets
 * SF_INFO_BANDWIDTH, -inf and NaN rows.  A candidate with no pixel in reach gets exactly 0, 0, 0; one whose patch is wider than
 * wmax + 1 pixels, or whose mu or sigma is not positive and finite, gets NaN for every walker; d_info[b] != 0 gives NaN rows.  The
 * model may have no global and no local kernel (Bd is then diagonal).
 * sf_local_scan_banded_max_patch: wmax + 1; 0: no window (m too large) or a grid that is not strictly increasing; SF_EINVAL: bad
 * context or model.  SF_EINVAL, the message starting with the call's name, before anything is enqueued (size query 0): B or ncand
 * outside 1 .. 65535; a bad context or model; a grid that is not strictly increasing; no window for 1 + m rows (use
 * sf_local_scan_batch); null d_params, d_cand, d_out or d_work.  A short workspace: SF_ENOMEM.  d_work:
 * sf_local_scan_banded_workspace_bytes: the workspace of sf_diagnose_banded_batch for one right-hand side with want_cinv_diag at
 * wmax, two ints per candidate and, per walker, ceil(n / 64) * (2 min(ceil(n / 64) - 1, 3) + 1) tiles of 64 x 64 doubles -- linear
 * in n.  Never synchronises. */
int sf_local_scan_banded_max_patch(const sf_ctx* ctx, const sf_model_desc* model);
size_t sf_local_scan_banded_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int ncand);
int sf_local_scan_banded_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const double* d_cand, int ncand,
                               double* d_out, double* d_lnl, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The likelihood and its gradient in the mean-flux parameters: vsini (column 0 of the parameter row), vz (1), log_scale (2), the
 * emulator grid parameters, the Chebyshev coefficients and Av.  They enter through the flux f, the scaled emulator rows X and
 * the emulator's weight covariance Sigma_w, not through the structured kernels.  With alpha = C^-1 r, V = C^-1 X^T, a = X alpha,
 * z_a = Sigma_w^-1 a and G = Sigma_w^-1 X V Sigma_w^-1,
 *     d lnL = -alpha^T df + sum_ki dX_ki (alpha_i z_a,k - (V Sigma_w^-1)_ik) - 1/2 z_a^T dS z_a + 1/2 tr(dS G),  dS = dSigma_w,
 * so no inverse is needed: the sequence of sf_apply_batch with SF_APPLY_CINV on the 1 + m right-hand sides [r, X_1 .. X_m]
 * (same transform chain, fill, factorisation and finish: d_lnl and d_info have sf_loglike_batch's bits, d_flux
 * sf_apply_batch's), per-walker m x m algebra, one pass over the pixels with the analytic row tangents (transform parameters:
 * dSigma_w = 0) and one over the rows of the emulator's z = Linv v12 (grid parameters: dX = 0, df = dmu^T X).  At vsini <= 0 the
 * likelihood is not differentiated: such walkers are flagged as by sf_loglike_batch.  h_slots (HOST): the nslots columns of the
 * parameter row to differentiate in, 1 <= nslots <= SF_MEAN_GRAD_MAX_SLOTS, no column twice; d_grad[b*grad_stride + j] belongs
 * to h_slots[j], and a subset of columns gives the bits of those columns of a larger call.  The matrix is the one that is
 * factorised (jitter included).  d_flux[B*n] and d_info[B] may be NULL.  Walkers with d_info[b] != 0 get NaN in every slot.
 * Every sum has a fixed order: a repeated call gives the same bits.  SF_EINVAL before anything is enqueued: B outside
 * 1 .. 65535, null d_params, h_slots, d_lnl or d_grad, nslots outside its range, a repeated column, a column that is none of
 * the above or that the model does not have (norm, the covariance hyper-parameters), grad_stride < nslots, a model without
 * log_scale (the renormalising scale is not differentiated), use_sigma_w, a bad context or model.  d_work:
 * sf_loglike_mean_grad_workspace_bytes(ctx, model, B, nslots) (0 for bad arguments): the workspace of sf_apply_batch with
 * 1 + m right-hand sides; per walker the m scaled rows, 2 m + 3 m^2 doubles, one double per (256-pixel block, slot), a second
 * set of spline coefficients if the model has vsini, and m M (m + 1) + m doubles for each of min(nslots, n_grid) grid columns. */
#define SF_MEAN_GRAD_MAX_SLOTS 16
size_t sf_loglike_mean_grad_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int nslots);
int sf_loglike_mean_grad_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const int* h_slots,
                               int nslots, double* d_lnl, double* d_grad, int grad_stride, double* d_flux, int* d_info,
                               void* d_work, size_t work_bytes, void* stream);
/* Timing aid (tools/bench_mean_gradient.py): the launches of sf_loglike_mean_grad_batch behind the solve alone (moments, pixel
 * pass, grid slots, sum), on the workspace that a call of sf_loglike_mean_grad_batch with the same ctx, model, B, d_params and slots left
 * behind. */
int sf_debug_loglike_mean_grad_contract(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params,
                                        const int* h_slots, int nslots, double* d_grad, int grad_stride, void* d_work,
                                        size_t work_bytes, void* stream);

/* The Fisher information of the mean-flux parameters at fixed covariance,
 *     F_ij = fdot_i^T C^-1 fdot_j,   fdot_j = d f / d theta_j,
 * for the columns h_slots of sf_loglike_mean_grad_batch (same columns, same slot checks): the inverse of F is the Laplace
 * covariance of vsini, vz, log_scale, Av, cheb:k and the grid parameters; the mean / covariance cross block of a Gaussian's
 * Fisher matrix is zero.  This is the Gauss-Newton, fixed-covariance matrix: the term 1/2 tr(C^-1 dC_i C^-1 dC_j) that a grid
 * parameter has because X sits inside the emulator's covariance is left out; the block of the covariance
 * hyper-parameters is sf_fisher_cov_batch's.  One pixel pass writes the tangent columns J (the row tangents of the gradient's pixel pass; a grid column
 * is dmu^T X; zero for a walker the transform chain flagged) as the right-hand sides of the likelihood's sequence,
 * SF_APPLY_LINV turns them into Z = L^-1 J, and F = Z^T Z is summed per 256-pixel block and then over the blocks in ascending
 * order, without atomics.  d_fisher[b*fisher_stride + i*nslots + j], fisher_stride >= nslots^2; the lower triangle is computed
 * and mirrored, so F_ij and F_ji are the same bits.  d_lnl and d_info (may be NULL) have sf_loglike_batch's bits; a walker with
 * info != 0 gets a NaN matrix.  A repeated call and a call on a sub-batch give the same bits; a subset of the slots agrees to
 * rounding, bit equality is not promised there.  SF_EINVAL before anything is enqueued for what sf_loglike_mean_grad_batch
 * refuses and for fisher_stride < nslots^2; sf_fisher_mean_workspace_bytes is 0 for the counts and models the call refuses.
 * The workspace is that of sf_loglike_mean_grad_batch with nslots right-hand sides plus one double per (256-pixel block, pair
 * of slots).  Never synchronises. */
size_t sf_fisher_mean_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int nslots);
int sf_fisher_mean_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, const int* h_slots, int nslots,
                         double* d_lnl, double* d_fisher, int fisher_stride, int* d_info, void* d_work, size_t work_bytes,
                         void* stream);

/* ---- multi-order batches (reference: the multi-order container
 * Starfish/spectrum.py:96-115, orders independent docs/intro.rst:71-73, EchelleModel stub
 * Starfish/models/echelle_model.py:1-2) -------------------------------------------------------------
 * Evaluates the (order x walker) units of several orders in ONE enqueue: segment i is an order
 * context with its own B_i parameter rows; every order runs its transform chain and covariance fill
 * into its slice of a common covariance array (orders shorter than the longest one of the group are
 * padded with an identity block, which changes neither logdet nor the quadratic form) and all
 * sum(B_i) matrices share one batched Cholesky.  Outputs are concatenated in segment order
 * (unit = sum_{j<i} B_j + b); the caller sums over orders.  All contexts must live on the same
 * device and agree in the number of eigenspectra and grid dimensions; one model descriptor describes
 * the parameter rows of every segment (sf_loglike_multi_batch_md below: one per segment).  Same values
 * as nseg calls of sf_loglike_batch. */
typedef struct sf_segment {
    sf_ctx* ctx;
    const double* d_params; /* DEVICE: B x sf_param_stride() rows of this order */
    int32_t B;
    int32_t reserved;
} sf_segment;
size_t sf_multi_workspace_bytes(const sf_segment* segs, int nseg, const sf_model_desc* model);
int sf_loglike_multi_batch(const sf_segment* segs, int nseg, const sf_model_desc* model,
                           double* d_lnl, double* d_logdet, double* d_sqmah, double* d_log_scale,
                           int* d_info, void* d_work, size_t work_bytes, void* stream);
/* The same with one model descriptor PER SEGMENT: models[i] describes the parameter rows of segs[i]
 * (row stride sf_param_stride(segs[i].ctx, models[i])), so orders with their own nuisance parameters
 * -- another number of local kernels or Chebyshev terms, with or without a global kernel -- still
 * share one batched Cholesky.  Every segment is checked before anything is enqueued (the error names
 * the segment); the transient buffers are sized for the union of the descriptors.  With every
 * models[i] equal to one descriptor the result is bit-identical to sf_loglike_multi_batch. */
size_t sf_multi_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models);
int sf_loglike_multi_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                              double* d_lnl, double* d_logdet, double* d_sqmah, double* d_log_scale,
                              int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The likelihood of the units of several orders AND its gradient, from ONE factorisation per unit: the sequence of
 * sf_loglike_multi_batch_md (same chunks, lanes and frame; d_lnl, d_log_scale and d_info have its bits for the same segments)
 * with the right-hand sides [r, X_1 .. X_m] of sf_loglike_mean_grad_batch (r alone in a call without mean slots) staged
 * behind every order's transform chain, SF_APPLY_CINV applied to the staging area of a whole chunk in one launch, the inverse
 * factor of sf_loglike_grad_batch formed for the chunks in which a segment wants covariance slots, and then per segment the
 * two contractions of the single-order calls: both need only alpha = C^-1 r, V = C^-1 X^T and X = L^-1 of the same factor.
 * requests[i] says what segment i is differentiated in: h_mean_slots (HOST) / n_mean_slots as sf_loglike_mean_grad_batch's
 * h_slots / nslots, except that 0 slots ask for none; want_cov != 0 for the covariance slots of models[i] in
 * sf_loglike_grad_batch's order.  d_grad[u * grad_stride + j], u = sum_{j<i} B_j + b: the row of a unit of segment i holds that
 * segment's mean slots in request order, then its covariance slots; entries of the row beyond them are not touched; a segment
 * that requests nothing gets lnl only.  Orders shorter than the group's common npad are padded with an identity block: every
 * contraction masks at the order's own n.  A subset of slots gives the bits of those slots of a larger request.  Units with
 * d_info[u] != 0 get NaN in every slot of theirs.  Every sum has a fixed order: a repeated call gives the same bits.
 * d_log_scale may be NULL.  SF_EINVAL before anything is enqueued, the message naming the segment: whatever
 * sf_loglike_multi_batch_md refuses; null requests, d_lnl, d_info or d_grad; a segment with more than 65535 units that requests
 * something; for a segment with mean slots whatever sf_loglike_mean_grad_batch refuses (a model without log_scale,
 * use_sigma_w, more than SF_MEAN_GRAD_MAX_SLOTS columns, a repeated or foreign column); want_cov on a model without global
 * and local kernels; a row shorter than a segment's slots; a call in which no segment requests anything ("nothing to
 * differentiate").  d_work: sf_multi_grad_workspace_bytes_md(...) (0 for bad arguments): the workspace of
 * sf_loglike_multi_batch_md, 1 + m (1 without mean slots) rows of the common npad doubles per unit, with covariance slots a
 * further row and the scratch of sf_potri_diag_batch per unit, and per segment what the single-order calls keep per walker
 * (sf_loglike_mean_grad_workspace_bytes, sf_loglike_grad_workspace_bytes) plus, with mean slots and vsini, a third set of
 * spline coefficients. */
typedef struct sf_grad_request {
    const int32_t* h_mean_slots; /* HOST: columns of the parameter row */
    int32_t n_mean_slots;        /* 0 .. SF_MEAN_GRAD_MAX_SLOTS */
    int32_t want_cov;            /* 1: the covariance slots of models[i], in sf_loglike_grad_batch's order */
} sf_grad_request;
size_t sf_multi_grad_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                        const sf_grad_request* requests, int grad_stride);
int sf_loglike_multi_grad_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                   const sf_grad_request* requests, double* d_lnl, double* d_log_scale, int* d_info,
                                   double* d_grad, int grad_stride, void* d_work, size_t work_bytes, void* stream);
/* The sum over the orders of what the call above leaves, for nseg segments of W walkers each (unit = i * W + w): per walker
 * d_lnl[w] = ((lnl_0 + lnl_1) + ...) in ascending order index, d_info[w] = the first non-zero unit code in that order, and
 * d_grad[w * out_stride + j], j < ncols, the same fixed-order sum of the unit slots that column j's list names:
 * d_col_src[2 q], d_col_src[2 q + 1] = (segment, slot) for d_col_ptr[j] <= q < d_col_ptr[j + 1] (DEVICE, int32, ascending in the
 * segment within a column); a column without a source is 0.0.  Where d_info[w] != 0, d_lnl[w] = -inf and every column is NaN.
 * Plain adds, no atomics: a repeated call gives the same bits.  A source outside the unit rows is not read (NaN).  SF_EINVAL: a
 * null pointer, nseg < 1, W outside 1 .. 65535, ncols < 0, grad_stride < 1, out_stride < ncols. */
int sf_multi_grad_reduce(int nseg, int W, const double* d_unit_lnl, const int* d_unit_info, const double* d_unit_grad,
                         int grad_stride, const int32_t* d_col_ptr, const int32_t* d_col_src, int ncols, double* d_lnl,
                         double* d_grad, int out_stride, int* d_info, void* stream);
/* sf_loglike_multi_grad_batch_md on the band + Woodbury solver (see the structure-exploiting solver below and
 * sf_loglike_banded_grad_batch): segs, models, requests, d_lnl, d_log_scale, d_info, d_grad and grad_stride mean exactly what
 * they mean there -- units in segment order, a unit's row its order's mean slots in request order and then all covariance slots
 * of its descriptor, NaN rows where d_info[u] != 0, a segment without a request gets lnl / info / log_scale only and its rows
 * of d_grad are not written.  h_halfwidth (HOST, one int per segment): the band half-width the caller vouches for per segment;
 * a unit whose support is wider gets d_info[u] = SF_INFO_BANDWIDTH.  No N x N matrix is formed.  Per segment, on the streams
 * sf_loglike_multi_batch_md runs its chains on: band fill, transform chain, row tangents; once per chunk of segments, over all
 * its units in one launch each: keeping sweep, capacitance step, backward sweep, mix, and with covariance slots selected
 * inversion and Vs; then per segment the contractions of sf_loglike_banded_grad_batch with the order's own n.  All units share
 * ONE frame taken from the whole call (never from a chunk, so a unit's bits do not depend on how a caller cuts its unit list
 * as long as the frame is the same): the largest n rounded up to 16 rows (shorter orders: identity rows, zero right-hand
 * sides), the largest npad, the largest half-width (a wider band than a unit needs holds zeros: exact).  A half-width may
 * exceed an order's length.  lnl and the slots agree with the dense call to rounding, not bit for bit; d_log_scale has its
 * bits.  Fixed summation order, no atomics in any sum: a repeated call gives the same bits.  The call never synchronises.
 * SF_EINVAL before anything is enqueued: whatever sf_loglike_multi_grad_batch_md refuses; a null h_halfwidth; a segment whose
 * wavelength grid is not strictly increasing; a half-width outside [0, sf_banded_window_halfwidth(ctx)] of its segment (the
 * bordered-tile path has no backward sweep: the message names sf_loglike_multi_grad_batch_md); a segment with more than 65535
 * units.  SF_ENOMEM: the workspace is too small.  d_work: sf_banded_multi_grad_workspace_bytes_md(...) (0 for bad
 * arguments): the workspace of sf_loglike_multi_batch_md without its matrices; per unit, in the common frame, the band, the
 * kept factor (~ n16 (W + 16 + 16) doubles), T and two staging areas of 1 + m rows, and with covariance slots the band of
 * Bd^-1; per segment what sf_loglike_multi_grad_batch_md keeps per segment. */
size_t sf_banded_multi_grad_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                               const sf_grad_request* requests, const int* h_halfwidth, int grad_stride);
int sf_loglike_banded_multi_grad_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                          const sf_grad_request* requests, const int* h_halfwidth, double* d_lnl,
                                          double* d_log_scale, int* d_info, double* d_grad, int grad_stride, void* d_work,
                                          size_t work_bytes, void* stream);

/* The Fisher information of the mean-flux parameters (sf_fisher_banded_mean_batch: F = G_JJ - U^T U at fixed covariance, the
 * Gauss-Newton block) for the units of several orders in one pass on the band + Woodbury solver.  segs, models and h_halfwidth
 * are exactly as for sf_loglike_banded_multi_grad_batch_md; requests[i].h_mean_slots / n_mean_slots are the tangent columns of
 * order i (p_i of them, 1 .. SF_MEAN_GRAD_MAX_SLOTS) and want_cov must be 0 (the covariance block is not computed).  Units in
 * segment order, u = sum_{j<i} B_j + b.  For a unit with d_info[u] == 0 the leading p_i x p_i block of
 * d_fisher[u * fisher_stride + a * fisher_ld + b] holds F of that unit in request order; only the lower triangle is computed
 * and it is mirrored, so F_ab and F_ba are the same bits; the block is NaN where d_info[u] != 0.  fisher_ld >= max p_i and
 * fisher_stride >= fisher_ld^2; outside the leading block the contents are unspecified.  d_lnl, d_info and d_log_scale (may be
 * NULL) are as for the gradient call.  Per segment, on the streams sf_loglike_multi_batch_md runs its chains on: band fill,
 * transform chain, row tangents and the sweep's rows [r; Y; J] into the segment's slice of a per-unit row buffer; once per
 * chunk of segments, over all its units in one launch each: ONE sweep (the likelihood's, not a keeping one; two half sweeps
 * where they pay for the frame), the capacitance step, lnl / info and F.  No kept factor, no backward sweep, no N x N matrix.
 * All units share ONE frame taken from the whole call, never from a chunk: the largest n rounded up to 16 rows (shorter
 * orders: identity rows, zero right-hand sides), the largest npad, the largest half-width and the largest row count
 * 1 + m + max p_i -- an order with fewer columns carries zero rows behind its own, which add exact zeros to the Gram matrix
 * and leave its p_i x p_i block what it is alone.  The row count 1 + m + max p_i picks the LDS window: half-widths up to
 * 144 with at most 16 rows, 128 with at most 32, 112 with at most 48.  A unit whose support is wider than its segment's half-width gets
 * SF_INFO_BANDWIDTH, -inf and a NaN block.  A unit's values agree with sf_fisher_banded_mean_batch on the same order to
 * rounding, not bit for bit (another frame picks another instantiation of the sweep).  The call never synchronises and uses no
 * atomics: a repeated call gives the same bits.  SF_EINVAL before anything is enqueued: whatever
 * sf_loglike_banded_multi_grad_batch_md refuses; want_cov != 0; a segment without mean slots; the call's largest half-width
 * beyond the window at the call's row count (the message names sf_fisher_mean_batch); null d_lnl, d_info or d_fisher;
 * fisher_ld < max p_i; fisher_stride < fisher_ld^2.  SF_ENOMEM: the workspace is too small.  d_work:
 * sf_fisher_banded_multi_workspace_bytes_md(...) (0 for what the call refuses on these arguments): the workspace of
 * sf_loglike_multi_batch_md without its matrices; per unit, in the common frame, the band, 1 + m + max p_i rows of npad
 * doubles, two Gram matrices and a compact block; the half sweeps' scratch; per segment what the tangent columns keep per
 * walker. */
size_t sf_fisher_banded_multi_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                 const sf_grad_request* requests, const int* h_halfwidth);
int sf_fisher_banded_multi_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                    const sf_grad_request* requests, const int* h_halfwidth, double* d_lnl, double* d_log_scale,
                                    int* d_info, double* d_fisher, int fisher_ld, int fisher_stride, void* d_work,
                                    size_t work_bytes, void* stream);
/* The sum over the orders of what the call above leaves, for nseg segments of W walkers each (unit = i * W + w), through the
 * column map of sf_multi_grad_reduce unchanged: d_col_ptr / d_col_src list, per label, its (segment, slot) sources ascending in
 * the segment, at most one per segment.  Entry (a, b) of walker w is the sum, over the segments that appear in BOTH labels'
 * lists and in ascending segment index, of that unit's F[slot_a][slot_b] = d_unit_fisher[u * fisher_stride + slot_a * fisher_ld
 * + slot_b], written s = f_0; s = s + f_1; ...; a pair with no common segment (two labels of different orders, a label without
 * a source) is exactly 0.0.  a >= b is computed and mirrored into d_fisher[w * out_stride + a * ncols + b].  d_lnl and d_info
 * follow sf_multi_grad_reduce's rule; where d_info[w] != 0, d_lnl[w] = -inf and the matrix is NaN.  Plain adds, no atomics: a
 * repeated call gives the same bits.  A source outside the unit block is not read (NaN).  SF_EINVAL: a null pointer, nseg < 1,
 * W outside 1 .. 65535, ncols outside 0 .. 32768, fisher_ld < 1, fisher_stride < fisher_ld^2, out_stride < ncols^2. */
int sf_multi_fisher_reduce(int nseg, int W, const double* d_unit_lnl, const int* d_unit_info, const double* d_unit_fisher,
                           int fisher_ld, int fisher_stride, const int32_t* d_col_ptr, const int32_t* d_col_src, int ncols,
                           double* d_lnl, double* d_fisher, int out_stride, int* d_info, void* stream);

/* The score scan for a new local kernel (sf_local_scan_banded_batch) for the units of several orders in one pass on the band +
 * Woodbury solver.  segs and models are exactly as for sf_loglike_banded_multi_grad_batch_md and must satisfy what it requires of
 * them: contexts of one device with the same number of eigenspectra and grid dimensions, a good descriptor and parameter rows
 * per segment, 1 .. 65535 units per segment, every wavelength grid strictly increasing.  There is no h_halfwidth: the frame's
 * half-width is wmax, the widest the LDS window takes for the 1 + m rows [r; Y] (144 / 128 / 112 for m <= 15 / 31 / 32), the rule
 * of the single-order call -- a wider band than a unit needs holds zeros, so every patch of at most wmax + 1 pixels is served
 * exactly whatever the orders' own support is.  A unit whose covariance support exceeds wmax gets SF_INFO_BANDWIDTH, -inf and NaN
 * rows.  Candidates: h_cand_ptr (HOST, nseg + 1 ascending ints); segment i scans d_cand[2 q], d_cand[2 q + 1] = mu, sigma in km/s
 * for h_cand_ptr[i] <= q < h_cand_ptr[i + 1], between 1 and 65535 of them, shared by its walkers; the lists of two segments may
 * differ in length.  d_out is unit-major, segment after segment: segment i starts at 3 * sum_{j<i} B_j ncand_j, and inside it
 * d_out[(b * ncand_i + q) * 3 + 0 .. 2] = quad, trace, fisher of walker b and the segment's candidate q, as in the single-order
 * call: exactly 0, 0, 0 with no pixel in reach; NaN for a patch wider than wmax + 1 pixels and for a centre or width that is not
 * positive and finite; NaN rows where d_info[u] != 0.  d_lnl and d_info (units in segment order) are required, d_log_scale may be
 * NULL.  Per segment, on the streams sf_loglike_multi_batch_md runs its chains on: the band fill, entry by entry, and the
 * transform chain; once per chunk of segments, over all its units in one launch each: keeping sweep, capacitance step, lnl /
 * info, backward sweep and mix (alpha), selected inversion and Vs; then per segment the launches of the single-order scan (tiles
 * of W, patches, candidates) with the order's own n, wavelength grid and candidates.  ONE frame from the whole call, never from a
 * chunk: the largest n rounded up to 16 rows (shorter orders: identity rows, zero right-hand sides), the largest npad, the row
 * count 1 + m and wmax.  Values agree with sf_local_scan_banded_batch on the same order to rounding.  The call never
 * synchronises and uses no atomics, every sum has a fixed order: a repeated call gives the same bits.
 * sf_local_scan_banded_multi_max_patch: wmax + 1 for that frame; 0: no window for 1 + m rows, or a grid that is not strictly
 * increasing; SF_EINVAL: a bad segment list.  SF_EINVAL, the message starting with the call's name and naming the segment, before
 * anything is enqueued (size query 0): a bad segment list, context, model or batch; a grid that is not strictly increasing; no
 * window; a null h_cand_ptr, a list that is not ascending from a non-negative start or a segment with a count outside 1 ..
 * 65535; null d_cand, d_out, d_lnl, d_info or d_work.  SF_ENOMEM: the workspace is too small.  d_work:
 * sf_local_scan_banded_multi_workspace_bytes_md(...): the workspace of sf_loglike_multi_batch_md without its matrices; per unit,
 * in the common frame, the band, the kept factor, the band of Bd^-1, T of 1 + m rows, alpha and Vs; and ONE patch list and ONE set
 * of tiles of W, sized for the segment that needs the most (the segments' scans run one after the other). */
int sf_local_scan_banded_multi_max_patch(const sf_segment* segs, int nseg, const sf_model_desc* const* models);
size_t sf_local_scan_banded_multi_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                     const int* h_cand_ptr);
int sf_local_scan_banded_multi_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models, const double* d_cand,
                                        const int* h_cand_ptr, double* d_out, double* d_lnl, double* d_log_scale, int* d_info,
                                        void* d_work, size_t work_bytes, void* stream);
/* The averaged proposal of a scan: for B walkers and ncand candidates with d_out[(b * ncand + q) * 3 + 0 .. 2] = quad, trace,
 * fisher (one segment's slice of the call above, or the output of a single-order scan), per candidate q the score statistic z =
 * U / sqrt(fisher) and the Newton step amp = U / fisher with U = (quad - trace) / 2 -- both NaN where fisher == 0 -- added over
 * the walkers with d_info[b] == 0 in ascending b (s = v_0; s = s + v_1; ...) and divided by their number: d_mean[2 q] = mean z,
 * d_mean[2 q + 1] = mean amp.  *d_count (DEVICE) receives the number of walkers used; with none the means are NaN.  One thread
 * per candidate, plain adds, no atomics: a repeated call gives the same bits.  SF_EINVAL: a null pointer, B < 1, ncand < 1. */
int sf_local_scan_mean(int B, int ncand, const double* d_out, const int* d_info, double* d_mean, int* d_count, void* stream);

/* ---- structure-exploiting solver -----------------------------------
 * Same value as sf_loglike_batch, computed without ever forming the N x N matrix: the covariance of
 * spectrum_model.py:334-363 is  C = Bd + Y^T Y  with Bd = sigma^2 + K_global + K_local + jitter
 * banded (the `r <= r0` masks of models/kernels.py:33,78 give it a half-width of ~24 ls/dv pixels)
 * and Y^T Y = X^T Sigma_w^-1 X of rank m, so a banded Cholesky plus the m x m Woodbury capacitance
 * matrix give logdet C and R^T C^-1 R in O(N W^2) flops.  `halfwidth` is the caller's bound W on
 * max |i-j| over the non-zero entries of Bd (in pixels, over the whole batch); walkers whose
 * support is wider get info = SF_INFO_BANDWIDTH and lnl = -inf and must be re-run through
 * sf_loglike_batch.  Requires a strictly increasing wavelength grid and
 * halfwidth <= sf_banded_max_halfwidth(ctx).  Up to sf_banded_window_halfwidth(ctx) (144 px for
 * m <= 15) the band is swept through an LDS-resident window; wider bands are factorised as bordered
 * band matrices on the 128 x 128 tile kernels of the dense factorisation with K loops limited to the
 * band -- their workspace is as large as the dense path's (cost grows with the half-width: group
 * walkers by width).  Results
 * agree with the dense path to rounding (different summation order), not bit for bit. */
int sf_banded_max_halfwidth(const sf_ctx* ctx);
int sf_banded_window_halfwidth(const sf_ctx* ctx);
size_t sf_banded_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int halfwidth);
int sf_loglike_banded_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params,
                            int halfwidth, double* d_lnl, double* d_logdet, double* d_sqmah,
                            double* d_resid, double* d_log_scale, int* d_info, void* d_work,
                            size_t work_bytes, void* stream);

/* Stand-alone banded kernel: for `batch` symmetric positive definite band matrices in lower band
 * storage d_band[b*stride + i*ldb + d] = A[i][i-d] (0 <= d <= halfwidth) and nrhs (<= 48) right-hand
 * sides d_rhs[b*rhs_stride + r*ldr + i], returns d_logdet[b] = log det A and
 * d_gram[b][r][c] = rhs_r^T A^-1 rhs_c (nrhs x nrhs, row-major).  d_info[b] (zeroed by the call) =
 * 1-based column of the first non-positive pivot.  (scipy.linalg.cholesky_banded + solves.) */
int sf_band_logdet_gram_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride,
                              int batch, const double* d_rhs, int nrhs, int ldr, int64_t rhs_stride,
                              double* d_logdet, double* d_gram, int* d_info, void* stream);

/* Test aid: sf_band_logdet_gram_batch (same arguments up to d_info, same results) with the form of its sweep chosen by the
 * caller.  form 0: one sweep per matrix, exactly what sf_band_logdet_gram_batch runs; no workspace (d_work may be NULL).
 * form 1: the two-sided sweep of the likelihood (two half sweeps per matrix, the merge of what they leave of the separator, a
 * third sweep over it); needs n a multiple of 16 and n / 16 >= 3 nbr - 1 block columns, nbr = max(3, (halfwidth + 31) / 16).
 * form -1: whichever of the two sf_loglike_banded_batch would run for this n, halfwidth and batch on the current device.
 * Forms 1 and -1 take a workspace of sf_debug_band_forms_workspace_bytes (0 for form 0 and for arguments the call refuses).
 * d_info[b] (zeroed by the call) = 1-based column of the first non-positive pivot, in the caller's numbering in every form.
 * SF_EINVAL, before anything is enqueued, for a null pointer, another form, a shape form 1 cannot take, nrhs outside 1 .. 48
 * or a half-width beyond the LDS window at that nrhs; SF_ENOMEM for a short workspace.  Never synchronises. */
size_t sf_debug_band_forms_workspace_bytes(int n, int halfwidth, int batch, int nrhs, int form);
int sf_debug_band_forms_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride, int batch, const double* d_rhs,
                              int nrhs, int ldr, int64_t rhs_stride, double* d_logdet, double* d_gram, int* d_info, int form,
                              void* d_work, size_t work_bytes, void* stream);

/* Stand-alone banded solve, the counterpart of sf_band_logdet_gram_batch that keeps the factor: for the same band matrices
 * and right-hand sides (nrhs in 1 .. 48) returns d_x[b*x_stride + r*ldx + i] = (A^-1 rhs_r)_i, i < n  (scipy.linalg.
 * cholesky_banded + cho_solve_banded), d_logdet[b] and, if d_gram is not NULL, the same Gram matrix.  d_band is not
 * modified: the factor goes to the workspace (sf_band_solve_workspace_bytes; 0 for arguments the call refuses), about
 * n (halfwidth + 32 + nrhs) doubles per matrix.  d_info[b] (zeroed by the call) = 1-based column of the first non-positive
 * pivot; such a matrix gets NaN in every entry of its x.  Only half-widths the LDS window takes (144 for nrhs <= 16, 128 for
 * nrhs <= 32, 112 beyond); ldx >= n.  SF_EINVAL, before anything is enqueued, for a null pointer, such a half-width or
 * nrhs outside 1 .. 48; SF_ENOMEM for a short workspace.  Never synchronises. */
size_t sf_band_solve_workspace_bytes(int n, int halfwidth, int batch, int nrhs);
int sf_band_solve_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride, int batch, const double* d_rhs,
                        int nrhs, int ldr, int64_t rhs_stride, double* d_x, int ldx, int64_t x_stride, double* d_logdet,
                        double* d_gram, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The mean-flux gradient of sf_loglike_mean_grad_batch (same h_slots, d_grad rows, refusals and NaN rows) on the band +
 * Woodbury solver: band fill and transforms as sf_loglike_banded_batch, the band sweep keeping its factor, the capacitance
 * step (d_lnl, d_info as sf_loglike_banded_batch reports them), a backward sweep giving T = Bd^-1 [r, Y^T], the mix
 * [alpha, V] = T M with the (1 + m) x (1 + m) matrix M of the Woodbury identity, then the dense call's contraction.
 * d_resid (may be NULL): [B][n], model flux minus data flux.  halfwidth as for sf_loglike_banded_batch but at most
 * sf_banded_window_halfwidth(ctx) -- beyond it SF_EINVAL (use sf_loglike_mean_grad_batch); a walker whose support is wider
 * than halfwidth gets SF_INFO_BANDWIDTH, -inf and a NaN row.  Values agree with the dense call to rounding, not bit for bit;
 * a repeated call, a call on a sub-batch and a call with a subset of the slots give the same bits.  Never synchronises. */
size_t sf_loglike_banded_mean_grad_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int halfwidth,
                                                   int nslots);
int sf_loglike_banded_mean_grad_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, int halfwidth,
                                      const int* h_slots, int nslots, double* d_lnl, double* d_grad, int grad_stride,
                                      double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* Stand-alone selected inversion, the counterpart of sf_band_solve_batch for the inverse itself: for the same band matrices
 * returns the entries of Sigma = A^-1 inside the band, d_out[b*out_stride + i*ldo + d] = Sigma[i][i-d] for
 * 0 <= d <= min(i, halfwidth), i < n (the band storage of d_band; nothing else of d_out is written), and d_logdet[b], by
 * the keeping sweep and Takahashi's recurrence over its factor, backwards: O(n halfwidth^2) per matrix, exact on the band.
 * The keeping sweep needs at least one right-hand side: the call feeds it one row of n zeros from the workspace, shared by the
 * batch, so d_logdet has the bits sf_band_solve_batch gives for these matrices.  d_band is not modified; the workspace
 * (sf_band_selinv_workspace_bytes; 0 for arguments the call refuses) holds the factor, about n (halfwidth + 48) doubles per
 * matrix.  d_info[b] (zeroed by the call) = 1-based column of the first non-positive pivot; such a matrix gets NaN in every
 * entry of its band.  Every half-width the LDS window takes (up to 144).  SF_EINVAL, before anything is enqueued, for a null
 * pointer, a half-width outside the window or ldb / ldo < halfwidth + 1; SF_ENOMEM for a short workspace.  Never synchronises. */
size_t sf_band_selinv_workspace_bytes(int n, int halfwidth, int batch);
int sf_band_selinv_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride, int batch, double* d_out, int ldo,
                         int64_t out_stride, double* d_logdet, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The likelihood gradient on the band + Woodbury solver in one call: one band fill, one keeping sweep, the capacitance step
 * and one backward sweep; then the nslots mean-flux columns exactly as sf_loglike_banded_mean_grad_batch makes them (nslots
 * may be 0, h_slots then NULL) and behind them, with want_cov, the covariance slots of sf_loglike_grad_batch in its order
 * (log_amp, log_ls of the global kernel if present, then mu, log_amp, log_sigma per local kernel):
 *     d lnL / d theta = 1/2 sum_{ij on the band} (alpha_i alpha_j - Sigma_ij + (Vs Vs^T)_ij) (dC / d theta)_ij,
 * C^-1 = Sigma - Vs Vs^T with Sigma = Bd^-1 on the band by selected inversion and Vs = Bd^-1 Y^T L_S^-T; dC / d theta has the
 * support of the kernel, which lies inside the band.  d_grad[b*grad_stride + j]: j < nslots the mean columns, nslots + q the
 * covariance slot q.  d_lnl, d_info, d_resid, refusals, SF_INFO_BANDWIDTH and NaN rows as in the mean call;
 * nslots == 0 without want_cov is SF_EINVAL; beyond sf_banded_window_halfwidth(ctx) SF_EINVAL (use sf_loglike_grad_batch).
 * Values agree with the dense calls to rounding, not bit for bit; the mean columns, d_lnl and d_info have the bits of
 * sf_loglike_banded_mean_grad_batch, the covariance columns the same bits whatever mean slots are asked for.  Never
 * synchronises. */
size_t sf_loglike_banded_grad_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int halfwidth, int nslots,
                                              int want_cov);
int sf_loglike_banded_grad_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, int halfwidth,
                                 const int* h_slots, int nslots, int want_cov, double* d_lnl, double* d_grad, int grad_stride,
                                 double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The residual diagnostics on the band + Woodbury solver: what sf_apply_batch with SF_APPLY_CINV, sf_pointwise_batch and
 * sf_decompose_batch give from the dense factor, from one band fill, one keeping sweep and one backward sweep.  d_rhs, nrhs,
 * ldr, rhs_stride as for sf_apply_batch (NULL: each walker's own residual, nrhs == 1; rhs_stride == 0: one block shared by the
 * walkers).  With k = nrhs right-hand sides the sweep carries the k + m rows [R; Y] (NULL: the gradient call's [r; Y]) and
 *     alpha_j = T_rj - T_Y S^-1 G_Y,rj,   T = Bd^-1 [R^T, Y^T],  G the sweep's Gram matrix,  S = I + G_YY = L_S L_S^T
 * goes to d_alpha[B][nrhs][n] (required).  Optional, not computed when NULL: d_cinv_diag[B][n] = diag(C^-1) = diag(Sigma) -
 * rowsum(Vs^2), Sigma = Bd^-1 on the band by selected inversion and Vs = T_Y L_S^-T (the sum over the m columns ascending);
 * d_cov_diag[B][n] = diag(C) of the matrix that is factorised, jitter included: the filled band's diagonal plus colsum(Y^2);
 * d_comp[B][3 + n_local][nrhs][n] = K_k alpha in the component order of sf_decompose_batch, by the same launches.  d_flux
 * [B][n] and d_info [B] may be NULL; d_info has the codes of sf_loglike_banded_batch, SF_INFO_BANDWIDTH included (with caller
 * right-hand sides there is no residual to be NaN: SF_INFO_NAN then says that logdet(Bd) is).  A walker with info != 0 gets NaN
 * in every row of every output.
 * The call takes every nrhs for which m + nrhs rows fit the LDS window at this half-width: at most 48 rows in all, the widest
 * half-width falling from 144 to 128 to 112 as the 16-row blocks of right-hand sides grow.  sf_diagnose_banded_max_nrhs: the
 * largest such nrhs, 0 if not even one fits (or the grid is not strictly increasing), SF_EINVAL for a bad context; more
 * right-hand sides go in several calls.  SF_EINVAL, before anything is enqueued, for B outside 1 .. 65535, nrhs < 1, m + nrhs
 * beyond the window (use sf_diagnose_banded_max_nrhs, or sf_pointwise_batch / sf_decompose_batch), a null d_params, d_alpha or
 * d_work, rhs_stride < 0, nrhs != 1 without d_rhs, ldr < n, a grid that is not strictly increasing, a bad context or model;
 * SF_ENOMEM for a short workspace (sf_diagnose_banded_workspace_bytes: 0 for whatever the call refuses).  Values agree with
 * the dense calls to rounding, not bit for bit; every sum has a fixed order, so a repeated call and a call on a sub-batch of
 * the walkers at the same halfwidth and nrhs give the same bits; the two diagonals do not depend on the right-hand sides.
 * The band is filled entry by entry (the likelihood calls tabulate the global kernel per diagonal on a log-uniform grid, which
 * is off by the rounding of the grid: inside the likelihood's tolerance, not inside the bound diag(C^-1) is held to).  Never
 * synchronises. */
int sf_diagnose_banded_max_nrhs(const sf_ctx* ctx, int halfwidth);
size_t sf_diagnose_banded_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int halfwidth, int nrhs,
                                          int want_cinv_diag, int want_comp);
int sf_diagnose_banded_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, int halfwidth,
                             const double* d_rhs, int nrhs, int ldr, int64_t rhs_stride, double* d_alpha, double* d_cinv_diag,
                             double* d_cov_diag, double* d_comp, double* d_flux, int* d_info, void* d_work, size_t work_bytes,
                             void* stream);

/* The Fisher matrix of sf_fisher_mean_batch (same h_slots, d_fisher layout, slot checks and NaN matrices) on the band + Woodbury
 * solver, from ONE sweep: band fill and transforms as sf_loglike_banded_batch, then the sweep -- the likelihood's, not the keeping
 * one, twisted where that pays -- over the 1 + m + nslots rows [r; Y; J].  With its Gram matrix G and S = I + G_YY = L_S L_S^T,
 *     F = G_JJ - U^T U,   U = L_S^-1 G_YJ   (the sum over the m rows of U ascending),
 * so there is no kept factor, no backward sweep and no N x N matrix.  d_lnl and d_info come from the leading (1 + m)^2 block of
 * the same Gram matrix through the capacitance step of sf_loglike_banded_batch; d_resid (may be NULL): [B][n], model minus data.
 * halfwidth: at most what the LDS window takes with 1 + m + nslots rows (144 up to 16 rows, 128 up to 32, 112 up to 48) --
 * beyond it SF_EINVAL (use sf_fisher_mean_batch; the bordered-tile path of wide bands has no Fisher call); a walker whose
 * support is wider than halfwidth gets SF_INFO_BANDWIDTH, -inf and a NaN matrix.  sf_fisher_banded_max_slots: the largest nslots
 * (at most SF_MEAN_GRAD_MAX_SLOTS) whose rows fit the window at this half-width, 0 if none does, SF_EINVAL for a bad context.
 * Values agree with the dense call to rounding, not bit for bit.  A repeated call and a call on a sub-batch at the same
 * half-width and slots give the same bits.  A SUBSET OF THE SLOTS AGREES TO ROUNDING ONLY: the number of 16-row blocks picks
 * another instantiation of the sweep, so bit equality is not promised there.  SF_EINVAL before anything is enqueued as for the
 * dense call, for a null d_work, a grid that is not strictly increasing and a half-width outside the window;
 * sf_fisher_banded_mean_workspace_bytes is 0 for the same counts.  Never synchronises. */
int sf_fisher_banded_max_slots(const sf_ctx* ctx, int halfwidth);
size_t sf_fisher_banded_mean_workspace_bytes(const sf_ctx* ctx, const sf_model_desc* model, int B, int halfwidth, int nslots);
int sf_fisher_banded_mean_batch(sf_ctx* ctx, const sf_model_desc* model, int B, const double* d_params, int halfwidth,
                                const int* h_slots, int nslots, double* d_lnl, double* d_fisher, int fisher_stride,
                                double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* Timing hooks for bench.py (process-global, not thread-safe): when enabled, the batched calls
 * record HIP events on the caller's stream around each stage and around every MFMA update launch.
 * sf_profile_read synchronises those events, returns the milliseconds accumulated since the last
 * read in ms_by_stage[6] = {transforms, fill, k_gemm_nt launches (overlapping launches of the two
 * Cholesky streams merged: union of their intervals), whole potrf, solve, k_gemm_nt launches (plain
 * sum of launch durations)}, the algorithmic flops and launch count of k_gemm_nt, and the number
 * of sf_loglike_batch calls; then it resets the counters. */
int sf_profile_enable(int on);
int sf_profile_read(double* ms_by_stage, double* gemm_flops, long* gemm_launches, long* calls);

/* Emulator training likelihood (Starfish/emulator/emulator.py:602-619): the matrix
 * v11 = iPhiPhi / lambda_xi + blockdiag_c(variance_c RBF_c(grid, grid)) (emulator.py:126-128, kernels.py:5-49) built on
 * the device into the padded layout of sf_potrf_batch: d_A[npad][lda], identity block from n = m M to npad.
 * d_grid[M*P], d_hyper = {lambda_xi, variances[m], lengthscales[m*P]}, d_iphiphi[n*n].  Emulator.train calls it once per
 * objective evaluation, followed by sf_potrf_batch + sf_logdet_sqmah_batch with the right-hand side w_hat. */
int sf_emulator_v11_build(const double* d_grid, int M, int P, int m, const double* d_hyper, const double* d_iphiphi,
                          double* d_A, int npad, int lda, void* stream);

/* The same matrix (emulator.py:126-128, kernels.py:5-49) for B hyper-parameter vectors in one launch: what Emulator.train
 * (emulator.py:484-524) evaluates when the points of a simplex iteration go to the device as one batch.
 * B matrices v11(hyper_b) in the layout of sf_potrf_batch; d_R (may be NULL): B x ldr copies of w_hat, zero padded.
 * d_hyper: B rows of {lambda_xi, variances[m], lengthscales[m*P]} (raw values, not logs), row stride hyper_stride >= 1 + m + m P.
 * Matrix b at d_A + b*stride (doubles), row stride lda >= npad, npad a multiple of 64 and >= m M, identity block from m M to
 * npad; columns npad..lda of a row are never touched.  lda and stride must be even and d_A 16-byte aligned (16-byte stores).
 * lower_only: 64 x 64 tiles strictly above the diagonal are skipped (entries above the diagonal INSIDE a diagonal tile may be
 * written; a factorisation never reads them), as in sf_cov_fill_batch.  P <= 8; SF_EINVAL otherwise, nothing is written. */
int sf_emulator_v11_build_batch(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride, int B,
                                const double* d_iphiphi, double* d_A, int npad, int lda, int64_t stride, int lower_only,
                                const double* d_w_hat, double* d_R, int ldr, void* stream);

/* Emulator.log_likelihood (Starfish/emulator/emulator.py:602-619) for B hyper-parameter vectors in ONE enqueue:
 * build (lower triangle) + sf_potrf_batch + sf_logdet_sqmah_batch + finish.  d_lnl[B] = -(logdet + sqmah)/2, -inf where
 * d_info[b] != 0 (k > 0: first non-positive pivot of matrix b; SF_INFO_INTERNAL as for every batched factorisation).
 * d_logdet / d_sqmah may be NULL.  No allocation: d_work (256-byte aligned) of sf_emulator_loglike_workspace_bytes(M, m, B),
 * which holds the B matrices, the right-hand sides and the workspace of sf_potrf_batch.  Arguments are checked before
 * anything is enqueued (SF_EINVAL; SF_ENOMEM for a short workspace); the call never synchronises. */
size_t sf_emulator_loglike_workspace_bytes(int M, int m, int B);
int sf_emulator_loglike_batch(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride, int B,
                              const double* d_iphiphi, const double* d_w_hat, double* d_lnl, double* d_logdet,
                              double* d_sqmah, int* d_info, void* d_work, size_t work_bytes, void* stream);

/* The training likelihood and its gradient in the LOGS of the hyper-parameters, for B hyper-parameter vectors in ONE enqueue:
 * d lnL / d theta = 1/2 sum_ij (alpha_i alpha_j - (v11^-1)_ij) (d v11 / d theta)_ij (Rasmussen & Williams, Gaussian Processes for
 * Machine Learning, eq. 5.9), alpha = v11^-1 w_hat, with (row i = component i / M, grid point i % M)
 *     log lambda_xi:   -iPhiPhi_ij / lambda_xi                                 (every entry of the dense n x n array)
 *     log variance_c:  K_c[g,h] = variance_c exp(-1/2 sum_p ((x_gp - x_hp) / l_cp)^2)     where i / M == j / M == c, else 0
 *     log l_cp:        K_c[g,h] ((x_gp - x_hp) / l_cp)^2                                   where i / M == j / M == c, else 0
 * Sequence: the four stages of sf_emulator_loglike_batch on the same layout (d_lnl and d_info carry ITS BITS for the same
 * rows), alpha by sf_potrs_batch's SF_APPLY_CINV, X = L^-1 by the launch of sf_potri_diag_batch, every 64 x 64 block of
 * v11^-1 = X^T X of the lower triangle as sf_potri_blocks_batch forms them, contracted with the analytic entries; a small
 * fixed-order sum over block rows.  No atomics: a repeated call, and a call on a part of the rows, give the same bits.
 * d_hyper: raw rows as for sf_emulator_loglike_batch.  d_grad[b*grad_stride + s]: the derivative in the LOG of
 * hyper-parameter s, in the order of the raw row (lambda_xi, variances[m], lengthscales[m*P]); grad_stride >= 1 + m + m P,
 * entries beyond the slots are not touched.  Rows with d_info[b] != 0 get lnl = -inf and NaN in every slot.
 * Error: with u = 2^-53 and |D| the entry derivative taken in absolute value, a slot is within
 *     1/2 sum_ij (|dalpha|_i |alpha|_j + |alpha|_i |dalpha|_j + |dG|_ij) |D|_ij + (1e-13 + gamma_k) 1/2 sum_ij |A_ij| |D|_ij
 * of the exact value for the matrix that is factorised, |dalpha| and |dG| being the bounds of sf_potrs_batch and
 * sf_potri_blocks_batch above with the build's entry error (1e-13 relative) in dC, k the number of non-zero entries of D.
 * SF_EINVAL before anything is enqueued: a null pointer, M or m not positive, P outside 1 .. 8, hyper_stride or grad_stride
 * below 1 + m + m P, B outside 1 .. 65535, d_work not 256-byte aligned; SF_ENOMEM for a short workspace.  d_work:
 * what sf_emulator_loglike_grad_workspace_bytes gives for M, P, m, B (0 for bad arguments): the workspace of sf_emulator_loglike_batch,
 * then alpha (npad doubles per row), the workspace of sf_potri_blocks_batch and one double per (row, 64-row block, slot).
 * The call never synchronises. */
size_t sf_emulator_loglike_grad_workspace_bytes(int M, int P, int m, int B);
int sf_emulator_loglike_grad_batch(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride, int B,
                                   const double* d_iphiphi, const double* d_w_hat, double* d_lnl, double* d_grad,
                                   int grad_stride, int* d_info, void* d_work, size_t work_bytes, void* stream);
/* Timing aid (tools/bench_emulator_gradient.py): the contraction launches of sf_emulator_loglike_grad_batch alone, on the
 * workspace and d_info that a call of it with the same arguments left behind. */
int sf_debug_emulator_grad_contract(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride, int B,
                                    const double* d_iphiphi, double* d_grad, int grad_stride, const int* d_info, void* d_work,
                                    size_t work_bytes, void* stream);

/* Process-global switch of the persistent-kernel ("dataflow") Cholesky sequence: enable = 0 makes every later factorisation
 * take a launch sequence (kernels without waits inside), 1 restores the default choice, < 0 only queries.  Returns the
 * previous setting.  The recovery path after SF_INFO_INTERNAL.
 * The persistent kernel's workgroups wait for each other inside ONE launch: it assumes the process has the device to itself
 * (one process per GPU).  Several processes oversubscribing one device can keep each other's workgroups from becoming
 * running; the launch is then given up FAST -- as soon as no task of it has completed for 25 ms while a workgroup was waiting
 * (the longest task of the largest matrix the kernel takes, N = 16384, runs ~5 ms), or after 4 s inside one wait --
 * (SF_INFO_INTERNAL for the batch) and the caller falls back: a shared device costs the first call ~25 ms + one factorisation
 * on the launch sequences.  A process that knows it shares its device should switch the sequence off up front. */
int sf_persistent_potrf(int enable);

/* The process's record of persistent-kernel launches, for the caller's warning and for tests (host memory, no
 * synchronisation: read it after the stream that carried the aborted call has been synchronised):
 * h_out8 = {aborted launches so far, reason of the last abort (1 = a wait reached its 4-s bound, 2 = no task completed for
 * 25 ms), workgroups of that launch that had started, its grid size (fewer started than launched = the grid was not
 * co-resident: the device is shared or partitioned), 100 MHz ticks the reporting wait had lasted, tasks the launch had
 * completed, persistent launches enqueued by this process so far, 1 if the sequence is enabled}. */
int sf_persistent_potrf_status(long long* h_out8);

/* Tuning / test aid (process-global): the batched Cholesky has three launch sequences -- the fused panel kernel
 * (128-column panels, two workgroups per CU; medium batches), the unfused one (256-column panels, separate panel-solve and
 * diagonal-update launches; kept selectable) and the wide one (pairs of panels, one 16-wave workgroup per CU keeps a 128 x 256 tile: a third less HBM
 * traffic; taken when batch x 128-row slabs >= 3400 and the matrices have 2048 or more rows).
 * mode -1 = choose by batch and matrix size (default), 0 = always fused, 1 = always unfused, 2 = always wide,
 * 3 = wide for the first half of the panels, then fused (test aid: exercises the hand-over between the two),
 * 4 = dataflow: the whole factorisation as ONE persistent launch whose workgroups draw tasks and wait on exactly the tasks
 * they depend on (the default while batch x 128-column panels <= 2048, batch <= 128 and N <= 8192 -- every scalar evaluation,
 * the half-ensembles of a sampler, the per-GPU batches of a strong split; forced, it takes up to 128 panels, N = 16384, beyond
 * that the fused sequence runs instead).
 * The fused and wide sequences factorise matrices of 64 mod 128 rows in a frame shifted by 64 virtual identity rows
 * (addressing only: nothing moves in memory, the caller's layout and the pivot index reported in d_info are unchanged).
 * Same results to rounding. */
int sf_debug_cholesky_sequence(int mode);

/* Tuning aid: one wave spins for `wall_ticks_100mhz` ticks of the 100 MHz wall clock on `stream` and
 * writes {shader-clock ticks, wall ticks} to d_out2[2] -> sustained shader clock under load. */
int sf_debug_clock_probe(long long* d_out2, long long wall_ticks_100mhz, void* stream);

/* Measurement aid (bench.py's fill leg): a plain streaming write of `count` doubles (16-byte stores, one pass, nothing
 * read) -- the HBM write rate this box sustains, next to which the write-only covariance fill is priced. */
int sf_debug_stream_write(double* d_dst, size_t count, double value, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STARFISH_AMD_H */
