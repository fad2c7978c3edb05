// C-ABI host layer: the context-free entry points (Starfish's free functions, the stand-alone Cholesky stage, emulator
// training) and the tuning / debug hooks.
#include <vector>

#include "sf_hostmath.h"
#include "sf_prof.h"
#include "sf_work.h"

extern "C" int sf_global_cov(const double* d_wave, int n, double amplitude, double lengthscale, double* d_out,
                             void* stream) {
    if (!d_wave || !d_out || n < 0) {
        sf_set_error("sf_global_cov: bad argument");
        return SF_EINVAL;
    }
    return sf_launch_global_cov(d_wave, n, amplitude, lengthscale, d_out, (hipStream_t)stream);
}
extern "C" int sf_local_cov(const double* d_wave, int n, double amplitude, double mu, double sigma,
                            int accumulate, double* d_out, void* stream) {
    if (!d_wave || !d_out || n < 0) {
        sf_set_error("sf_local_cov: bad argument");
        return SF_EINVAL;
    }
    return sf_launch_local_cov(d_wave, n, amplitude, mu, sigma, accumulate, d_out, (hipStream_t)stream);
}

extern "C" size_t sf_fft_workspace_bytes(int rows, int nf) {
    if (rows <= 0 || nf <= 0) return 0;
    return carve_fft(rows, nf, nullptr, 0).bytes;
}
static int broaden_free(const double* d_flux, int rows, int nf, double dv, int kind, double param,
                        double* d_out, void* d_work, size_t work_bytes, hipStream_t s) {
    if (!d_flux || !d_out || rows <= 0 || !d_work || work_bytes < sf_fft_workspace_bytes(rows, nf)) {
        sf_set_error("broaden: bad argument or workspace");
        return SF_EINVAL;
    }
    if (nf < 2 || (nf & (nf - 1))) {
        sf_set_error("broaden: nf=%d must be a power of two", nf);
        return SF_EINVAL;
    }
    const FftWork w = carve_fft(rows, nf, d_work, work_bytes);
    std::vector<double> tw;
    make_twiddles(nf, tw);
    // pageable host -> device copy: synchronous w.r.t. the host buffer, safe to free afterwards
    SF_HIP(hipMemcpyAsync(w.tw, tw.data(), sizeof(double) * (size_t)nf, hipMemcpyHostToDevice, s));
    SF_HIP(hipStreamSynchronize(s));
    sf_broaden_args a;
    a.in = d_flux;
    a.spec = nullptr;
    a.B = 1;
    a.rows = rows;
    a.nf = nf;
    a.tw = (const double2*)w.tw;
    a.dv = dv;
    a.kind = kind;
    a.params = nullptr;
    a.pstride = 0;
    a.poff = 0;
    a.scalar_param = param;
    a.out = d_out;
    a.ob = 0;
    a.orow = nf;
    a.oelem = 1;
    a.gscratch = w.scratch;
    a.mult = nullptr;
    a.info = nullptr;
    return sf_launch_broaden(a, s);
}
extern "C" int sf_rotational_broaden(const double* d_flux, int rows, int nf, double dv, double vsini,
                                     double* d_out, void* d_work, size_t work_bytes, void* stream) {
    if (!(vsini > 0.0)) {
        sf_set_error("vsini must be positive");  // transforms.py:121-122
        return SF_EINVAL;
    }
    return broaden_free(d_flux, rows, nf, dv, 1, vsini, d_out, d_work, work_bytes, (hipStream_t)stream);
}
extern "C" int sf_instrumental_broaden(const double* d_flux, int rows, int nf, double dv, double fwhm,
                                       double* d_out, void* d_work, size_t work_bytes, void* stream) {
    if (fwhm < 0.0) {
        sf_set_error("FWHM must be non-negative");  // transforms.py:78-79
        return SF_EINVAL;
    }
    return broaden_free(d_flux, rows, nf, dv, 2, fwhm, d_out, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" size_t sf_resample_workspace_bytes(int n, int rows) {
    if (n <= 0 || rows <= 0) return 0;
    return carve_resample(n, rows, nullptr, 0).bytes;
}
extern "C" int sf_resample(const double* h_wave, int n, const double* d_flux, int rows, const double* d_new_wave,
                           int nq, double* d_out, void* d_work, size_t work_bytes, void* stream) {
    // (no queries: the caller's query and output buffers may be empty, i.e. null)
    if (!h_wave || !d_flux || (nq > 0 && (!d_new_wave || !d_out)) || rows <= 0 || nq < 0 || !d_work ||
        work_bytes < sf_resample_workspace_bytes(n, rows)) {
        sf_set_error("sf_resample: bad argument or workspace");
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    std::vector<double> t, Lf, Uf, rdiag;
    int rc = quintic_collocation_lu(h_wave, n, t, Lf, Uf, rdiag);
    if (rc) return rc;
    const ResampleWork w = carve_resample(n, rows, d_work, work_bytes);
    SF_HIP(hipMemcpyAsync(w.t, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, s));
    SF_HIP(hipMemcpyAsync(w.Lf, Lf.data(), sizeof(double) * Lf.size(), hipMemcpyHostToDevice, s));
    SF_HIP(hipMemcpyAsync(w.Uf, Uf.data(), sizeof(double) * Uf.size(), hipMemcpyHostToDevice, s));
    SF_HIP(hipMemcpyAsync(w.rdiag, rdiag.data(), sizeof(double) * rdiag.size(), hipMemcpyHostToDevice, s));
    SF_HIP(hipMemcpyAsync(w.coef, d_flux, sizeof(double) * (size_t)n * rows, hipMemcpyDeviceToDevice, s));
    SF_HIP(hipStreamSynchronize(s));  // the host vectors go out of scope below
    rc = sf_launch_spline_solve(w.coef, 1, rows, 0, n, 1, n, w.Lf, w.Uf, w.rdiag, s);
    if (rc) return rc;
    if (nq == 0) return SF_OK;
    return sf_launch_spline_eval(w.coef, rows, n, w.t, d_new_wave, nq, d_out, s);
}

// `count` host doubles ride in a small device buffer of `cap` doubles owned by this call: uploaded on s, run(buffer)
// enqueues its user, then the stream is synchronised and the buffer freed (also when the upload or the launch failed)
template <class F>
static int with_device_copy(const double* h_src, size_t count, size_t cap, hipStream_t s, F&& run) {
    double* d = nullptr;
    SF_HIP(hipMalloc((void**)&d, sizeof(double) * cap));
    int rc = SF_OK;
    if (hipMemcpyAsync(d, h_src, sizeof(double) * count, hipMemcpyHostToDevice, s) != hipSuccess) rc = SF_EHIP;
    if (!rc) rc = run(d);
    (void)hipStreamSynchronize(s);
    (void)hipFree(d);
    return rc;
}

extern "C" int sf_chebyshev_correct(const double* d_wave, int n, double wave_max, const double* d_flux, int rows,
                                    const double* h_coeffs, int ncoef, double* d_out, void* stream) {
    if (!d_wave || !d_flux || !h_coeffs || !d_out || n < 0 || rows <= 0 || ncoef < 1 || ncoef > 64) {
        sf_set_error("sf_chebyshev_correct: bad argument");
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    return with_device_copy(h_coeffs, ncoef, 64, s, [&](const double* dco) {
        return sf_launch_cheb_rows(d_wave, n, wave_max, d_flux, rows, dco, ncoef, d_out, s);
    });
}

extern "C" int sf_extinct_ccm89(const double* d_wave, int n, const double* d_flux, int rows, double Av, double Rv,
                                double* d_out, void* stream) {
    if (!d_wave || !d_flux || !d_out || n < 0 || rows <= 0 || !(Rv > 0.0)) {
        sf_set_error("sf_extinct_ccm89: bad argument");
        return SF_EINVAL;
    }
    return sf_launch_extinct_rows(d_wave, n, d_flux, rows, Av, Rv, 0, d_out, (hipStream_t)stream);
}
extern "C" int sf_extinct(const double* d_wave, int n, const double* d_flux, int rows, double Av, double Rv, int law,
                          double* d_out, void* stream) {
    if (!d_wave || !d_flux || !d_out || n < 0 || rows <= 0 || !(Rv > 0.0) || law < 0 || law > 4) {
        sf_set_error("sf_extinct: bad argument");
        return SF_EINVAL;
    }
    if (law <= 2) return sf_launch_extinct_rows(d_wave, n, d_flux, rows, Av, Rv, law, d_out, (hipStream_t)stream);
    std::vector<double> tab;
    int rc = extinct_spline_table(law, Rv, tab);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    return with_device_copy(tab.data(), tab.size(), tab.size(), s, [&](const double* dtab) {
        return sf_launch_extinct_spline_rows(d_wave, n, d_flux, rows, Av, Rv, dtab, d_out, s);
    });
}

extern "C" size_t sf_potrf_workspace_bytes(int n, int batch) {
    if (n <= 0 || batch <= 0) return 0;
    return carve_potrf(n, batch, nullptr, 0).bytes;
}
extern "C" int sf_potrf_batch(double* d_A, int n, int lda, int64_t stride, int batch, int* d_info, void* d_work,
                              size_t work_bytes, void* stream) {
    if (!d_A || !d_info || !d_work || work_bytes < sf_potrf_workspace_bytes(n, batch)) {
        sf_set_error("sf_potrf_batch: bad argument or workspace");
        return SF_EINVAL;
    }
    double* ltbuf = carve_potrf(n, batch, d_work, work_bytes).ltbuf;
    ProfScope ps((hipStream_t)stream, PS_POTRF);
    return sf_launch_potrf(d_A, n, lda, stride, batch, d_info, ltbuf, nullptr, 0, (hipStream_t)stream);
}
extern "C" int sf_logdet_sqmah_batch(const double* d_L, int n, int lda, int64_t stride, int batch,
                                     const double* d_R, int ldr, void* d_work, size_t work_bytes,
                                     double* d_logdet, double* d_sqmah, void* stream) {
    if (!d_L || !d_R || !d_logdet || !d_sqmah || ldr < n) {
        sf_set_error("sf_logdet_sqmah_batch: bad argument");
        return SF_EINVAL;
    }
    double* z = nullptr;
    if (d_work && work_bytes >= sf_potrf_workspace_bytes(n, batch)) z = carve_potrf(n, batch, d_work, work_bytes).z;
    ProfScope ps((hipStream_t)stream, PS_SOLVE);
    return sf_launch_logdet_sqmah(d_L, n, lda, stride, batch, d_R, ldr, z, d_logdet, d_sqmah,
                                  (hipStream_t)stream);
}
// every argument check of the factor's application, before any HIP call
static int potrs_args_ok(const double* d_L, int n, int lda, int batch, int op, const double* d_rhs, int nrhs, int ldr,
                         int64_t rhs_stride, const double* d_out, int ldo, int64_t out_stride) {
    if (!d_L || !d_rhs || !d_out) {
        sf_set_error("sf_potrs_batch: d_L, d_rhs and d_out are required");
        return SF_EINVAL;
    }
    if (n <= 0 || n % SF_LEAF != 0 || lda < n || batch < 1) {
        sf_set_error("sf_potrs_batch: n=%d must be a positive multiple of %d, lda=%d >= n, batch=%d >= 1", n, SF_LEAF, lda, batch);
        return SF_EINVAL;
    }
    if (nrhs < 1 || ldr < n || ldo < n || rhs_stride < 0 || out_stride < 0) {
        sf_set_error("sf_potrs_batch: nrhs=%d must be at least 1, ldr=%d and ldo=%d at least n=%d, strides not negative", nrhs,
                     ldr, ldo, n);
        return SF_EINVAL;
    }
    if (op < SF_APPLY_L || op > SF_APPLY_CINV) {
        sf_set_error("sf_potrs_batch: unknown op %d (SF_APPLY_L 0, SF_APPLY_LINV 1, SF_APPLY_LINVT 2, SF_APPLY_CINV 3)", op);
        return SF_EINVAL;
    }
    if (d_out == d_rhs && (rhs_stride == 0 || ldo != ldr || out_stride != rhs_stride)) {
        sf_set_error("sf_potrs_batch: in place (d_out == d_rhs) needs rhs_stride != 0, ldo == ldr and out_stride == rhs_stride");
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" int sf_potrs_batch(const double* d_L, int n, int lda, int64_t stride, int batch, int op, const double* d_rhs,
                              int nrhs, int ldr, int64_t rhs_stride, double* d_out, int ldo, int64_t out_stride, void* stream) {
    SF_CHECK(potrs_args_ok(d_L, n, lda, batch, op, d_rhs, nrhs, ldr, rhs_stride, d_out, ldo, out_stride));
    return sf_launch_chol_apply(d_L, n, lda, stride, batch, op, d_rhs, nrhs, ldr, rhs_stride, d_out, ldo, out_stride,
                                (hipStream_t)stream);
}

extern "C" size_t sf_potri_diag_workspace_bytes(int n, int batch) {
    if (n <= 0 || n % SF_LEAF != 0 || batch <= 0) return 0;
    return carve_potri(n, batch, nullptr, 0).bytes;
}
extern "C" int sf_potri_diag_batch(double* d_L, int n, int lda, int64_t stride, int batch, double* d_out, int64_t out_stride,
                                   void* d_work, size_t work_bytes, void* stream) {
    if (!d_L || !d_out || !d_work) {
        sf_set_error("sf_potri_diag_batch: d_L, d_out and d_work are required");
        return SF_EINVAL;
    }
    if (n <= 0 || n % SF_LEAF != 0 || lda < n || batch < 1 || out_stride < n) {
        sf_set_error("sf_potri_diag_batch: n=%d must be a positive multiple of %d, lda=%d >= n, batch=%d >= 1, out_stride=%lld >= n",
                     n, SF_LEAF, lda, batch, (long long)out_stride);
        return SF_EINVAL;
    }
    const PotriWork w = carve_potri(n, batch, d_work, work_bytes);
    if (work_bytes < w.bytes) {
        sf_set_error("sf_potri_diag_batch: workspace too small: have %zu, need %zu", work_bytes, w.bytes);
        return SF_EINVAL;
    }
    return sf_launch_chol_inverse_diag(d_L, n, lda, stride, batch, w.winv, d_out, out_stride, (hipStream_t)stream);
}

extern "C" size_t sf_potri_blocks_workspace_bytes(int n, int batch) {
    if (n <= 0 || n % SF_LEAF != 0 || batch <= 0) return 0;
    return carve_potri(n, batch, nullptr, 0, true).bytes;
}
extern "C" int sf_potri_blocks_batch(double* d_L, int n, int lda, int64_t stride, int batch, const int* d_pairs, int npairs,
                                     double* d_out, void* d_work, size_t work_bytes, void* stream) {
    if (!d_L || !d_pairs || !d_out || !d_work) {
        sf_set_error("sf_potri_blocks_batch: d_L, d_pairs, d_out and d_work are required");
        return SF_EINVAL;
    }
    if (n <= 0 || n % SF_LEAF != 0 || lda < n || batch < 1 || npairs < 1) {
        sf_set_error("sf_potri_blocks_batch: n=%d must be a positive multiple of %d, lda=%d >= n, batch=%d >= 1, npairs=%d >= 1", n,
                     SF_LEAF, lda, batch, npairs);
        return SF_EINVAL;
    }
    const PotriWork w = carve_potri(n, batch, d_work, work_bytes, true);
    if (work_bytes < w.bytes) {
        sf_set_error("sf_potri_blocks_batch: workspace too small: have %zu, need %zu", work_bytes, w.bytes);
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(sf_launch_chol_inverse_diag(d_L, n, lda, stride, batch, w.winv, w.diag, n, s));
    return sf_launch_cinv_blocks(d_L, n, lda, stride, batch, w.winv, d_pairs, npairs, d_out, s);
}

extern "C" int sf_emulator_v11_build(const double* d_grid, int M, int P, int m, const double* d_hyper, const double* d_iphiphi,
                                     double* d_A, int npad, int lda, void* stream) {
    return sf_launch_v11_build(d_grid, M, P, m, d_hyper, d_iphiphi, d_A, npad, lda, (hipStream_t)stream);
}
extern "C" int sf_emulator_v11_build_batch(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride,
                                           int B, const double* d_iphiphi, double* d_A, int npad, int lda, int64_t stride,
                                           int lower_only, const double* d_w_hat, double* d_R, int ldr, void* stream) {
    return sf_launch_v11_build_batch(d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, d_A, npad, lda, stride, lower_only,
                                     d_w_hat, d_R, ldr, (hipStream_t)stream);
}

// The training objective for B hyper-parameter rows, alone or with its gradient in the logs of the hyper-parameters
// (workspace: carve_emu_train, with the grid axes for the gradient)
static bool emu_counts_ok(int M, int P, int m, int B) {
    return M > 0 && m > 0 && P >= 1 && P <= 8 && B >= 1 && B <= 65535 && (int64_t)m * M <= (1 << 30) &&
           (int64_t)m * (P + 1) < (1 << 30);
}
extern "C" size_t sf_emulator_loglike_workspace_bytes(int M, int m, int B) { return carve_emu_train(M, m, B, nullptr, 0).bytes; }
extern "C" size_t sf_emulator_loglike_grad_workspace_bytes(int M, int P, int m, int B) {
    if (!emu_counts_ok(M, P, m, B)) return 0;
    return carve_emu_train(M, m, B, nullptr, 0, P).bytes;
}
// every argument check of the three calls below, before any HIP call, and their workspace.  grad_stride: NULL for a call
// without a gradient, whose workspace ends behind the factorisation's
static int emu_open(const char* name, bool required, int M, int P, int m, int hyper_stride, int B, const int* grad_stride,
                    void* d_work, size_t work_bytes, EmuTrainWork* w) {
    if (!required || !d_work) {
        sf_set_error("%s: a required pointer is NULL", name);
        return SF_EINVAL;
    }
    if (!emu_counts_ok(M, P, m, B)) {
        sf_set_error("%s: M=%d and m=%d must be positive, P=%d in 1 .. 8, B=%d in 1 .. 65535", name, M, m, P, B);
        return SF_EINVAL;
    }
    const int slots = sf_emu_grad_slots(m, P);
    if (hyper_stride < slots || (grad_stride && *grad_stride < slots)) {
        sf_set_error("%s: hyper_stride=%d and, with a gradient, grad_stride=%d must be at least 1 + m + m P = %d", name, hyper_stride,
                     grad_stride ? *grad_stride : 0, slots);
        return SF_EINVAL;
    }
    if ((uintptr_t)d_work & 255) {
        sf_set_error("%s: d_work must be 256-byte aligned", name);
        return SF_EINVAL;
    }
    *w = carve_emu_train(M, m, B, d_work, work_bytes, grad_stride ? P : 0);
    if (work_bytes < w->bytes) {
        sf_set_error("%s: workspace of %zu bytes, %zu needed", name, work_bytes, w->bytes);
        return SF_ENOMEM;
    }
    return SF_OK;
}
// build (lower triangle, R = w_hat), factorisation, logdet / sqmah, finish: the four stages of the likelihood
static int emu_loglike_stages(const EmuTrainWork& w, const double* d_grid, int M, int P, int m, const double* d_hyper,
                              int hyper_stride, int B, const double* d_iphiphi, const double* d_w_hat, double* d_lnl,
                              double* d_logdet, double* d_sqmah, int* d_info, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    double* logdet = d_logdet ? d_logdet : w.logdet;
    double* sqmah = d_sqmah ? d_sqmah : w.sqmah;
    int rc = sf_launch_v11_build_batch(d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, w.A, w.npad, w.lda, w.stride, 1, d_w_hat,
                                       w.R, w.npad, s);
    if (rc) return rc;
    rc = sf_potrf_batch(w.A, w.npad, w.lda, w.stride, B, w.info_c, w.potrf, w.potrf_bytes, stream);
    if (rc) return rc;
    rc = sf_logdet_sqmah_batch(w.A, w.npad, w.lda, w.stride, B, w.R, w.npad, w.potrf, w.potrf_bytes, logdet, sqmah, stream);
    if (rc) return rc;
    ProfScope ps(s, PS_SOLVE);
    return sf_launch_finish(B, logdet, sqmah, w.info_c, nullptr, d_lnl, d_info, s);
}
extern "C" int sf_emulator_loglike_batch(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride,
                                         int B, const double* d_iphiphi, const double* d_w_hat, double* d_lnl, double* d_logdet,
                                         double* d_sqmah, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    EmuTrainWork w;
    SF_CHECK(emu_open("sf_emulator_loglike_batch", d_grid && d_hyper && d_iphiphi && d_w_hat && d_lnl && d_info, M, P, m,
                      hyper_stride, B, nullptr, d_work, work_bytes, &w));
    return emu_loglike_stages(w, d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, d_w_hat, d_lnl, d_logdet, d_sqmah, d_info,
                              stream);
}
// 1/2 sum (alpha alpha^T - v11^-1) o dv11/dtheta from the alpha and the X the stages before left in the workspace
static int emu_grad_contract(const EmuTrainWork& w, const double* d_grid, int M, int P, int m, const double* d_hyper,
                             int hyper_stride, int B, const double* d_iphiphi, const int* d_info, double* d_grad, int grad_stride,
                             hipStream_t s) {
    return sf_launch_emu_grad(d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, w.A, w.npad, w.lda, w.stride, w.winv, w.alpha,
                              w.npad, d_info, w.part, d_grad, grad_stride, s);
}
extern "C" int sf_emulator_loglike_grad_batch(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride,
                                              int B, const double* d_iphiphi, const double* d_w_hat, double* d_lnl, double* d_grad,
                                              int grad_stride, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    EmuTrainWork w;
    SF_CHECK(emu_open("sf_emulator_loglike_grad_batch", d_grid && d_hyper && d_iphiphi && d_w_hat && d_lnl && d_grad && d_info, M, P, m,
                      hyper_stride, B, &grad_stride, d_work, work_bytes, &w));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(emu_loglike_stages(w, d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, d_w_hat, d_lnl, nullptr, nullptr, d_info,
                                stream));
    // (the factor is applied first: the inverse's launch takes the strict upper triangle of the matrices as scratch)
    SF_CHECK(sf_launch_chol_apply(w.A, w.npad, w.lda, w.stride, B, SF_APPLY_CINV, w.R, 1, w.npad, w.npad, w.alpha, w.npad, w.npad, s));
    SF_CHECK(sf_launch_chol_inverse_diag(w.A, w.npad, w.lda, w.stride, B, w.winv, w.cinv_diag, w.npad, s));
    return emu_grad_contract(w, d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, d_info, d_grad, grad_stride, s);
}
// The contraction launches of sf_emulator_loglike_grad_batch alone, on the workspace and d_info a call with the same arguments
// left (tools/bench_emulator_gradient.py times them)
extern "C" int sf_debug_emulator_grad_contract(const double* d_grid, int M, int P, int m, const double* d_hyper, int hyper_stride,
                                               int B, const double* d_iphiphi, double* d_grad, int grad_stride, const int* d_info,
                                               void* d_work, size_t work_bytes, void* stream) {
    EmuTrainWork w;
    SF_CHECK(emu_open("sf_debug_emulator_grad_contract", d_grid && d_hyper && d_iphiphi && d_grad && d_info, M, P, m, hyper_stride, B,
                      &grad_stride, d_work, work_bytes, &w));
    return emu_grad_contract(w, d_grid, M, P, m, d_hyper, hyper_stride, B, d_iphiphi, d_info, d_grad, grad_stride,
                             (hipStream_t)stream);
}

// Recovery switch of the callers (process-global): after a batch came back SF_INFO_INTERNAL the host layer turns the
// persistent-kernel sequence off and re-runs the batch on a launch sequence (starfish_amd/_runtime.py).
extern "C" int sf_persistent_potrf(int enable) { return sf_set_persistent_potrf(enable); }
extern "C" int sf_persistent_potrf_status(long long* h_out8) {
    if (!h_out8) {
        sf_set_error("sf_persistent_potrf_status: h_out8 is required");
        return SF_EINVAL;
    }
    return sf_persistent_potrf_read_status(h_out8);
}

// Tuning / test aid: pin the launch sequence of the batched Cholesky (process-global).
extern "C" int sf_debug_cholesky_sequence(int mode) { return sf_set_cholesky_sequence(mode); }

// Tuning aid (not part of the Starfish surface): sustained shader clock while other streams are busy.
extern "C" int sf_debug_stream_write(double* d_dst, size_t count, double value, void* stream) {
    if (!d_dst) {
        sf_set_error("sf_debug_stream_write: d_dst is required");
        return SF_EINVAL;
    }
    return sf_launch_stream_write(d_dst, count, value, (hipStream_t)stream);
}

extern "C" int sf_debug_clock_probe(long long* d_out2, long long wall_ticks_100mhz, void* stream) {
    return sf_launch_clock_probe(d_out2, wall_ticks_100mhz, (hipStream_t)stream);
}
