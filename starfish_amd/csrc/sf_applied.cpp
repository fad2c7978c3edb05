// C-ABI host layer: the calls that run the likelihood's sequence and then work on the Cholesky factor (sf_apply_batch,
// sf_decompose_batch, sf_pointwise_batch, sf_loglike_grad_batch, sf_fisher_cov_batch, sf_local_scan_batch,
// sf_loglike_mean_grad_batch, sf_fisher_mean_batch and the five timing aids).  One description per call, one argument check, one workspace layout
// (carve_applied) and one way to open a call.
#include "sf_stages.h"

struct AppliedCall {
    const char* name;      // the entry point, as its messages start
    const char* required;  // the pointers that must not be NULL, as the message names them
    unsigned parts;        // of the workspace behind the staging area (AppliedParts)
    bool rhs;              // takes right-hand sides (d_rhs, ldr, rhs_stride); false: nothing but the walker's own residual
    bool op;               // takes one of SF_APPLY_*
};
static const AppliedCall APPLY = {"sf_apply_batch", "d_params and d_out", 0, true, true};
static const AppliedCall DECOMPOSE = {"sf_decompose_batch", "d_params and d_comp", AW_YV, true, false};
static const AppliedCall DECOMPOSE_MATVEC = {"sf_debug_decompose_matvec", "d_params and d_comp", AW_YV, false, false};
static const AppliedCall POINTWISE = {"sf_pointwise_batch", "d_params, d_alpha and d_cinv_diag", AW_COV_DIAG | AW_INVERSE, true,
                                      false};
static const AppliedCall GRAD = {"sf_loglike_grad_batch", "d_params, d_lnl and d_grad", AW_INVERSE | AW_PART, false, false};
static const AppliedCall GRAD_CONTRACT = {"sf_debug_loglike_grad_contract", "d_params and d_grad", AW_INVERSE | AW_PART, false,
                                          false};
static const AppliedCall MEAN_GRAD = {"sf_loglike_mean_grad_batch", "d_params, h_slots, d_lnl and d_grad", AW_MEAN, false, false};
static const AppliedCall MEAN_GRAD_CONTRACT = {"sf_debug_loglike_mean_grad_contract", "d_params, h_slots and d_grad", AW_MEAN,
                                               false, false};
static const AppliedCall FISHER = {"sf_fisher_mean_batch", "d_params, h_slots, d_lnl and d_fisher", AW_MEAN | AW_FISHER, false, false};
static const AppliedCall FISHER_COV = {"sf_fisher_cov_batch", "d_params and d_fisher", AW_INVERSE | AW_PART | AW_FISHER_COV, false, false};
static const AppliedCall FISHER_COV_CONTRACT = {"sf_debug_fisher_cov_contract", "d_params and d_fisher",
                                                AW_INVERSE | AW_PART | AW_FISHER_COV, false, false};
static const AppliedCall LOCAL_SCAN = {"sf_local_scan_batch", "d_params, d_cand and d_out", AW_INVERSE | AW_LOCAL_SCAN, false, false};
static const AppliedCall LOCAL_SCAN_CONTRACT = {"sf_debug_local_scan_contract", "d_params, d_cand and d_out",
                                                AW_INVERSE | AW_LOCAL_SCAN, false, false};
// what a call was handed, as far as the check looks at it
struct AppliedArgs {
    int B, nrhs;
    bool required;  // every required pointer is there
    int op = SF_APPLY_CINV;
    const double* d_rhs = nullptr;
    int ldr = 0;
    int64_t rhs_stride = 0;
    int grad_stride = 0;           // (AW_FISHER: the stride of a walker's matrix)
    const int* h_slots = nullptr;  // (AW_MEAN)
    int nslots = 0;
};

// (the staging and export launches take one grid row per right-hand side and one grid plane per walker)
static int counts_ok(const AppliedCall& k, int B, int nrhs) {
    if (B <= 0 || B > 65535 || nrhs < 1 || nrhs > 65535) {
        sf_set_error("%s: B=%d and nrhs=%d must lie in 1 .. 65535", k.name, B, nrhs);
        return SF_EINVAL;
    }
    return SF_OK;
}
// the gradient's own: something to differentiate, and rows that hold it
static int grad_slots_ok(const AppliedCall& k, const sf_model_desc* mdl, int grad_stride) {
    if (!mdl || mdl->n_local < 0 || mdl->n_local > SF_MAX_LOCAL) return SF_OK;  // (model_ok refuses it next)
    const int slots = sf_cov_grad_slots(mdl->has_global, mdl->n_local);
    if (slots == 0) {
        sf_set_error("%s: nothing to differentiate (no global and no local kernel)", k.name);
        return SF_EINVAL;
    }
    if (k.parts & AW_FISHER_COV) {  // (the stride holds a matrix)
        if (grad_stride < slots * slots) {
            sf_set_error("%s: fisher_stride=%d < slots^2 = %d", k.name, grad_stride, slots * slots);
            return SF_EINVAL;
        }
        return SF_OK;
    }
    if (grad_stride < slots) {
        sf_set_error("%s: grad_stride=%d < %d slots", k.name, grad_stride, slots);
        return SF_EINVAL;
    }
    return SF_OK;
}
// the mean gradient's own (behind model_ok): a model it differentiates, and columns that are mean-flux parameters of it
// (shared with the multi-order gradient call: sf_stages.h)
bool mean_counts_ok(const sf_model_desc* mdl, int nslots) {
    return mdl->has_log_scale && !mdl->use_sigma_w && nslots >= 1 && nslots <= SF_MEAN_GRAD_MAX_SLOTS;
}
int mean_slots_ok(const char* who, const sf_ctx* c, const sf_model_desc* mdl, const int* h_slots, int nslots, int grad_stride) {
    if (!mean_counts_ok(mdl, nslots)) {  // (says which)
        if (!mdl->has_log_scale || mdl->use_sigma_w)
            sf_set_error("%s: %s", who, mdl->use_sigma_w ? "use_sigma_w (the paper's form of the emulator term) is not differentiated"
                                                         : "a model without log_scale (the renormalising scale) is not differentiated");
        else sf_set_error("%s: nslots=%d must lie in 1 .. %d", who, nslots, SF_MEAN_GRAD_MAX_SLOTS);
        return SF_EINVAL;
    }
    if (grad_stride < nslots) {
        sf_set_error("%s: grad_stride=%d < %d slots", who, grad_stride, nslots);
        return SF_EINVAL;
    }
    const int off_cheb = 6 + c->P, off_av = off_cheb + mdl->n_cheb + 3 * mdl->n_local;
    for (int j = 0; j < nslots; ++j) {
        const int col = h_slots[j];
        for (int i = 0; i < j; ++i)
            if (h_slots[i] == col) {
                sf_set_error("%s: column %d is listed twice", who, col);
                return SF_EINVAL;
            }
        const bool ok = (col == 0 && mdl->has_vsini) || (col == 1 && mdl->has_vz) || col == 2 || (col >= 6 && col < off_av) ||
                        (col == off_av && mdl->has_av);
        if (ok && !(col >= off_cheb + mdl->n_cheb && col < off_av)) continue;
        sf_set_error("%s: column %d is not a differentiable mean parameter of this model (vsini, vz, log_scale, grid, cheb, Av)",
                     who, col);
        return SF_EINVAL;
    }
    return SF_OK;
}
// The checks that need no context come first: the counts, the required pointers, op and the right-hand-side conventions;
// then the context and the model; then ldr against the order's n.
static int args_ok(const AppliedCall& k, const sf_ctx* c, const sf_model_desc* mdl, const AppliedArgs& a) {
    SF_CHECK(counts_ok(k, a.B, a.nrhs));
    if (!a.required) {
        sf_set_error("%s: %s are required", k.name, k.required);
        return SF_EINVAL;
    }
    if (k.op && (a.op < SF_APPLY_L || a.op > SF_APPLY_CINV)) {
        sf_set_error("%s: op=%d is none of SF_APPLY_*", k.name, a.op);
        return SF_EINVAL;
    }
    if (k.rhs && (a.d_rhs ? a.rhs_stride < 0 : a.nrhs != 1)) {
        sf_set_error("%s: rhs_stride >= 0 with d_rhs, nrhs == 1 without", k.name);
        return SF_EINVAL;
    }
    if (k.parts & AW_PART) SF_CHECK(grad_slots_ok(k, mdl, a.grad_stride));
    SF_CHECK(model_ok(c, mdl));
    // (AW_FISHER: the stride holds a matrix, not a row, and fisher_counts_ok has looked at it)
    const int row_stride = (k.parts & AW_FISHER) ? a.nslots : a.grad_stride;
    if (k.parts & AW_MEAN) SF_CHECK(mean_slots_ok(k.name, c, mdl, a.h_slots, a.nslots, row_stride));
    if (k.rhs && a.d_rhs && a.ldr < c->n) {
        sf_set_error("%s: ldr=%d < n (%d)", k.name, a.ldr, c->n);
        return SF_EINVAL;
    }
    return SF_OK;
}
static size_t workspace_bytes(const AppliedCall& k, const sf_ctx* c, const sf_model_desc* mdl, int B, int nrhs, int nslots = 0) {
    if (counts_ok(k, B, nrhs) || model_ok(c, mdl)) return 0;
    if ((k.parts & AW_PART) && sf_cov_grad_slots(mdl->has_global, mdl->n_local) == 0) return 0;
    return carve_applied(c, mdl, B, nrhs, k.parts, nullptr, 0, carve(c, mdl, B, nullptr, 0, true).bytes, nslots).bytes;
}
// the arguments checked, then the workspace of the call
static int open_applied(const AppliedCall& k, const sf_ctx* c, const sf_model_desc* mdl, const AppliedArgs& a, void* d_work,
                        size_t work_bytes, Work* w, AppliedWork* aw) {
    SF_CHECK(args_ok(k, c, mdl, a));
    SF_CHECK(open_call(c, mdl, a.B, d_work, work_bytes, true, w));
    *aw = carve_applied(c, mdl, a.B, a.nrhs, k.parts, d_work, work_bytes, w->bytes, a.nslots);
    return work_fits(work_bytes, aw->bytes);
}
static int export_status(int* d_info, const AppliedWork& aw, int B, hipStream_t s) {
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, aw.info, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

// transform chain, staging, fill, the likelihood's factorisation and `op` on the staging area, in place.  cov_diag (may be
// NULL): [B][npad], the diagonal of the filled matrices, copied out before the factorisation overwrites it.  xs (may be NULL;
// nrhs = 1 + m, no d_rhs): the transform chain leaves the scaled rows X there and [r, X_1 .. X_m] are the right-hand sides.
// cols (may be NULL; with xs, nrhs = its slots): the right-hand sides are the tangent columns d f / d theta of its slots instead
static int apply_staged(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int op, const double* d_rhs, int nrhs,
                        int ldr, int64_t rhs_stride, double* d_flux, const Work& w, const AppliedWork& aw, hipStream_t s,
                        double* cov_diag = nullptr, double* xs = nullptr, const sf_mean_grad_args* cols = nullptr) {
    const Layout L = layout_of(c);
    int rc;
    {
        ProfScope ps(s, PS_TRANSFORM);
        rc = run_transforms(c, mdl, B, d_params, w, d_flux, xs, nullptr, nullptr, true, s);
        if (rc) return rc;
    }
    // (before the factorisation: the residual rides through it and comes out as L^-1 R)
    if (cols) {  // (behind the transform chain: its broadened rows, multiplier table and FFT scratch are free again)
        SF_CHECK(sf_launch_mean_tangents(broaden_args(c, mdl, B, d_params, w), c->inv_band.as<double>(),
                                         emu_args(c, mdl, d_params, w, w.mu, nullptr, w.Lw, w.info_e), *cols, B, s, false));
        rc = sf_launch_fisher_tangents(eval_args(c, mdl, d_params, w), *cols, aw.stage, (int64_t)nrhs * L.npad, B, s);
    } else
        rc = xs ? sf_launch_mean_stage(w.resid, xs, w.info_e, c->n, L.npad, c->m, B, aw.stage, s)
                : sf_launch_apply_stage(d_rhs, ldr, rhs_stride, w.resid, c->n, L.npad, nrhs, B, aw.stage, s);
    if (rc) return rc;
    const int fp = sf_potrf_front_pad(c->npad, B);  // (once per call: see sf_loglike_batch)
    {
        ProfScope ps(s, PS_FILL);
        rc = sf_launch_fill(loglike_fill_args(c, mdl, d_params, w, L, fp), B, s);
        if (rc) return rc;
    }
    if (cov_diag) SF_CHECK(sf_launch_diag_copy(w.C, L.npad, L.lda, (int64_t)L.npad * L.lda, B, cov_diag, s));
    // the likelihood's factorisation and status, as sf_loglike_batch reports it
    rc = loglike_factor_finish(w, L, fp, B, w.ltbuf, aw.lnl, aw.info, s, &c->exec);
    if (rc) return rc;
    const int64_t sstride = (int64_t)nrhs * L.npad;
    return sf_launch_chol_apply(w.C, L.npad, L.lda, (int64_t)L.npad * L.lda, B, op, aw.stage, nrhs, L.npad, sstride, aw.stage,
                                L.npad, sstride, s);
}
// alpha = C^-1 rhs in the staging area, then the inverse: its diagonal in aw.cinv_diag, X in the matrices.  (The factor is
// applied first: the inverse's launch takes the strict upper triangle of the matrices as scratch.)
static int apply_cinv_and_invert(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_rhs, int nrhs,
                                 int ldr, int64_t rhs_stride, double* d_flux, const Work& w, const AppliedWork& aw, hipStream_t s,
                                 double* cov_diag = nullptr) {
    const Layout L = layout_of(c);
    SF_CHECK(apply_staged(c, mdl, B, d_params, SF_APPLY_CINV, d_rhs, nrhs, ldr, rhs_stride, d_flux, w, aw, s, cov_diag));
    return sf_launch_chol_inverse_diag(w.C, L.npad, L.lda, (int64_t)L.npad * L.lda, B, aw.winv, aw.cinv_diag, L.npad, s);
}

// ----------------------------------------------------------------------------------- the factor applied to right-hand sides
extern "C" size_t sf_apply_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int nrhs) {
    return workspace_bytes(APPLY, c, mdl, B, nrhs);
}
extern "C" int sf_apply_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int op, const double* d_rhs,
                              int nrhs, int ldr, int64_t rhs_stride, double* d_out, double* d_flux, int* d_info, void* d_work,
                              size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(APPLY, c, mdl, {B, nrhs, d_params && d_out, op, d_rhs, ldr, rhs_stride}, d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_staged(c, mdl, B, d_params, op, d_rhs, nrhs, ldr, rhs_stride, d_flux, w, aw, s));
    SF_CHECK(sf_launch_apply_export(aw.stage, aw.info, c->n, c->npad, nrhs, B, d_out, s));
    return export_status(d_info, aw, B, s);
}

// ----------------------------------------------------------------------------------- the residual split by covariance component
extern "C" size_t sf_decompose_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int nrhs) {
    return workspace_bytes(DECOMPOSE, c, mdl, B, nrhs);
}
// K_k v for the v in the staging area, with the Y the transform chain left (the factorisation only reads it)
static int decompose_matvec(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int nrhs, const Work& w,
                            const AppliedWork& aw, double* d_comp, hipStream_t s) {
    return sf_launch_cov_matvec(fill_args(c, mdl, d_params, w), c->m, aw.stage, c->npad, nrhs, B, aw.yv, aw.info, d_comp, s);
}
extern "C" int sf_decompose_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_rhs,
                                  int nrhs, int ldr, int64_t rhs_stride, double* d_comp, double* d_alpha, double* d_flux,
                                  int* d_info, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(DECOMPOSE, c, mdl, {B, nrhs, d_params && d_comp, SF_APPLY_CINV, d_rhs, ldr, rhs_stride}, d_work,
                          work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_staged(c, mdl, B, d_params, SF_APPLY_CINV, d_rhs, nrhs, ldr, rhs_stride, d_flux, w, aw, s));
    SF_CHECK(decompose_matvec(c, mdl, B, d_params, nrhs, w, aw, d_comp, s));
    if (d_alpha) SF_CHECK(sf_launch_apply_export(aw.stage, aw.info, c->n, c->npad, nrhs, B, d_alpha, s));
    return export_status(d_info, aw, B, s);
}
// The last step of sf_decompose_batch alone, on the workspace a call with the same ctx, model, B, nrhs and d_params left
// (tools/bench_decompose.py times it)
extern "C" int sf_debug_decompose_matvec(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int nrhs,
                                         double* d_comp, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(DECOMPOSE_MATVEC, c, mdl, {B, nrhs, d_params && d_comp}, d_work, work_bytes, &w, &aw));
    return decompose_matvec(c, mdl, B, d_params, nrhs, w, aw, d_comp, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------- per-pixel leave-one-out diagnostics
extern "C" size_t sf_pointwise_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int nrhs) {
    return workspace_bytes(POINTWISE, c, mdl, B, nrhs);
}
extern "C" int sf_pointwise_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_rhs,
                                  int nrhs, int ldr, int64_t rhs_stride, double* d_alpha, double* d_cinv_diag,
                                  double* d_cov_diag, double* d_flux, int* d_info, void* d_work, size_t work_bytes,
                                  void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(POINTWISE, c, mdl, {B, nrhs, d_params && d_alpha && d_cinv_diag, SF_APPLY_CINV, d_rhs, ldr, rhs_stride},
                          d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_cinv_and_invert(c, mdl, B, d_params, d_rhs, nrhs, ldr, rhs_stride, d_flux, w, aw, s,
                                   d_cov_diag ? aw.cov_diag : nullptr));
    SF_CHECK(sf_launch_apply_export(aw.stage, aw.info, c->n, c->npad, nrhs, B, d_alpha, s));
    SF_CHECK(sf_launch_apply_export(aw.cinv_diag, aw.info, c->n, c->npad, 1, B, d_cinv_diag, s));
    if (d_cov_diag) SF_CHECK(sf_launch_apply_export(aw.cov_diag, aw.info, c->n, c->npad, 1, B, d_cov_diag, s));
    return export_status(d_info, aw, B, s);
}

// ----------------------------------------------------------------------------------- gradient in the covariance hyper-parameters
extern "C" size_t sf_loglike_grad_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B) {
    return workspace_bytes(GRAD, c, mdl, B, 1);
}
// 1/2 sum (alpha alpha^T - C^-1) o dC/dtheta from the alpha in the staging area and the X the inverse's launch left in the matrices
static int grad_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w, const AppliedWork& aw,
                         double* d_grad, int grad_stride, hipStream_t s) {
    sf_fill_args f = fill_args(c, mdl, d_params, w);
    f.C = w.C, f.lda = w.L.lda, f.stride = (int64_t)w.L.npad * w.L.lda, f.lower_only = 1, f.add_jitter = 1;
    return sf_launch_cov_grad(f, B, aw.winv, aw.stage, w.L.npad, aw.info, aw.part, d_grad, grad_stride, s);
}
static AppliedArgs grad_args(int B, bool required, int grad_stride) {
    AppliedArgs a = {B, 1, required};
    a.grad_stride = grad_stride;
    return a;
}
extern "C" int sf_loglike_grad_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, double* d_lnl,
                                     double* d_grad, int grad_stride, double* d_flux, int* d_info, void* d_work,
                                     size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(GRAD, c, mdl, grad_args(B, d_params && d_lnl && d_grad, grad_stride), d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_cinv_and_invert(c, mdl, B, d_params, nullptr, 1, c->n, 0, d_flux, w, aw, s));
    SF_CHECK(grad_contract(c, mdl, B, d_params, w, aw, d_grad, grad_stride, s));
    SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return export_status(d_info, aw, B, s);
}
// The contraction launches of sf_loglike_grad_batch alone, on the workspace a call with the same ctx, model, B and d_params
// left (tools/bench_gradient.py times them)
extern "C" int sf_debug_loglike_grad_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, double* d_grad,
                                              int grad_stride, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(GRAD_CONTRACT, c, mdl, grad_args(B, d_params && d_grad, grad_stride), d_work, work_bytes, &w, &aw));
    return grad_contract(c, mdl, B, d_params, w, aw, d_grad, grad_stride, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------- Fisher information in the covariance hyper-parameters
extern "C" size_t sf_fisher_cov_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B) {
    return workspace_bytes(FISHER_COV, c, mdl, B, 1);
}
// all of W = C^-1 from the X the inverse's launch left in the matrices, then per slot T_j = W dC_j and 1/2 sum dC_i o (T_j W)
static int fisher_cov_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w, const AppliedWork& aw,
                               double* d_fisher, int fisher_stride, hipStream_t s) {
    sf_fill_args f = fill_args(c, mdl, d_params, w);
    f.C = w.C, f.lda = w.L.lda, f.stride = (int64_t)w.L.npad * w.L.lda, f.lower_only = 1, f.add_jitter = 1;
    return sf_launch_fisher_cov(f, B, aw.winv, aw.info, aw.wfull, aw.tj, aw.part, d_fisher, fisher_stride, s);
}
extern "C" int sf_fisher_cov_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, double* d_lnl, double* d_fisher,
                                   int fisher_stride, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(FISHER_COV, c, mdl, grad_args(B, d_params && d_fisher, fisher_stride), d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_cinv_and_invert(c, mdl, B, d_params, nullptr, 1, c->n, 0, nullptr, w, aw, s));
    SF_CHECK(fisher_cov_contract(c, mdl, B, d_params, w, aw, d_fisher, fisher_stride, s));
    if (d_lnl) SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return export_status(d_info, aw, B, s);
}
// The launches of sf_fisher_cov_batch behind the inverse alone, on the workspace a call with the same ctx, model, B and d_params
// left (tools/bench_cov_fisher.py times them)
extern "C" int sf_debug_fisher_cov_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, double* d_fisher,
                                            int fisher_stride, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(FISHER_COV_CONTRACT, c, mdl, grad_args(B, d_params && d_fisher, fisher_stride), d_work, work_bytes, &w, &aw));
    return fisher_cov_contract(c, mdl, B, d_params, w, aw, d_fisher, fisher_stride, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------- score scan for a new local kernel
// the call's own refusals, before the context is looked at: the counts (with the candidates named) and the required pointers
static int local_scan_counts_ok(const AppliedCall& k, int B, int ncand, bool required) {
    if (B <= 0 || B > 65535 || ncand < 1 || ncand > 65535) {
        sf_set_error("%s: B=%d and ncand=%d must lie in 1 .. 65535", k.name, B, ncand);
        return SF_EINVAL;
    }
    if (!required) {
        sf_set_error("%s: %s are required", k.name, k.required);
        return SF_EINVAL;
    }
    return SF_OK;
}
// behind model_ok: the patch of a candidate is contiguous on a sorted grid only
static int local_scan_grid_ok(const AppliedCall& k, const sf_ctx* c) {
    if (!c->monotonic) {
        sf_set_error("%s: the wavelength grid is not monotonic (a candidate's pixels are no contiguous patch)", k.name);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_local_scan_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int ncand) {
    if (ncand < 1 || ncand > 65535 || counts_ok(LOCAL_SCAN, B, 1) || model_ok(c, mdl) || !c->monotonic) return 0;
    return workspace_bytes(LOCAL_SCAN, c, mdl, B, 1, ncand);
}
// the band of W = C^-1 from the X the inverse's launch left in the matrices, the candidates' patches, then per (walker,
// candidate) the three contractions with the alpha in the staging area
static int local_scan_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_cand, int ncand,
                               const Work& w, const AppliedWork& aw, double* d_out, hipStream_t s) {
    sf_fill_args f = fill_args(c, mdl, d_params, w);
    f.C = w.C, f.lda = w.L.lda, f.stride = (int64_t)w.L.npad * w.L.lda, f.lower_only = 1, f.add_jitter = 1;
    return sf_launch_local_scan(f, B, aw.winv, aw.stage, w.L.npad, aw.info, d_cand, ncand, aw.patch, aw.wband, d_out, s);
}
static int open_local_scan(const AppliedCall& k, const sf_ctx* c, const sf_model_desc* mdl, int B, int ncand, bool required,
                           void* d_work, size_t work_bytes, Work* w, AppliedWork* aw) {
    SF_CHECK(local_scan_counts_ok(k, B, ncand, required));
    SF_CHECK(model_ok(c, mdl));
    SF_CHECK(local_scan_grid_ok(k, c));
    const size_t need = workspace_bytes(LOCAL_SCAN, c, mdl, B, 1, ncand);
    if (!d_work || work_bytes < need) {  // (said here, so that the message names the call)
        sf_set_error("%s: workspace too small: have %zu, need %zu", k.name, d_work ? work_bytes : (size_t)0, need);
        return SF_ENOMEM;
    }
    AppliedArgs a = {B, 1, true};
    a.nslots = ncand;
    return open_applied(k, c, mdl, a, d_work, work_bytes, w, aw);
}
extern "C" int sf_local_scan_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_cand, int ncand,
                                   double* d_out, double* d_lnl, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_local_scan(LOCAL_SCAN, c, mdl, B, ncand, d_params && d_cand && d_out, d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_cinv_and_invert(c, mdl, B, d_params, nullptr, 1, c->n, 0, nullptr, w, aw, s));
    SF_CHECK(local_scan_contract(c, mdl, B, d_params, d_cand, ncand, w, aw, d_out, s));
    if (d_lnl) SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return export_status(d_info, aw, B, s);
}
// The launches of sf_local_scan_batch behind the inverse alone, on the workspace a call with the same ctx, model, B, d_params
// and ncand left (tools/bench_local_scan.py times them)
extern "C" int sf_debug_local_scan_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_cand,
                                            int ncand, double* d_out, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_local_scan(LOCAL_SCAN_CONTRACT, c, mdl, B, ncand, d_params && d_cand && d_out, d_work, work_bytes, &w, &aw));
    return local_scan_contract(c, mdl, B, d_params, d_cand, ncand, w, aw, d_out, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------- gradient in the mean-flux parameters
extern "C" size_t sf_loglike_mean_grad_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int nslots) {
    if (model_ok(c, mdl) || nslots < 1 || nslots > SF_MEAN_GRAD_MAX_SLOTS) return 0;
    return workspace_bytes(MEAN_GRAD, c, mdl, B, 1 + c->m, nslots);
}
sf_mean_grad_args mean_grad_kernel_args(const sf_ctx* c, const int* h_slots, int nslots, const Work& w, const AppliedWork& aw,
                                        double* d_grad, int grad_stride) {
    sf_mean_grad_args a;
    a.stage = aw.stage, a.Xs = aw.xs, a.Lw = w.Lw, a.mu = w.mu, a.scale = w.scale, a.info = aw.info;
    a.fin = aw.fin, a.part = aw.mpart, a.grad = d_grad;
    a.dcoef = aw.dcoef, a.kdot = aw.kdot, a.mudot = aw.mudot, a.zdot = aw.zdot;
    a.n = c->n, a.npad = w.L.npad, a.m = c->m, a.nslots = nslots, a.grad_stride = grad_stride;
    a.want_vz = a.want_vsini = a.ng = 0;
    for (int j = 0; j < SF_MEAN_GRAD_MAX_SLOTS; ++j) {
        a.slots[j] = j < nslots ? h_slots[j] : -1;
        a.gcols[j] = -1;
        if (a.slots[j] == 0) a.want_vsini = 1;
        if (a.slots[j] == 1) a.want_vz = 1;
        if (a.slots[j] >= 6 && a.slots[j] < 6 + c->P) a.gcols[a.ng++] = a.slots[j];
    }
    return a;
}
// the moments, the pixel pass, the grid slots and the sum over the blocks, from alpha and V = C^-1 X^T in the staging area
static int mean_grad_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const int* h_slots, int nslots,
                              const Work& w, const AppliedWork& aw, double* d_grad, int grad_stride, hipStream_t s) {
    return sf_launch_mean_grad(eval_args(c, mdl, d_params, w), mean_grad_kernel_args(c, h_slots, nslots, w, aw, d_grad, grad_stride),
                               w.zs, c->m * c->M, B, s);
}
static AppliedArgs mean_grad_args(const sf_ctx* c, int B, bool required, const int* h_slots, int nslots, int grad_stride) {
    AppliedArgs a = {B, c ? 1 + c->m : 1, required};
    a.grad_stride = grad_stride, a.h_slots = h_slots, a.nslots = nslots;
    return a;
}
extern "C" int sf_loglike_mean_grad_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const int* h_slots,
                                          int nslots, double* d_lnl, double* d_grad, int grad_stride, double* d_flux, int* d_info,
                                          void* d_work, size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(MEAN_GRAD, c, mdl, mean_grad_args(c, B, d_params && h_slots && d_lnl && d_grad, h_slots, nslots, grad_stride),
                          d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(apply_staged(c, mdl, B, d_params, SF_APPLY_CINV, nullptr, 1 + c->m, c->n, 0, d_flux, w, aw, s, nullptr, aw.xs));
    // (behind the transform chain: its broadened rows, multiplier table and FFT scratch are free again)
    SF_CHECK(sf_launch_mean_tangents(broaden_args(c, mdl, B, d_params, w), c->inv_band.as<double>(),
                                     emu_args(c, mdl, d_params, w, w.mu, nullptr, w.Lw, w.info_e),
                                     mean_grad_kernel_args(c, h_slots, nslots, w, aw, d_grad, grad_stride), B, s));
    SF_CHECK(mean_grad_contract(c, mdl, B, d_params, h_slots, nslots, w, aw, d_grad, grad_stride, s));
    SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return export_status(d_info, aw, B, s);
}
// The launches of sf_loglike_mean_grad_batch behind the solve alone, on the workspace a call with the same ctx, model, B,
// d_params and slots left (tools/bench_mean_gradient.py times them)
extern "C" int sf_debug_loglike_mean_grad_contract(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                                   const int* h_slots, int nslots, double* d_grad, int grad_stride, void* d_work,
                                                   size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(open_applied(MEAN_GRAD_CONTRACT, c, mdl, mean_grad_args(c, B, d_params && h_slots && d_grad, h_slots, nslots, grad_stride),
                          d_work, work_bytes, &w, &aw));
    return mean_grad_contract(c, mdl, B, d_params, h_slots, nslots, w, aw, d_grad, grad_stride, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------- Fisher information in the mean-flux parameters
// what both Fisher calls refuse before they look at the context (shared with sf_banded.cpp: sf_stages.h)
int fisher_counts_ok(const char* who, bool required, int nslots, int fisher_stride) {
    if (!required) {
        sf_set_error("%s: d_params, h_slots, d_lnl, d_fisher and d_work are required", who);
        return SF_EINVAL;
    }
    if (nslots < 1 || nslots > SF_MEAN_GRAD_MAX_SLOTS) {
        sf_set_error("%s: nslots=%d must lie in 1 .. %d", who, nslots, SF_MEAN_GRAD_MAX_SLOTS);
        return SF_EINVAL;
    }
    if (fisher_stride < nslots * nslots) {
        sf_set_error("%s: fisher_stride=%d < nslots^2 = %d", who, fisher_stride, nslots * nslots);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_fisher_mean_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int nslots) {
    if (model_ok(c, mdl) || !mean_counts_ok(mdl, nslots)) return 0;
    return workspace_bytes(FISHER, c, mdl, B, nslots, nslots);
}
// The likelihood's sequence with the tangent columns J as right-hand sides, Z = L^-1 J in the staging area, F = Z^T Z
extern "C" int sf_fisher_mean_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const int* h_slots, int nslots,
                                    double* d_lnl, double* d_fisher, int fisher_stride, int* d_info, void* d_work,
                                    size_t work_bytes, void* stream) {
    Work w;
    AppliedWork aw;
    SF_CHECK(fisher_counts_ok(FISHER.name, d_params && h_slots && d_lnl && d_fisher && d_work, nslots, fisher_stride));
    AppliedArgs a = {B, nslots, true};
    a.grad_stride = fisher_stride, a.h_slots = h_slots, a.nslots = nslots;
    SF_CHECK(open_applied(FISHER, c, mdl, a, d_work, work_bytes, &w, &aw));
    hipStream_t s = (hipStream_t)stream;
    sf_mean_grad_args cols = mean_grad_kernel_args(c, h_slots, nslots, w, aw, nullptr, 0);
    cols.info = w.info_e;  // (the columns are staged before the factorisation: the transform chain's status)
    SF_CHECK(apply_staged(c, mdl, B, d_params, SF_APPLY_LINV, nullptr, nslots, c->n, 0, nullptr, w, aw, s, nullptr, aw.xs, &cols));
    SF_CHECK(sf_launch_fisher_ztz(aw.stage, c->n, c->npad, nslots, B, aw.info, aw.fpart, d_fisher, fisher_stride, s));
    SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return export_status(d_info, aw, B, s);
}
