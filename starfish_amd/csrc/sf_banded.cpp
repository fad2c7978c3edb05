// C-ABI host layer: the structure-exploiting (banded + low-rank) solver.
#include "sf_stages.h"

extern "C" int sf_banded_max_halfwidth(const sf_ctx* c) {
    if (!c || !c->n) return SF_EINVAL;
    if (!c->monotonic) return -1;
    const bool tiles = sfb_admit(SF_BAND_TILES_MAX_HALFWIDTH, c->m + 1) == SFB_TILES;  // (beyond what the window takes)
    return tiles ? SF_BAND_TILES_MAX_HALFWIDTH : sf_band_max_halfwidth(c->m + 1);
}
extern "C" int sf_banded_window_halfwidth(const sf_ctx* c) {
    if (!c || !c->n) return SF_EINVAL;
    return c->monotonic ? sf_band_max_halfwidth(c->m + 1) : -1;
}
extern "C" size_t sf_banded_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth) {
    if (model_ok(c, mdl) || B <= 0 || halfwidth < 0) return 0;
    const size_t base = carve(c, mdl, B, nullptr, 0, false).bytes;
    return carve_band(c, B, halfwidth, nullptr, 0, base).bytes;
}
// One call of the band solver (sf_band_call): the band view, the order and the batch, the right-hand sides, the outputs
static sf_band_call band_call(const double* band, int64_t sband, int ldb, int halfwidth, int n, int batch, const sf_band_rhs& r,
                              double* logdet, double* gram, int* info) {
    sf_band_call k = {};
    k.band = band, k.sband = sband, k.ldb = ldb, k.halfwidth = halfwidth;
    k.n = n, k.batch = batch;
    k.r = r;
    k.logdet = logdet, k.gram = gram, k.info = info;
    return k;
}
// What the calls that share the likelihood's head differ in, beyond the layout (tiles or window) that the BandWork says
// Caller right-hand sides R in place of the walker's own residual (sf_diagnose_banded_batch): the sweep then runs over the k + m
// rows [R; Y] staged in buf, its Gram matrix goes to gram, and the capacitance step is left to the mix (sf_launch_band_mix with
// flag): there is no squared distance, lnl is -logdet(Bd) / 2 (not a likelihood) and info what fill, emulator and sweep reported
struct BandHeadRhs {
    const double* d_rhs;
    int k, ldr;
    int64_t rhs_stride;
    double *buf, *gram, *zero;  // (carve_band_diag: rhs, gram, zero)
};
// The tangent columns J = d f / d theta behind the walker's own rows (sf_fisher_banded_mean_batch): the sweep -- not a keeping
// one -- runs over the 1 + m + p rows [r; Y; J] staged in buf, its Gram matrix goes to gram and its leading (1 + m)^2 block to
// the capacitance step as ever; behind the status, F = G_JJ - U^T U
struct BandHeadFisher {
    const int* h_slots;
    int nslots;
    const AppliedWork* aw;                    // xs and the tangents' buffers
    double *buf, *gram, *twist;               // (carve_band_fisher: aw.stage, gram, twist)
    double* d_fisher;
    int fisher_stride;
};
struct BandHead {
    double* fac;                              // the sweep keeps its factor here (window only); NULL: it keeps nothing
    double *d_X, *d_resid, *d_log_scale;      // optional outputs of run_transforms
    double* lnl;                              // where sf_launch_finish leaves lnl / info
    int* info;
    double* d_flux = nullptr;                 // one more of them
    const BandHeadRhs* rhs = nullptr;         // NULL: the walker's own residual, [r; Y]
    bool per_entry_fill = false;              // true: every entry of the band from its own pixel pair, no table per diagonal
    const BandHeadFisher* fisher = nullptr;   // NULL: no columns behind [r; Y]
};
// The head of the likelihood on the band solver: band fill, transforms, sweep, capacitance step, lnl / info.
// The band fill depends on the covariance hyper-parameters only, the transforms on the stellar ones: the two run side by
// side (fill on a library-owned auxiliary stream, joined before the sweep).
static int banded_head(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth, const Work& w,
                       const BandWork& bw, const BandHead& h, hipStream_t s) {
    if (use_device(c)) return SF_EHIP;
    prof_count_call();
    sf_exec* aux = &c->exec;
    SF_CHECK(sf_exec_prepare(aux));
    hipStream_t sf = aux->aux;
    if (sf != s) {
        SF_HIP(hipEventRecord(aux->fork, s));
        SF_HIP(hipStreamWaitEvent(sf, aux->fork, 0));
    }
    const int n16 = (c->n + 15) / 16 * 16;  // (the window's band is filled with identity rows up to whole blocks)
    const int64_t sband = (int64_t)c->npad * bw.ldb;
    {
        ProfScope ps(sf, PS_FILL);
        SF_HIP(hipMemsetAsync(w.info_c, 0, sizeof(int) * (size_t)B, sf));
        sf_fill_args f = fill_args(c, mdl, d_params, w);
        f.C = nullptr;
        f.lda = 0;
        f.stride = 0;
        f.lower_only = 1;
        f.add_jitter = 1;
        f.npad = bw.tiles ? c->npad : n16;
        if (bw.tiles) {  // straight into the 128 x 128 tiles of the bordered band matrix
            static const bool poison = SF_TUNE_FLAG("SF_BAND_TILES_POISON");  // test aid: NaN wherever a tile is read before it is written
            if (poison) SF_HIP(hipMemsetAsync(bw.tiles, 0xff, sizeof(double) * sf_band_tiles_doubles(c->npad, B), sf));
            const int lda_t = sf_band_tiles_lda(c->npad);
            SF_CHECK(sf_launch_band_fill(f, B, bw.tiles, bw.ldb, halfwidth, lda_t, (int64_t)(c->npad + 64) * lda_t, w.info_c, bw.gtab, sf,
                                         sf_band_tiles_wt(halfwidth)));
        } else
            SF_CHECK(sf_launch_band_fill(f, B, bw.band, halfwidth + 1, halfwidth, bw.ldb, sband, w.info_c,
                                         h.per_entry_fill ? nullptr : bw.gtab, sf));
    }
    if (sf != s) SF_HIP(hipEventRecord(aux->join, sf));
    {
        ProfScope ps(s, PS_TRANSFORM);
        SF_CHECK(run_transforms(c, mdl, B, d_params, w, h.d_flux, h.d_X, h.d_resid, h.d_log_scale, true, s));
    }
    sf_band_rhs rhs = {w.Y, (int64_t)c->mpad * c->npad, c->npad, c->m + 1, w.resid, c->npad};
    if (h.rhs) {
        const BandHeadRhs& r = *h.rhs;
        SF_CHECK(sf_launch_band_diag_stage(r.d_rhs, r.ldr, r.rhs_stride, w.Y, (int64_t)c->mpad * c->npad, c->n, c->npad, r.k, c->m, B,
                                           r.buf, s));
        SF_HIP(hipMemsetAsync(r.zero, 0, sizeof(double) * (size_t)B, s));
        rhs = sf_band_rhs{r.buf, (int64_t)(r.k + c->m) * c->npad, c->npad, r.k + c->m, nullptr, 0};
    }
    const int nin = h.fisher ? 1 + c->m + h.fisher->nslots : 0;
    if (h.fisher) {
        const BandHeadFisher& f = *h.fisher;
        sf_mean_grad_args cols = mean_grad_kernel_args(c, f.h_slots, f.nslots, w, *f.aw, nullptr, 0);
        cols.info = w.info_e;  // (before the sweep: the transform chain's status)
        // (behind the transform chain: its broadened rows, multiplier table and FFT scratch are free again)
        SF_CHECK(sf_launch_mean_tangents(broaden_args(c, mdl, B, d_params, w), c->inv_band.as<double>(),
                                         emu_args(c, mdl, d_params, w, w.mu, nullptr, w.Lw, w.info_e), cols, B, s, false));
        SF_CHECK(sf_launch_fisher_rows(w.resid, w.Y, (int64_t)c->mpad * c->npad, c->n, c->npad, c->m, nin, B, f.buf, s));
        SF_CHECK(sf_launch_fisher_tangents(eval_args(c, mdl, d_params, w), cols, f.buf + (int64_t)(1 + c->m) * c->npad,
                                           (int64_t)nin * c->npad, B, s));
        rhs = sf_band_rhs{f.buf, (int64_t)nin * c->npad, c->npad, nin, nullptr, 0};
    }
    if (sf != s) SF_HIP(hipStreamWaitEvent(s, aux->join, 0));
    {
        ProfScope ps(s, PS_POTRF);
        const sf_band_call k = band_call(bw.band, sband, bw.ldb, halfwidth, bw.tiles ? c->n : n16, B, rhs, bw.logdet_band,
                                         h.rhs ? h.rhs->gram : h.fisher ? h.fisher->gram : bw.gram, w.info_c);
        if (bw.tiles) SF_CHECK(sf_launch_potrf_band(k, c->npad, bw.tiles, s));
        else if (h.fac) SF_CHECK(sf_launch_band_keep(k, h.fac, s));
        else if (sf_band_twisted_applicable(k.n, halfwidth, B))
            SF_CHECK(sf_launch_band_forms_twisted(k, h.fisher ? h.fisher->twist : bw.twist, s));
        else SF_CHECK(sf_launch_band_forms(k, s));
    }
    {
        ProfScope ps(s, PS_SOLVE);
        if (h.rhs) return sf_launch_finish(B, bw.logdet_band, h.rhs->zero, w.info_e, w.info_c, h.lnl, h.info, s);
        if (h.fisher) SF_CHECK(sf_launch_fisher_lead(h.fisher->gram, nin, c->m + 1, B, bw.gram, s));
        SF_CHECK(sf_launch_woodbury(bw.gram, c->m + 1, B, bw.logdet_band, w.logdet, w.sqmah, w.info_c, s));
        SF_CHECK(sf_launch_finish(B, w.logdet, w.sqmah, w.info_e, w.info_c, h.lnl, h.info, s));
        if (h.fisher)
            SF_CHECK(sf_launch_fisher_band(h.fisher->gram, c->m, h.fisher->nslots, B, h.info, h.fisher->d_fisher,
                                           h.fisher->fisher_stride, s));
    }
    return SF_OK;
}
extern "C" int sf_loglike_banded_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                       double* d_lnl, double* d_logdet, double* d_sqmah, double* d_resid, double* d_log_scale,
                                       int* d_info, void* d_work, size_t work_bytes, void* stream) {
    if (model_ok(c, mdl)) return SF_EINVAL;
    if (B <= 0 || !d_work || !d_lnl) {
        sf_set_error("sf_loglike_banded_batch: bad batch size / workspace / d_lnl");
        return SF_EINVAL;
    }
    const int wmax = sf_banded_max_halfwidth(c);
    if (halfwidth < 0 || halfwidth > wmax) {
        sf_set_error("sf_loglike_banded_batch: half-width %d outside [0, %d] (use sf_loglike_batch)", halfwidth, wmax);
        return SF_EINVAL;
    }
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandWork bw = carve_band(c, B, halfwidth, d_work, work_bytes, w.bytes);
    SF_CHECK(work_fits(work_bytes, bw.bytes));
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(banded_head(c, mdl, B, d_params, halfwidth, w, bw, BandHead{nullptr, nullptr, d_resid, d_log_scale, d_lnl, d_info}, s));
    return export_logdet_sqmah(d_logdet, d_sqmah, w, B, s);
}

extern "C" int sf_band_logdet_gram_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride,
                                         int batch, const double* d_rhs, int nrhs, int ldr, int64_t rhs_stride,
                                         double* d_logdet, double* d_gram, int* d_info, void* stream) {
    if (!d_band || !d_rhs || !d_logdet || !d_gram || !d_info) {
        sf_set_error("sf_band_logdet_gram_batch: null pointer");
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    SF_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * (size_t)batch, s));
    return sf_launch_band_forms(band_call(d_band, stride, ldb, halfwidth, n, batch, sf_band_rhs{d_rhs, rhs_stride, ldr, nrhs, nullptr, 0},
                                          d_logdet, d_gram, d_info), s);
}

// what sf_band_solve_batch refuses before it touches the device; who == NULL: silently (the size query)
static int band_solve_shape_ok(const char* who, int n, int halfwidth, int batch, int nrhs);
// The same sweep with its form chosen by the caller (the stage tests): 0 = one sweep per matrix, what sf_band_logdet_gram_batch
// runs; 1 = two half sweeps, merge and separator; -1 = what the likelihood's head would run for this order, half-width and batch
static const char* const DEBUG_FORMS = "sf_debug_band_forms_batch";
static int debug_band_forms_ok(bool say, int n, int halfwidth, int batch, int nrhs, int form) {
    if (form < -1 || form > 1) {
        if (say) sf_set_error("%s: form=%d must be 0 (single sweep), 1 (two half sweeps) or -1 (the likelihood's choice)", DEBUG_FORMS, form);
        return SF_EINVAL;
    }
    SF_CHECK(band_solve_shape_ok(say ? DEBUG_FORMS : nullptr, n, halfwidth, batch, nrhs));
    if (form == 1 && (n % BB || !sfb_twist_fits(n / BB, sfb_nbr(halfwidth)))) {
        if (say)
            sf_set_error("%s: two half sweeps need whole 16-row blocks and at least %d of them at half-width %d (n=%d)", DEBUG_FORMS,
                         3 * sfb_nbr(halfwidth) - 1, halfwidth, n);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_debug_band_forms_workspace_bytes(int n, int halfwidth, int batch, int nrhs, int form) {
    if (debug_band_forms_ok(false, n, halfwidth, batch, nrhs, form) || form == 0) return 0;
    return sizeof(double) * sfb_twist_carve(nullptr, halfwidth, nrhs, batch).doubles;
}
extern "C" int sf_debug_band_forms_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride, int batch,
                                         const double* d_rhs, int nrhs, int ldr, int64_t rhs_stride, double* d_logdet, double* d_gram,
                                         int* d_info, int form, void* d_work, size_t work_bytes, void* stream) {
    if (!d_band || !d_rhs || !d_logdet || !d_gram || !d_info || (form != 0 && !d_work)) {
        sf_set_error("%s: null pointer", DEBUG_FORMS);
        return SF_EINVAL;
    }
    SF_CHECK(debug_band_forms_ok(true, n, halfwidth, batch, nrhs, form));
    if (ldb < halfwidth + 1 || ldr < n) {
        sf_set_error("%s: ldb=%d < halfwidth + 1, or ldr=%d < n (%d)", DEBUG_FORMS, ldb, ldr, n);
        return SF_EINVAL;
    }
    SF_CHECK(work_fits(work_bytes, sf_debug_band_forms_workspace_bytes(n, halfwidth, batch, nrhs, form)));
    hipStream_t s = (hipStream_t)stream;
    SF_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * (size_t)batch, s));
    const sf_band_call k = band_call(d_band, stride, ldb, halfwidth, n, batch, sf_band_rhs{d_rhs, rhs_stride, ldr, nrhs, nullptr, 0},
                                     d_logdet, d_gram, d_info);
    if (form == 1 || (form == -1 && sf_band_twisted_applicable(n, halfwidth, batch)))
        return sf_launch_band_forms_twisted(k, (double*)d_work, s);
    return sf_launch_band_forms(k, s);
}

// ----------------------------------------------------------------------------------- the full banded solve
static int band_solve_shape_ok(const char* who, int n, int halfwidth, int batch, int nrhs) {
    if (n <= 0 || batch <= 0 || halfwidth < 0 || nrhs < 1 || nrhs > 48) {
        if (who) sf_set_error("%s: n=%d, batch=%d must be positive, halfwidth=%d >= 0, nrhs=%d in 1 .. 48", who, n, batch, halfwidth, nrhs);
        return SF_EINVAL;
    }
    if (sfb_admit(halfwidth, nrhs) != SFB_WINDOW) {
        if (who)
            sf_set_error("%s: half-width %d with %d right-hand sides exceeds the LDS window (max %d)", who, halfwidth, nrhs,
                         sf_band_max_halfwidth(nrhs));
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_band_solve_workspace_bytes(int n, int halfwidth, int batch, int nrhs) {
    if (band_solve_shape_ok(nullptr, n, halfwidth, batch, nrhs)) return 0;
    return carve_band_solve(n, halfwidth, batch, nrhs, nullptr, 0).bytes;
}
extern "C" int sf_band_solve_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride, int batch,
                                   const double* d_rhs, int nrhs, int ldr, int64_t rhs_stride, double* d_x, int ldx,
                                   int64_t x_stride, double* d_logdet, double* d_gram, int* d_info, void* d_work, size_t work_bytes,
                                   void* stream) {
    if (!d_band || !d_rhs || !d_x || !d_logdet || !d_info || !d_work) {
        sf_set_error("sf_band_solve_batch: null pointer");
        return SF_EINVAL;
    }
    SF_CHECK(band_solve_shape_ok("sf_band_solve_batch", n, halfwidth, batch, nrhs));
    if (ldb < halfwidth + 1 || ldr < n || ldx < n) {
        sf_set_error("sf_band_solve_batch: ldb=%d < halfwidth + 1, or ldr=%d / ldx=%d < n (%d)", ldb, ldr, ldx, n);
        return SF_EINVAL;
    }
    const BandSolveWork bs = carve_band_solve(n, halfwidth, batch, nrhs, d_work, work_bytes);
    SF_CHECK(work_fits(work_bytes, bs.bytes));
    hipStream_t s = (hipStream_t)stream;
    SF_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * (size_t)batch, s));
    const sf_band_call k = band_call(d_band, stride, ldb, halfwidth, n, batch, sf_band_rhs{d_rhs, rhs_stride, ldr, nrhs, nullptr, 0},
                                     d_logdet, d_gram ? d_gram : bs.gram, d_info);
    SF_CHECK(sf_launch_band_keep(k, bs.fac, s));
    return sf_launch_band_back(bs.fac, n, halfwidth, batch, nrhs, d_info, d_x, ldx, x_stride, s);
}

// ----------------------------------------------------------------------------------- the stand-alone selected inversion
static int band_selinv_shape_ok(const char* who, int n, int halfwidth, int batch) {
    if (n <= 0 || batch <= 0 || halfwidth < 0) {
        if (who) sf_set_error("%s: n=%d, batch=%d must be positive, halfwidth=%d >= 0", who, n, batch, halfwidth);
        return SF_EINVAL;
    }
    if (!sfb_selinv_admits(halfwidth)) {
        if (who) sf_set_error("%s: half-width %d exceeds the LDS window (max %d)", who, halfwidth, sf_band_max_halfwidth(1));
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_band_selinv_workspace_bytes(int n, int halfwidth, int batch) {
    if (band_selinv_shape_ok(nullptr, n, halfwidth, batch)) return 0;
    return carve_band_selinv(n, halfwidth, batch, nullptr, 0).bytes;
}
extern "C" int sf_band_selinv_batch(const double* d_band, int n, int halfwidth, int ldb, int64_t stride, int batch, double* d_out, int ldo,
                                    int64_t out_stride, double* d_logdet, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    if (!d_band || !d_out || !d_logdet || !d_info || !d_work) {
        sf_set_error("sf_band_selinv_batch: null pointer");
        return SF_EINVAL;
    }
    SF_CHECK(band_selinv_shape_ok("sf_band_selinv_batch", n, halfwidth, batch));
    if (ldb < halfwidth + 1 || ldo < halfwidth + 1) {
        sf_set_error("sf_band_selinv_batch: ldb=%d or ldo=%d < halfwidth + 1 (%d)", ldb, ldo, halfwidth + 1);
        return SF_EINVAL;
    }
    const BandSelinvWork bs = carve_band_selinv(n, halfwidth, batch, d_work, work_bytes);
    SF_CHECK(work_fits(work_bytes, bs.bytes));
    hipStream_t s = (hipStream_t)stream;
    SF_HIP(hipMemsetAsync(d_info, 0, sizeof(int) * (size_t)batch, s));
    SF_HIP(hipMemsetAsync(bs.zero, 0, sizeof(double) * (size_t)n, s));  // the sweep's one right-hand side, shared by the batch
    const sf_band_call k = band_call(d_band, stride, ldb, halfwidth, n, batch, sf_band_rhs{bs.zero, 0, n, 1, nullptr, 0}, d_logdet,
                                     bs.gram, d_info);
    SF_CHECK(sf_launch_band_keep(k, bs.fac, s));
    return sf_launch_band_selinv(bs.fac, n, halfwidth, batch, 1, d_info, d_out, ldo, out_stride, s);
}

// ----------------------------------------------------------------------------------- likelihood gradient on the band solver
// (the mean-flux columns: sf_loglike_banded_mean_grad_batch; with the covariance columns behind them: sf_loglike_banded_grad_batch)
// What the two calls differ in: the names their messages use, and that the mean call has no want_cov and so requires mean slots
struct BandGradCall {
    const char *who, *dense;
    bool mean_only;
};
static const BandGradCall MEAN_CALL = {"sf_loglike_banded_mean_grad_batch", "sf_loglike_mean_grad_batch", true};
static const BandGradCall GRAD_CALL = {"sf_loglike_banded_grad_batch", "sf_loglike_grad_batch", false};
static int banded_grad_counts_ok(const BandGradCall& k, const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, bool say) {
    // (no context is needed to refuse what no window takes; with one, the limit is that of its 1 + m right-hand sides)
    const int wmax = c && c->n ? sf_banded_window_halfwidth(c) : sf_band_max_halfwidth(1);
    if (halfwidth < 0 || halfwidth > wmax) {
        if (say) sf_set_error("%s: half-width %d outside [0, %d], the LDS window (use %s)", k.who, halfwidth, wmax, k.dense);
        return SF_EINVAL;
    }
    if (model_ok(c, mdl)) return SF_EINVAL;
    if (B <= 0 || B > 65535) {
        if (say) sf_set_error("%s: B=%d must lie in 1 .. 65535", k.who, B);
        return SF_EINVAL;
    }
    return SF_OK;
}
// what the counts of the combined call must satisfy beyond banded_grad_counts_ok; say == false: silently (the size query)
static int banded_grad_slots_ok(const sf_model_desc* mdl, int nslots, int want_cov, bool say) {
    const char* who = GRAD_CALL.who;
    if (nslots < 0 || nslots > SF_MEAN_GRAD_MAX_SLOTS || (nslots == 0 && !want_cov)) {
        if (say) sf_set_error("%s: nothing to differentiate (nslots=%d must lie in 0 .. %d, and be positive without want_cov)", who,
                              nslots, SF_MEAN_GRAD_MAX_SLOTS);
        return SF_EINVAL;
    }
    if (want_cov && sf_cov_grad_slots(mdl->has_global, mdl->n_local) == 0) {
        if (say) sf_set_error("%s: nothing to differentiate (no global and no local kernel)", who);
        return SF_EINVAL;
    }
    return SF_OK;
}
static size_t banded_grad_bytes(const BandGradCall& k, const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nslots,
                                int want_cov) {
    if (banded_grad_counts_ok(k, c, mdl, B, halfwidth, false)) return 0;
    const bool slots_ok = k.mean_only ? nslots >= 1 && nslots <= SF_MEAN_GRAD_MAX_SLOTS  // (as mean_slots_ok has it)
                                      : banded_grad_slots_ok(mdl, nslots, want_cov, false) == SF_OK;
    if (!slots_ok) return 0;
    return carve_band_grad(c, mdl, B, halfwidth, nslots, want_cov != 0, nullptr, 0, carve(c, mdl, B, nullptr, 0, false).bytes).bytes;
}
// The likelihood's head with a keeping sweep, then the backward sweep; then the mean columns (nslots > 0) and, behind them,
// the covariance columns (want_cov) of every walker's row of d_grad
static int banded_grad_call(const BandGradCall& k, sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                            const int* h_slots, int nslots, int want_cov, double* d_lnl, double* d_grad, int grad_stride,
                            double* d_resid, int* d_info, void* d_work, size_t work_bytes, hipStream_t s) {
    if (!d_params || (!h_slots && (k.mean_only || nslots > 0)) || !d_lnl || !d_grad || !d_work) {
        sf_set_error("%s: d_params, h_slots%s, d_lnl, d_grad and d_work are required", k.who, k.mean_only ? "" : " (with nslots > 0)");
        return SF_EINVAL;
    }
    // (the combined call says so before the context is looked at; the mean call leaves nslots = 0 to mean_slots_ok)
    if (!k.mean_only && nslots == 0 && !want_cov) return banded_grad_slots_ok(nullptr, nslots, want_cov, true);
    SF_CHECK(banded_grad_counts_ok(k, c, mdl, B, halfwidth, true));
    if (!k.mean_only) SF_CHECK(banded_grad_slots_ok(mdl, nslots, want_cov, true));
    if (k.mean_only || nslots > 0) SF_CHECK(mean_slots_ok(k.who, c, mdl, h_slots, nslots, grad_stride));
    const int ncols = nslots + (want_cov ? sf_cov_grad_slots(mdl->has_global, mdl->n_local) : 0);
    if (grad_stride < ncols) {
        sf_set_error("%s: grad_stride=%d < %d columns", k.who, grad_stride, ncols);
        return SF_EINVAL;
    }
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandGradWork g = carve_band_grad(c, mdl, B, halfwidth, nslots, want_cov != 0, d_work, work_bytes, w.bytes);
    SF_CHECK(work_fits(work_bytes, g.bytes));
    const BandWork& bw = g.bw;
    const AppliedWork& aw = g.aw;
    SF_CHECK(banded_head(c, mdl, B, d_params, halfwidth, w, bw, BandHead{g.fac, aw.xs, d_resid, nullptr, aw.lnl, aw.info}, s));
    const int n16 = (c->n + 15) / 16 * 16, nrhs = c->m + 1;  // (the sweep's order: whole blocks)
    const int64_t sstage = (int64_t)nrhs * c->npad;
    {
        ProfScope ps(s, PS_SOLVE);
        // T = Bd^-1 [r, Y^T], then [alpha, V] = T M in the staging area
        SF_CHECK(sf_launch_band_back(g.fac, n16, halfwidth, B, nrhs, aw.info, g.T, c->npad, sstage, s));
        SF_CHECK(sf_launch_band_mix(bw.gram, w.Lw, 1, c->m, c->m, aw.info, nullptr, g.T, c->n, c->npad, B, g.M, aw.stage, s));
    }
    if (nslots > 0) {
        const sf_mean_grad_args ma = mean_grad_kernel_args(c, h_slots, nslots, w, aw, d_grad, grad_stride);
        SF_CHECK(sf_launch_mean_tangents(broaden_args(c, mdl, B, d_params, w), c->inv_band.as<double>(),
                                         emu_args(c, mdl, d_params, w, w.mu, nullptr, w.Lw, w.info_e), ma, B, s));
        SF_CHECK(sf_launch_mean_grad(eval_args(c, mdl, d_params, w), ma, w.zs, c->m * c->M, B, s));
    }
    if (want_cov) {
        // the band of Sigma = Bd^-1 and Vs of C^-1 = Sigma - Vs Vs^T, then the contraction with dC / d theta over the band
        SF_CHECK(sf_launch_band_selinv(g.fac, n16, halfwidth, B, nrhs, aw.info, g.sigma, bw.ldb, (int64_t)n16 * bw.ldb, s));
        SF_CHECK(sf_launch_band_vs(bw.gram, 1, c->m, 1, aw.info, g.T, c->n, c->npad, B, g.M2, g.stage2, s));
        SF_CHECK(sf_launch_band_cov_grad(fill_args(c, mdl, d_params, w), B, g.sigma, bw.ldb, (int64_t)n16 * bw.ldb, halfwidth, aw.stage,
                                         g.stage2 + c->npad, c->npad, sstage, c->m, aw.info, g.part, d_grad + nslots, grad_stride, s));
    }
    SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, aw.info, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

extern "C" size_t sf_loglike_banded_mean_grad_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth,
                                                              int nslots) {
    return banded_grad_bytes(MEAN_CALL, c, mdl, B, halfwidth, nslots, 0);
}
extern "C" int sf_loglike_banded_mean_grad_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                                 const int* h_slots, int nslots, double* d_lnl, double* d_grad, int grad_stride,
                                                 double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    return banded_grad_call(MEAN_CALL, c, mdl, B, d_params, halfwidth, h_slots, nslots, 0, d_lnl, d_grad, grad_stride, d_resid, d_info,
                            d_work, work_bytes, (hipStream_t)stream);
}
extern "C" size_t sf_loglike_banded_grad_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nslots,
                                                         int want_cov) {
    return banded_grad_bytes(GRAD_CALL, c, mdl, B, halfwidth, nslots, want_cov);
}
extern "C" int sf_loglike_banded_grad_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                            const int* h_slots, int nslots, int want_cov, double* d_lnl, double* d_grad, int grad_stride,
                                            double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    return banded_grad_call(GRAD_CALL, c, mdl, B, d_params, halfwidth, h_slots, nslots, want_cov, d_lnl, d_grad, grad_stride, d_resid,
                            d_info, d_work, work_bytes, (hipStream_t)stream);
}

// ----------------------------------------------------------------------------------- Fisher information on the band solver
static const char* const FISHER = "sf_fisher_banded_mean_batch";
extern "C" int sf_fisher_banded_max_slots(const sf_ctx* c, int halfwidth) {
    if (!c || !c->n) return SF_EINVAL;
    if (!c->monotonic || c->m < 1 || c->m > 32) return 0;
    for (int k = SF_MEAN_GRAD_MAX_SLOTS; k >= 1; --k)
        if (sfb_admit(halfwidth, 1 + c->m + k) == SFB_WINDOW) return k;
    return 0;
}
// The window's limit, stated once: 1 + m + nslots rows at this half-width.  Without a context (the call looks at it next) m is the
// one low-rank row every order has at least: what no window takes is refused before it.  say == false: silently (the size query)
static int fisher_window_ok(const sf_ctx* c, int halfwidth, int nslots, bool say) {
    const int m = c && c->n ? c->m : 1;
    if (m < 1 || m > 32 || halfwidth < 0 || sfb_admit(halfwidth, 1 + m + nslots) != SFB_WINDOW) {
        if (say)
            sf_set_error("%s: half-width %d with 1 + %d + %d rows lies outside the LDS window (at most %d at this row count; use "
                         "sf_fisher_mean_batch)", FISHER, halfwidth, m, nslots, sf_band_max_halfwidth(1 + m + nslots));
        return SF_EINVAL;
    }
    return SF_OK;
}
// the batch, the context and model, and a grid the band solver takes; say == false: silently
static int fisher_banded_ctx_ok(const sf_ctx* c, const sf_model_desc* mdl, int B, bool say) {
    if (B <= 0 || B > 65535) {
        if (say) sf_set_error("%s: B=%d must lie in 1 .. 65535", FISHER, B);
        return SF_EINVAL;
    }
    if (model_ok(c, mdl)) return SF_EINVAL;
    if (!c->n || !c->monotonic) {
        if (say) sf_set_error("%s: the band solver needs a strictly increasing wavelength grid (use sf_fisher_mean_batch)", FISHER);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_fisher_banded_mean_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nslots) {
    if (fisher_window_ok(c, halfwidth, nslots, false) || fisher_banded_ctx_ok(c, mdl, B, false)) return 0;
    if (!mean_counts_ok(mdl, nslots)) return 0;
    return carve_band_fisher(c, mdl, B, halfwidth, nslots, nullptr, 0, carve(c, mdl, B, nullptr, 0, false).bytes).bytes;
}
// The likelihood's head over the rows [r; Y; J]: one sweep with nslots more rows, no kept factor, no backward sweep
extern "C" int sf_fisher_banded_mean_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                           const int* h_slots, int nslots, double* d_lnl, double* d_fisher, int fisher_stride,
                                           double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    SF_CHECK(fisher_counts_ok(FISHER, d_params && h_slots && d_lnl && d_fisher && d_work, nslots, fisher_stride));
    SF_CHECK(fisher_window_ok(c, halfwidth, nslots, true));
    SF_CHECK(fisher_banded_ctx_ok(c, mdl, B, true));
    SF_CHECK(mean_slots_ok(FISHER, c, mdl, h_slots, nslots, nslots));
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandFisherWork g = carve_band_fisher(c, mdl, B, halfwidth, nslots, d_work, work_bytes, w.bytes);
    SF_CHECK(work_fits(work_bytes, g.bytes));
    hipStream_t s = (hipStream_t)stream;
    const BandHeadFisher f = {h_slots, nslots, &g.aw, g.aw.stage, g.gram, g.twist, d_fisher, fisher_stride};
    SF_CHECK(banded_head(c, mdl, B, d_params, halfwidth, w, g.bw,
                         BandHead{nullptr, g.aw.xs, d_resid, nullptr, d_lnl, g.aw.info, nullptr, nullptr, false, &f}, s));
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, g.aw.info, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

// ----------------------------------------------------------------------------------- residual diagnostics on the band solver
static const char* const DIAGNOSE = "sf_diagnose_banded_batch";
extern "C" int sf_diagnose_banded_max_nrhs(const sf_ctx* c, int halfwidth) {
    if (!c || !c->n) return SF_EINVAL;
    if (!c->monotonic) return 0;
    for (int k = SFB_MIX_MAX_ROWS - c->m; k >= 1; --k)
        if (sfb_admit(halfwidth, c->m + k) == SFB_WINDOW) return k;
    return 0;
}
// what the call refuses on its counts, context and model; say == false: silently (the size query)
static int diagnose_counts_ok(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nrhs, bool say) {
    if (B <= 0 || B > 65535 || nrhs < 1) {
        if (say) sf_set_error("%s: B=%d must lie in 1 .. 65535 and nrhs=%d be positive", DIAGNOSE, B, nrhs);
        return SF_EINVAL;
    }
    if (model_ok(c, mdl)) return SF_EINVAL;
    if (!c->n || !c->monotonic) {
        if (say) sf_set_error("%s: the band solver needs a strictly increasing wavelength grid (use sf_pointwise_batch / sf_decompose_batch)",
                              DIAGNOSE);
        return SF_EINVAL;
    }
    if (c->m < 1 || c->m > 32 || halfwidth < 0 || nrhs > SFB_MIX_MAX_ROWS || sfb_admit(halfwidth, c->m + nrhs) != SFB_WINDOW) {
        if (say)
            sf_set_error("%s: %d low-rank rows + %d right-hand sides at half-width %d exceed the LDS window (at most "
                         "sf_diagnose_banded_max_nrhs = %d per call; or use sf_pointwise_batch / sf_decompose_batch)",
                         DIAGNOSE, c->m, nrhs, halfwidth, halfwidth < 0 ? 0 : sf_diagnose_banded_max_nrhs(c, halfwidth));
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_diagnose_banded_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nrhs,
                                                     int want_cinv_diag, int want_comp) {
    if (diagnose_counts_ok(c, mdl, B, halfwidth, nrhs, false)) return 0;
    return carve_band_diag(c, mdl, B, halfwidth, nrhs, want_cinv_diag != 0, want_comp != 0, nullptr, 0,
                           carve(c, mdl, B, nullptr, 0, false).bytes).bytes;
}
// The likelihood's head with a keeping sweep over [R; Y] (or the gradient call's [r; Y]), the backward sweep and the mix for
// k right-hand sides: alpha in the staging area.  The band is filled entry by entry: on a log-uniform grid the likelihood's table
// of the global kernel per diagonal (k_band_gtab) is off by the rounding of the grid, ~3e-11 in r, which a narrow kernel turns
// into element errors far beyond the 1e-13 that diag(C^-1) is held to against the oracle's matrix; the likelihood's 1e-10 does not
// notice.  On a workspace carved with want_cinv_diag, behind them: the selected inversion (g.sigma) and Vs (g.vs).
// (sf_diagnose_banded_batch; sf_local_scan_banded_batch with the walker's own residual)
static int banded_diag_head(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth, const double* d_rhs,
                            int nrhs, int ldr, int64_t rhs_stride, double* d_flux, const Work& w, const BandDiagWork& g,
                            hipStream_t s) {
    const BandWork& bw = g.bw;
    const AppliedWork& aw = g.aw;
    const BandHeadRhs own = {d_rhs, nrhs, ldr, rhs_stride, g.rhs, g.gram, g.zero};
    SF_CHECK(banded_head(c, mdl, B, d_params, halfwidth, w, bw,
                         BandHead{g.fac, nullptr, nullptr, nullptr, aw.lnl, aw.info, d_flux, d_rhs ? &own : nullptr, true}, s));
    const int n16 = (c->n + 15) / 16 * 16, m = c->m, nin = nrhs + m;  // (the sweep's order: whole blocks)
    const double* gram = d_rhs ? g.gram : bw.gram;
    {
        ProfScope ps(s, PS_SOLVE);
        // T = Bd^-1 [R^T, Y^T], then alpha = T M in the staging area (with caller right-hand sides the mix is the first to
        // look at the capacitance matrix: it completes the status)
        SF_CHECK(sf_launch_band_back(g.fac, n16, halfwidth, B, nin, aw.info, g.T, c->npad, (int64_t)nin * c->npad, s));
        SF_CHECK(sf_launch_band_mix(gram, w.Lw, nrhs, m, 0, aw.info, d_rhs ? aw.info : nullptr, g.T, c->n, c->npad, B, g.M, aw.stage, s));
    }
    if (g.sigma) {
        // the band of Sigma = Bd^-1 and Vs of C^-1 = Sigma - Vs Vs^T
        SF_CHECK(sf_launch_band_selinv(g.fac, n16, halfwidth, B, nin, aw.info, g.sigma, bw.ldb, (int64_t)n16 * bw.ldb, s));
        SF_CHECK(sf_launch_band_vs(gram, nrhs, m, 0, aw.info, g.T, c->n, c->npad, B, g.M2, g.vs, s));
    }
    return SF_OK;
}
// That head, then what is asked for: the read-out of diag(C^-1); the diagonal of C; the split of alpha by covariance component
extern "C" int sf_diagnose_banded_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                        const double* d_rhs, int nrhs, int ldr, int64_t rhs_stride, double* d_alpha,
                                        double* d_cinv_diag, double* d_cov_diag, double* d_comp, double* d_flux, int* d_info,
                                        void* d_work, size_t work_bytes, void* stream) {
    if (!d_params || !d_alpha || !d_work) {
        sf_set_error("%s: d_params, d_alpha and d_work are required", DIAGNOSE);
        return SF_EINVAL;
    }
    if (d_rhs ? rhs_stride < 0 : nrhs != 1) {
        sf_set_error("%s: rhs_stride >= 0 with d_rhs, nrhs == 1 without", DIAGNOSE);
        return SF_EINVAL;
    }
    SF_CHECK(diagnose_counts_ok(c, mdl, B, halfwidth, nrhs, true));
    if (d_rhs && ldr < c->n) {
        sf_set_error("%s: ldr=%d < n (%d)", DIAGNOSE, ldr, c->n);
        return SF_EINVAL;
    }
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandDiagWork g = carve_band_diag(c, mdl, B, halfwidth, nrhs, d_cinv_diag != nullptr, d_comp != nullptr, d_work, work_bytes,
                                           w.bytes);
    SF_CHECK(work_fits(work_bytes, g.bytes));
    const BandWork& bw = g.bw;
    const AppliedWork& aw = g.aw;
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(banded_diag_head(c, mdl, B, d_params, halfwidth, d_rhs, nrhs, ldr, rhs_stride, d_flux, w, g, s));
    const int n16 = (c->n + 15) / 16 * 16, m = c->m;  // (the sweep's order: whole blocks)
    SF_CHECK(sf_launch_apply_export(aw.stage, aw.info, c->n, c->npad, nrhs, B, d_alpha, s));
    if (d_cinv_diag)
        SF_CHECK(sf_launch_band_cinv_diag(g.sigma, bw.ldb, (int64_t)n16 * bw.ldb, g.vs, c->npad, (int64_t)m * c->npad, m, aw.info, c->n,
                                          B, d_cinv_diag, s));
    if (d_cov_diag)
        SF_CHECK(sf_launch_band_cov_diag(bw.band, bw.ldb, (int64_t)c->npad * bw.ldb, w.Y, c->npad, (int64_t)c->mpad * c->npad, m,
                                         aw.info, c->n, B, d_cov_diag, s));
    if (d_comp)  // K_k alpha with the Y, parameter rows and sigma the head's transform chain and fill worked on
        SF_CHECK(sf_launch_cov_matvec(fill_args(c, mdl, d_params, w), m, aw.stage, c->npad, nrhs, B, aw.yv, aw.info, d_comp, s));
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, aw.info, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

// ----------------------------------------------------------------------------------- score scan for new local kernels on the band solver
static const char* const LOCAL_SCAN_BANDED = "sf_local_scan_banded_batch";
// The half-width the head runs at: the widest the LDS window takes for the 1 + m rows [r; Y], whatever the model's own support is
// (a wider band than the kernels need holds zeros: exact) -- so that a candidate's numbers depend on m alone, not on the other
// candidates, the batch or the group.  -1: no window, or a grid the band solver does not take
static int local_scan_banded_halfwidth(const sf_ctx* c) {
    if (!c->n || !c->monotonic || c->m < 1 || c->m > 32) return -1;
    return sf_band_max_halfwidth(1 + c->m);
}
extern "C" int sf_local_scan_banded_max_patch(const sf_ctx* c, const sf_model_desc* mdl) {
    if (model_ok(c, mdl)) return SF_EINVAL;
    return local_scan_banded_halfwidth(c) + 1;
}
// what the call refuses on its counts, context and model; say == false: silently (the size query)
static int local_scan_banded_ok(const sf_ctx* c, const sf_model_desc* mdl, int B, int ncand, bool say) {
    if (B <= 0 || B > 65535 || ncand < 1 || ncand > 65535) {
        if (say) sf_set_error("%s: B=%d and ncand=%d must lie in 1 .. 65535", LOCAL_SCAN_BANDED, B, ncand);
        return SF_EINVAL;
    }
    if (model_ok(c, mdl)) {
        const std::string why = sf_last_error();
        if (say) sf_set_error("%s: %s", LOCAL_SCAN_BANDED, why.c_str());
        return SF_EINVAL;
    }
    if (!c->n || !c->monotonic) {
        if (say)
            sf_set_error("%s: the wavelength grid is not monotonic (the band solver needs a strictly increasing one, and a candidate's "
                         "pixels are no contiguous patch)", LOCAL_SCAN_BANDED);
        return SF_EINVAL;
    }
    if (local_scan_banded_halfwidth(c) < 0) {
        if (say)
            sf_set_error("%s: 1 + %d rows exceed the LDS window at every half-width (use sf_local_scan_batch)", LOCAL_SCAN_BANDED, c->m);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_local_scan_banded_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int ncand) {
    if (local_scan_banded_ok(c, mdl, B, ncand, false)) return 0;
    return carve_band_local_scan(c, mdl, B, local_scan_banded_halfwidth(c), ncand, nullptr, 0, carve(c, mdl, B, nullptr, 0, false).bytes)
        .bytes;
}
// The diagnostics' head for the walker's own residual with the selected inversion and Vs, at the window's widest half-width;
// behind it the tiles of W = Sigma - Vs Vs^T, the candidates' patches and k_ls_cand with the alpha in the staging area
extern "C" int sf_local_scan_banded_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const double* d_cand,
                                          int ncand, double* d_out, double* d_lnl, int* d_info, void* d_work, size_t work_bytes,
                                          void* stream) {
    SF_CHECK(local_scan_banded_ok(c, mdl, B, ncand, true));
    if (!d_params || !d_cand || !d_out || !d_work) {
        sf_set_error("%s: d_params, d_cand, d_out and d_work are required", LOCAL_SCAN_BANDED);
        return SF_EINVAL;
    }
    const int wmax = local_scan_banded_halfwidth(c), n16 = (c->n + 15) / 16 * 16, m = c->m;
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandLocalScanWork g = carve_band_local_scan(c, mdl, B, wmax, ncand, d_work, work_bytes, w.bytes);
    if (work_bytes < g.bytes) {  // (said here, so that the message names the call)
        sf_set_error("%s: workspace too small: have %zu, need %zu", LOCAL_SCAN_BANDED, work_bytes, g.bytes);
        return SF_ENOMEM;
    }
    const BandDiagWork& d = g.d;
    hipStream_t s = (hipStream_t)stream;
    SF_CHECK(banded_diag_head(c, mdl, B, d_params, wmax, nullptr, 1, 0, 0, nullptr, w, d, s));
    SF_CHECK(sf_launch_local_scan_banded(fill_args(c, mdl, d_params, w), B, d.sigma, d.bw.ldb, (int64_t)n16 * d.bw.ldb, wmax, d.vs,
                                         c->npad, (int64_t)m * c->npad, m, d.aw.stage, c->npad, d.aw.info, d_cand, ncand, g.patch,
                                         g.wband, d_out, s));
    if (d_lnl) SF_HIP(hipMemcpyAsync(d_lnl, d.aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, d.aw.info, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}
