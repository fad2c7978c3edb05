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
extern "C" int sf_loglike_banded_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                       int halfwidth, double* d_lnl, double* d_logdet, double* d_sqmah,
                                       double* d_resid, double* d_log_scale, int* d_info, void* d_work,
                                       size_t work_bytes, void* stream) {
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
    Work w = carve(c, mdl, B, d_work, work_bytes, false);
    BandWork bw = carve_band(c, B, halfwidth, d_work, work_bytes, w.bytes);
    int rc = work_fits(work_bytes, bw.bytes);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (use_device(c)) return SF_EHIP;
    prof_count_call();
    // The band fill depends on the covariance hyper-parameters only, the transforms on the stellar ones:
    // the two run side by side (fill on a library-owned auxiliary stream, joined before the sweep).
    sf_exec* aux = &c->exec;
    rc = sf_exec_prepare(aux);
    if (rc) return rc;
    hipStream_t sf = aux->aux;
    if (sf != s) {
        SF_HIP(hipEventRecord(aux->fork, s));
        SF_HIP(hipStreamWaitEvent(sf, aux->fork, 0));
    }
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
        f.npad = (c->n + 15) / 16 * 16;
        if (bw.tiles) {  // straight into the 128 x 128 tiles of the bordered band matrix
            static const bool poison = SF_TUNE_FLAG("SF_BAND_TILES_POISON");  // test aid: NaN wherever a tile is read before it is written
            if (poison) SF_HIP(hipMemsetAsync(bw.tiles, 0xff, sizeof(double) * sf_band_tiles_doubles(c->npad, B), sf));
            f.npad = c->npad;
            const int lda_t = sf_band_tiles_lda(c->npad);
            rc = sf_launch_band_fill(f, B, bw.tiles, bw.ldb, halfwidth, lda_t, (int64_t)(c->npad + 64) * lda_t, w.info_c, bw.gtab, sf,
                                     sf_band_tiles_wt(halfwidth));
        } else
            rc = sf_launch_band_fill(f, B, bw.band, halfwidth + 1, halfwidth, bw.ldb, sband, w.info_c, bw.gtab, sf);
        if (rc) return rc;
    }
    if (sf != s) SF_HIP(hipEventRecord(aux->join, sf));
    {
        ProfScope ps(s, PS_TRANSFORM);
        rc = run_transforms(c, mdl, B, d_params, w, nullptr, nullptr, d_resid, d_log_scale, true, s);
        if (rc) return rc;
    }
    if (sf != s) SF_HIP(hipStreamWaitEvent(s, aux->join, 0));
    {
        ProfScope ps(s, PS_POTRF);
        sf_band_call k = {};
        k.band = bw.band, k.sband = sband, k.ldb = bw.ldb, k.halfwidth = halfwidth;
        k.n = bw.tiles ? c->n : (c->n + 15) / 16 * 16;  // (the window's band is filled with identity rows up to whole blocks)
        k.batch = B;
        k.r = sf_band_rhs{w.Y, (int64_t)c->mpad * c->npad, c->npad, c->m + 1, w.resid, c->npad};
        k.logdet = bw.logdet_band, k.gram = bw.gram, k.info = w.info_c;
        if (bw.tiles) rc = sf_launch_potrf_band(k, c->npad, bw.tiles, s);
        else if (sf_band_twisted_applicable(k.n, halfwidth, B)) rc = sf_launch_band_forms_twisted(k, bw.twist, s);
        else rc = sf_launch_band_forms(k, s);
        if (rc) return rc;
    }
    {
        ProfScope ps(s, PS_SOLVE);
        rc = sf_launch_woodbury(bw.gram, c->m + 1, B, bw.logdet_band, w.logdet, w.sqmah, w.info_c, s);
        if (rc) return rc;
        rc = sf_launch_finish(B, w.logdet, w.sqmah, w.info_e, w.info_c, d_lnl, d_info, s);
        if (rc) return rc;
    }
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
    sf_band_call k = {};
    k.band = d_band, k.sband = stride, k.ldb = ldb, k.halfwidth = halfwidth;
    k.n = n, k.batch = batch;
    k.r = sf_band_rhs{d_rhs, rhs_stride, ldr, nrhs, nullptr, 0};
    k.logdet = d_logdet, k.gram = d_gram, k.info = d_info;
    return sf_launch_band_forms(k, s);
}

// ----------------------------------------------------------------------------------- the full banded solve
// what sf_band_solve_batch refuses before it touches the device; who == NULL: silently (the size query)
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
    sf_band_call k = {};
    k.band = d_band, k.sband = stride, k.ldb = ldb, k.halfwidth = halfwidth;
    k.n = n, k.batch = batch;
    k.r = sf_band_rhs{d_rhs, rhs_stride, ldr, nrhs, nullptr, 0};
    k.logdet = d_logdet, k.gram = d_gram ? d_gram : bs.gram, k.info = d_info;
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
    sf_band_call k = {};
    k.band = d_band, k.sband = stride, k.ldb = ldb, k.halfwidth = halfwidth;
    k.n = n, k.batch = batch;
    k.r = sf_band_rhs{bs.zero, 0, n, 1, nullptr, 0};
    k.logdet = d_logdet, k.gram = bs.gram, k.info = d_info;
    SF_CHECK(sf_launch_band_keep(k, bs.fac, s));
    return sf_launch_band_selinv(bs.fac, n, halfwidth, batch, 1, d_info, d_out, ldo, out_stride, s);
}

// ----------------------------------------------------------------------------------- likelihood gradient on the band solver
// (the mean-flux columns: sf_loglike_banded_mean_grad_batch; with the covariance columns behind them: sf_loglike_banded_grad_batch)
static int banded_grad_counts_ok(const char* who, const char* dense, const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth,
                                 bool say) {
    // (no context is needed to refuse what no window takes; with one, the limit is that of its 1 + m right-hand sides)
    const int wmax = c && c->n ? sf_banded_window_halfwidth(c) : sf_band_max_halfwidth(1);
    if (halfwidth < 0 || halfwidth > wmax) {
        if (say) sf_set_error("%s: half-width %d outside [0, %d], the LDS window (use %s)", who, halfwidth, wmax, dense);
        return SF_EINVAL;
    }
    if (model_ok(c, mdl)) return SF_EINVAL;
    if (B <= 0 || B > 65535) {
        if (say) sf_set_error("%s: B=%d must lie in 1 .. 65535", who, B);
        return SF_EINVAL;
    }
    return SF_OK;
}
// One band fill, one keeping sweep, the capacitance step and the backward sweep; then the mean columns (nslots > 0) and,
// behind them, the covariance columns (cv != NULL) of every walker's row of d_grad
static int banded_grad_run(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth, const int* h_slots,
                           int nslots, const Work& w, const BandGradWork& g, const BandCovGradWork* cv, double* d_lnl, double* d_grad,
                           int grad_stride, double* d_resid, int* d_info, hipStream_t s) {
    const BandWork& bw = g.bw;
    const AppliedWork& aw = g.aw;
    if (use_device(c)) return SF_EHIP;
    prof_count_call();
    // band fill and transforms side by side, as in sf_loglike_banded_batch
    sf_exec* aux = &c->exec;
    SF_CHECK(sf_exec_prepare(aux));
    hipStream_t sf = aux->aux;
    if (sf != s) {
        SF_HIP(hipEventRecord(aux->fork, s));
        SF_HIP(hipStreamWaitEvent(sf, aux->fork, 0));
    }
    const int n16 = (c->n + 15) / 16 * 16, nrhs = c->m + 1;  // (the window's band is filled with identity rows up to whole blocks)
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
        f.npad = n16;
        SF_CHECK(sf_launch_band_fill(f, B, bw.band, halfwidth + 1, halfwidth, bw.ldb, sband, w.info_c, bw.gtab, sf));
    }
    if (sf != s) SF_HIP(hipEventRecord(aux->join, sf));
    {
        ProfScope ps(s, PS_TRANSFORM);
        SF_CHECK(run_transforms(c, mdl, B, d_params, w, nullptr, aw.xs, d_resid, nullptr, true, s));
    }
    if (sf != s) SF_HIP(hipStreamWaitEvent(s, aux->join, 0));
    {
        ProfScope ps(s, PS_POTRF);
        sf_band_call k = {};
        k.band = bw.band, k.sband = sband, k.ldb = bw.ldb, k.halfwidth = halfwidth;
        k.n = n16, k.batch = B;
        k.r = sf_band_rhs{w.Y, (int64_t)c->mpad * c->npad, c->npad, nrhs, w.resid, c->npad};
        k.logdet = bw.logdet_band, k.gram = bw.gram, k.info = w.info_c;
        SF_CHECK(sf_launch_band_keep(k, g.fac, s));
    }
    const int64_t sstage = (int64_t)nrhs * c->npad;
    {
        ProfScope ps(s, PS_SOLVE);
        SF_CHECK(sf_launch_woodbury(bw.gram, nrhs, B, bw.logdet_band, w.logdet, w.sqmah, w.info_c, s));
        SF_CHECK(sf_launch_finish(B, w.logdet, w.sqmah, w.info_e, w.info_c, aw.lnl, aw.info, s));
        // T = Bd^-1 [r, Y^T], then [alpha, V] = T M in the staging area
        SF_CHECK(sf_launch_band_back(g.fac, n16, halfwidth, B, nrhs, aw.info, g.T, c->npad, sstage, s));
        SF_CHECK(sf_launch_band_mix(bw.gram, w.Lw, c->m, aw.info, g.T, c->n, c->npad, B, g.M, aw.stage, s));
    }
    if (nslots > 0) {
        const sf_mean_grad_args ma = mean_grad_kernel_args(c, h_slots, nslots, w, aw, d_grad, grad_stride);
        SF_CHECK(sf_launch_mean_tangents(broaden_args(c, mdl, B, d_params, w), c->inv_band.as<double>(),
                                         emu_args(c, mdl, d_params, w, w.mu, nullptr, w.Lw, w.info_e), ma, B, s));
        SF_CHECK(sf_launch_mean_grad(eval_args(c, mdl, d_params, w), ma, w.zs, c->m * c->M, B, s));
    }
    if (cv) {
        // the band of Sigma = Bd^-1 and Vs of C^-1 = Sigma - Vs Vs^T, then the contraction with dC / d theta over the band
        SF_CHECK(sf_launch_band_selinv(g.fac, n16, halfwidth, B, nrhs, aw.info, cv->sigma, bw.ldb, (int64_t)n16 * bw.ldb, s));
        SF_CHECK(sf_launch_band_vs(bw.gram, c->m, aw.info, g.T, c->n, c->npad, B, cv->M2, cv->stage2, s));
        SF_CHECK(sf_launch_band_cov_grad(fill_args(c, mdl, d_params, w), B, cv->sigma, bw.ldb, (int64_t)n16 * bw.ldb, halfwidth, aw.stage,
                                         cv->stage2 + c->npad, c->npad, sstage, c->m, aw.info, cv->part, d_grad + nslots, grad_stride, s));
    }
    SF_HIP(hipMemcpyAsync(d_lnl, aw.lnl, sizeof(double) * (size_t)B, hipMemcpyDeviceToDevice, s));
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, aw.info, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

static const char MEAN_NAME[] = "sf_loglike_banded_mean_grad_batch", MEAN_DENSE[] = "sf_loglike_mean_grad_batch";
extern "C" size_t sf_loglike_banded_mean_grad_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth,
                                                              int nslots) {
    if (banded_grad_counts_ok(MEAN_NAME, MEAN_DENSE, c, mdl, B, halfwidth, false) || nslots < 1 || nslots > SF_MEAN_GRAD_MAX_SLOTS)
        return 0;
    return carve_band_grad(c, mdl, B, halfwidth, nslots, nullptr, 0, carve(c, mdl, B, nullptr, 0, false).bytes).bytes;
}
extern "C" int sf_loglike_banded_mean_grad_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                                 const int* h_slots, int nslots, double* d_lnl, double* d_grad, int grad_stride,
                                                 double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    if (!d_params || !h_slots || !d_lnl || !d_grad || !d_work) {
        sf_set_error("sf_loglike_banded_mean_grad_batch: d_params, h_slots, d_lnl, d_grad and d_work are required");
        return SF_EINVAL;
    }
    SF_CHECK(banded_grad_counts_ok(MEAN_NAME, MEAN_DENSE, c, mdl, B, halfwidth, true));
    SF_CHECK(mean_slots_ok(MEAN_NAME, c, mdl, h_slots, nslots, grad_stride));
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandGradWork g = carve_band_grad(c, mdl, B, halfwidth, nslots, d_work, work_bytes, w.bytes);
    SF_CHECK(work_fits(work_bytes, g.bytes));
    return banded_grad_run(c, mdl, B, d_params, halfwidth, h_slots, nslots, w, g, nullptr, d_lnl, d_grad, grad_stride, d_resid, d_info,
                           (hipStream_t)stream);
}

static const char GRAD_NAME[] = "sf_loglike_banded_grad_batch", GRAD_DENSE[] = "sf_loglike_grad_batch";
// what the counts of the combined call must satisfy beyond banded_grad_counts_ok; say == false: silently (the size query)
static int banded_grad_slots_ok(const sf_model_desc* mdl, int nslots, int want_cov, bool say) {
    if (nslots < 0 || nslots > SF_MEAN_GRAD_MAX_SLOTS || (nslots == 0 && !want_cov)) {
        if (say) sf_set_error("%s: nothing to differentiate (nslots=%d must lie in 0 .. %d, and be positive without want_cov)", GRAD_NAME,
                              nslots, SF_MEAN_GRAD_MAX_SLOTS);
        return SF_EINVAL;
    }
    if (want_cov && sf_cov_grad_slots(mdl->has_global, mdl->n_local) == 0) {
        if (say) sf_set_error("%s: nothing to differentiate (no global and no local kernel)", GRAD_NAME);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_loglike_banded_grad_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B, int halfwidth, int nslots,
                                                         int want_cov) {
    if (banded_grad_counts_ok(GRAD_NAME, GRAD_DENSE, c, mdl, B, halfwidth, false) || banded_grad_slots_ok(mdl, nslots, want_cov, false))
        return 0;
    return carve_band_cov_grad(c, mdl, B, halfwidth, nslots, want_cov != 0, nullptr, 0, carve(c, mdl, B, nullptr, 0, false).bytes).bytes;
}
extern "C" int sf_loglike_banded_grad_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, int halfwidth,
                                            const int* h_slots, int nslots, int want_cov, double* d_lnl, double* d_grad, int grad_stride,
                                            double* d_resid, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    if (!d_params || (!h_slots && nslots > 0) || !d_lnl || !d_grad || !d_work) {
        sf_set_error("sf_loglike_banded_grad_batch: d_params, h_slots (with nslots > 0), d_lnl, d_grad and d_work are required");
        return SF_EINVAL;
    }
    if (nslots == 0 && !want_cov) return banded_grad_slots_ok(nullptr, nslots, want_cov, true);  // (before the context is looked at)
    SF_CHECK(banded_grad_counts_ok(GRAD_NAME, GRAD_DENSE, c, mdl, B, halfwidth, true));
    SF_CHECK(banded_grad_slots_ok(mdl, nslots, want_cov, true));
    if (nslots > 0) SF_CHECK(mean_slots_ok(GRAD_NAME, c, mdl, h_slots, nslots, grad_stride));
    const int ncols = nslots + (want_cov ? sf_cov_grad_slots(mdl->has_global, mdl->n_local) : 0);
    if (grad_stride < ncols) {
        sf_set_error("%s: grad_stride=%d < %d columns", GRAD_NAME, grad_stride, ncols);
        return SF_EINVAL;
    }
    const Work w = carve(c, mdl, B, d_work, work_bytes, false);
    const BandCovGradWork cv = carve_band_cov_grad(c, mdl, B, halfwidth, nslots, want_cov != 0, d_work, work_bytes, w.bytes);
    SF_CHECK(work_fits(work_bytes, cv.bytes));
    return banded_grad_run(c, mdl, B, d_params, halfwidth, h_slots, nslots, w, cv.g, want_cov ? &cv : nullptr, d_lnl, d_grad,
                           grad_stride, d_resid, d_info, (hipStream_t)stream);
}
