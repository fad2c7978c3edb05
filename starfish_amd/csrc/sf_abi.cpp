// C-ABI host layer (include/starfish_amd.h): the stages of the likelihood and the single-order launch sequences.
// Host code only prepares constants (sf_ctx.cpp, sf_hostmath.cpp); all per-walker arithmetic runs in the HIP kernels.
#include "sf_stages.h"

// ----------------------------------------------------------------------------------- stages
sf_emu_args emu_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w, double* d_mu, double* d_cov,
                     double* d_Lw, int* d_info) {
    sf_emu_args e;
    e.params = d_params;
    e.pstride = sf_param_stride(c, mdl);
    e.off_grid = 6;
    e.m = c->m;
    e.M = c->M;
    e.P = c->P;
    e.grid = c->grid.as<double>();
    e.variances = c->variances.as<double>();
    e.lengthscales = c->lengthscales.as<double>();
    e.gmin = c->gmin.as<double>();
    e.gmax = c->gmax.as<double>();
    e.alpha = c->alpha.as<double>();
    e.LinvT = c->Linv.as<double>();
    e.zscratch = w.zs;
    e.kbuf = w.kv;
    e.mu = d_mu;
    e.cov = d_cov;
    e.Lw = d_Lw;
    e.info = d_info;
    return e;
}
static int run_emulator(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w,
                        double* d_mu, double* d_cov, double* d_Lw, int* d_info, hipStream_t s) {
    return sf_launch_emulator(emu_args(c, mdl, d_params, w, d_mu, d_cov, d_Lw, d_info), B, s);
}

int export_info(int* d_info, const Work& w, int units, hipStream_t s) {
    if (d_info) SF_HIP(hipMemcpyAsync(d_info, w.info_e, sizeof(int) * (size_t)units, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}
int export_logdet_sqmah(double* d_logdet, double* d_sqmah, const Work& w, int units, hipStream_t s) {
    if (d_logdet) SF_HIP(hipMemcpyAsync(d_logdet, w.logdet, sizeof(double) * (size_t)units, hipMemcpyDeviceToDevice, s));
    if (d_sqmah) SF_HIP(hipMemcpyAsync(d_sqmah, w.sqmah, sizeof(double) * (size_t)units, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}
// the residual rows without their padding
static int export_resid(double* d_resid_out, const sf_ctx* c, const Work& w, int B, hipStream_t s) {
    if (d_resid_out)
        SF_HIP(hipMemcpy2DAsync(d_resid_out, sizeof(double) * c->n, w.resid, sizeof(double) * w.L.npad,
                                sizeof(double) * c->n, B, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

// the rotational broadening of the context's half spectra into w.ybro
sf_broaden_args broaden_args(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w) {
    sf_broaden_args a;
    a.in = nullptr;
    a.spec = c->spec.as<double2>();
    a.B = B;
    a.rows = c->rows;
    a.nf = c->nf;
    a.tw = c->tw.as<double2>();
    a.dv = c->dv;
    a.kind = 1;
    a.params = d_params;
    a.pstride = sf_param_stride(c, mdl);
    a.poff = 0;
    a.scalar_param = 0.0;
    a.out = w.ybro;  // [B][rows][nf]: every row contiguous (coalesced stores)
    a.ob = (int64_t)c->nf * c->rows;
    a.orow = c->nf;
    a.oelem = 1;
    a.gscratch = w.fft;
    a.mult = w.mult;
    a.info = w.info_e;
    return a;
}
// the per-pixel evaluation's arguments on the workspace w (the coefficients: the walkers' own behind the broadening)
sf_eval_args eval_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w) {
    sf_eval_args ev;
    ev.wave = c->wave.as<double>();
    ev.knots = c->knots.as<double>();
    ev.coef = mdl->has_vsini ? w.coef : c->coef_static.as<double>();
    ev.coef_batched = mdl->has_vsini ? 1 : 0;
    ev.params = d_params;
    ev.mu = w.mu;
    ev.X = w.Xraw;
    ev.flux = w.fraw;
    ev.info = w.info_e;
    ev.n = c->n;
    ev.nf = c->nf;
    ev.m = c->m;
    ev.ldx = w.L.npad;
    ev.pstride = sf_param_stride(c, mdl);
    ev.has_vz = mdl->has_vz;
    ev.n_cheb = mdl->n_cheb;
    ev.off_cheb = 6 + c->P;
    ev.has_av = mdl->has_av;
    ev.off_av = 6 + c->P + mdl->n_cheb + 3 * mdl->n_local;
    ev.wave_max = c->wave_max;
    return ev;
}

// emulator + transform chain -> unscaled X / flux, scale, then residual / Y
int run_transforms(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w, double* d_flux_out,
                   double* d_X_out, double* d_resid_out, double* d_log_scale, bool want_Y, hipStream_t s) {
    // (the broadening + spline-fit launches depend on vsini only, not on the emulator; forked onto a stream of their own beside
    // the emulator's launches and the band fill they do not shorten the banded step: every one of these launches fills the chip
    // by itself -- with three streams each simply takes longer, profiles/r05_q_banded_step_timelines.txt)
    const int pstride = sf_param_stride(c, mdl);
    SF_HIP(hipMemsetAsync(w.info_e, 0, sizeof(int) * (size_t)B, s));
    int rc = run_emulator(c, mdl, B, d_params, w, w.mu, nullptr, w.Lw, w.info_e, s);
    if (rc) return rc;
    if (mdl->has_vsini) {
        rc = sf_launch_broaden(broaden_args(c, mdl, B, d_params, w), s);
        if (rc) return rc;
        // spline coefficients of the broadened rows: truncated-inverse band product (fully parallel)
        rc = sf_launch_spline_apply(w.ybro, w.coef, B, c->rows, c->nf, c->inv_band.as<double>(), s);
        if (rc) return rc;
    }
    const sf_eval_args ev = eval_args(c, mdl, d_params, w);
    sf_resid_args r;
    r.dflux = c->flux.as<double>();
    r.flux = w.fraw;
    r.X = w.Xraw;
    r.scale = w.scale;
    r.Lw = w.Lw;
    r.info = w.info_e;
    r.resid = w.resid;
    r.Y = want_Y ? w.Y : nullptr;
    r.flux_out = d_flux_out;
    r.X_out = d_X_out;
    r.n = c->n;
    r.m = c->m;
    r.mpad = c->mpad;
    r.ldx = w.L.npad;
    r.ldy = w.L.npad;
    r.use_sigma_w = mdl->use_sigma_w;
    // the scale factor does not depend on the flux when it is given: rows, scale and residual / Y in one pass, X never stored
    static const bool unfused = SF_TUNE_FLAG("SF_TRANSFORM_UNFUSED");  // (tests: the three launches give the same bits)
    if (mdl->has_log_scale && !unfused) {
        rc = sf_launch_eval_resid_y(ev, r, w.scale, d_log_scale, B, s);
        if (rc) return rc;
    } else {
        rc = sf_launch_eval_rows(ev, B, s);
        if (rc) return rc;

        sf_scale_args sc;
        sc.wave = c->wave.as<double>();
        sc.dflux = c->flux.as<double>();
        sc.flux = w.fraw;
        sc.params = d_params;
        sc.scale = w.scale;
        sc.log_scale_out = d_log_scale;
        sc.n = c->n;
        sc.ldx = w.L.npad;
        sc.pstride = pstride;
        sc.has_log_scale = mdl->has_log_scale;
        rc = sf_launch_scale(sc, B, s);
        if (rc) return rc;

        rc = sf_launch_resid_y(r, B, s);
        if (rc) return rc;
    }
    return export_resid(d_resid_out, c, w, B, s);
}

sf_fill_args fill_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w) {
    sf_fill_args f;
    f.wave = c->wave.as<double>();
    f.sigma = c->sigma.as<double>();
    f.Y = w.Y;
    f.params = d_params;
    f.n = c->n;
    f.npad = w.L.npad;
    f.mpad = c->mpad;
    f.ldy = w.L.npad;
    f.pstride = sf_param_stride(c, mdl);
    f.has_global = mdl->has_global;
    f.n_local = mdl->n_local;
    f.off_global = 4;
    f.off_local = 6 + c->P + mdl->n_cheb;
    f.monotonic = c->monotonic;
    f.loguniform = c->loguniform;
    f.nout = 0;
    f.tilemap = nullptr;
    f.nt128 = 0;
    f.fp = 0;
    f.tilelist = nullptr;
    f.tilecount = nullptr;
    f.list_cap = 0;
    f.gtab = nullptr;
    return f;
}

// ----------------------------------------------------------------------------------- single-order calls
extern "C" size_t sf_workspace_bytes(const sf_ctx* c, const sf_model_desc* mdl, int B) {
    if (model_ok(c, mdl) || B <= 0) return 0;
    return carve(c, mdl, B, nullptr, 0, true).bytes;
}
int open_call(const sf_ctx* c, const sf_model_desc* mdl, int B, void* d_work, size_t have, bool need_C, Work* w) {
    if (model_ok(c, mdl)) return SF_EINVAL;
    if (B <= 0 || !d_work) {
        sf_set_error("bad batch size / workspace");
        return SF_EINVAL;
    }
    *w = carve(c, mdl, B, d_work, have, need_C);
    int rc = work_fits(have, w->bytes);
    if (rc) return rc;
    return use_device(c);
}

extern "C" int sf_emulator_query_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                       double* d_mu, double* d_cov, int* d_info, void* d_work,
                                       size_t work_bytes, void* stream) {
    Work w;
    int rc = open_call(c, mdl, B, d_work, work_bytes, false, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    int* info = d_info ? d_info : w.info_e;
    SF_HIP(hipMemsetAsync(info, 0, sizeof(int) * (size_t)B, s));
    return run_emulator(c, mdl, B, d_params, w, d_mu ? d_mu : w.mu, d_cov, w.Lw, info, s);
}

extern "C" int sf_emulator_joint_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                       double* d_mu, double* d_cov, int* d_info, void* d_work,
                                       size_t work_bytes, void* stream) {
    Work w;
    int rc = open_call(c, mdl, B, d_work, work_bytes, false, &w);
    if (rc) return rc;
    if (!d_mu || !d_cov) {
        sf_set_error("sf_emulator_joint_batch: d_mu and d_cov are required");
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    int* info = d_info ? d_info : w.info_e;
    SF_HIP(hipMemsetAsync(info, 0, sizeof(int) * (size_t)B, s));
    rc = run_emulator(c, mdl, B, d_params, w, w.mu, nullptr, nullptr, info, s);
    if (rc) return rc;
    return sf_launch_emu_joint(emu_args(c, mdl, d_params, w, w.mu, nullptr, nullptr, info), B, w.mu, d_mu, d_cov, s);
}

extern "C" int sf_transform_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                  double* d_flux, double* d_X, double* d_resid, double* d_log_scale,
                                  int* d_info, void* d_work, size_t work_bytes, void* stream) {
    Work w;
    int rc = open_call(c, mdl, B, d_work, work_bytes, false, &w);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = run_transforms(c, mdl, B, d_params, w, d_flux, d_X, d_resid, d_log_scale, false, s);
    if (rc) return rc;
    return export_info(d_info, w, B, s);
}

// dense (both triangles unless lower_only) covariance matrices of the caller
static int fill_dense(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, const Work& w, double* d_cov, int ld,
                      int64_t stride, int lower_only, int add_jitter, int nout, hipStream_t s) {
    sf_fill_args f = fill_args(c, mdl, d_params, w);
    f.C = d_cov;
    f.lda = ld;
    f.stride = stride;
    f.lower_only = lower_only;
    f.add_jitter = add_jitter;
    f.nout = nout;
    int rc = sf_exec_prepare(&c->exec);
    if (rc) return rc;
    return sf_launch_fill_dense(f, B, w.dmap, w.dlist, w.dcount, s, &c->exec);  // (lower_only: the tile grid of sf_launch_fill)
}

extern "C" int sf_forward_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                double* d_flux, double* d_cov, double* d_log_scale, int* d_info,
                                void* d_work, size_t work_bytes, void* stream) {
    Work w;
    int rc = open_call(c, mdl, B, d_work, work_bytes, false, &w);
    if (rc) return rc;
    if (!d_cov) {
        sf_set_error("sf_forward_batch: d_cov is required");
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    rc = run_transforms(c, mdl, B, d_params, w, d_flux, nullptr, nullptr, d_log_scale, true, s);
    if (rc) return rc;
    rc = fill_dense(c, mdl, B, d_params, w, d_cov, c->n, (int64_t)c->n * c->n, 0, 0, 0, s);
    if (rc) return rc;
    return export_info(d_info, w, B, s);
}

extern "C" int sf_cov_fill_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params, double* d_cov, int ld,
                                 int64_t stride, int lower_only, int add_jitter, int* d_info, void* d_work, size_t work_bytes,
                                 void* stream) {
    Work w;
    int rc = open_call(c, mdl, B, d_work, work_bytes, false, &w);
    if (rc) return rc;
    if (!d_cov || ld < c->n || stride < (int64_t)c->n * ld) {
        sf_set_error("sf_cov_fill_batch: d_cov required, ld >= n (%d), stride >= n * ld", c->n);
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    prof_count_call();
    {
        // (the rank-m term needs Y = L_w^-1 (Omega X): the transform chain and the emulator query run first)
        ProfScope ps(s, PS_TRANSFORM);
        rc = run_transforms(c, mdl, B, d_params, w, nullptr, nullptr, nullptr, nullptr, true, s);
        if (rc) return rc;
    }
    {
        ProfScope ps(s, PS_FILL);
        // (nout: the caller's matrices have n rows: no identity padding, it belongs to the workspace layout only)
        rc = fill_dense(c, mdl, B, d_params, w, d_cov, ld, stride, lower_only ? 1 : 0, add_jitter ? 1 : 0, c->n, s);
        if (rc) return rc;
    }
    return export_info(d_info, w, B, s);
}

sf_fill_args loglike_fill_args(sf_ctx* c, const sf_model_desc* mdl, const double* d_params, const Work& w, const Layout& L,
                               int fp) {
    sf_fill_args f = fill_args(c, mdl, d_params, w);
    f.C = w.C;
    f.lda = L.lda;
    f.stride = (int64_t)L.npad * L.lda;
    f.lower_only = 1;
    f.add_jitter = 1;
    f.gtab = w.gtab;  // per-diagonal table of the global kernel (used on log-uniform grids only)
    f.tilemap = w.tilemap;
    f.tilelist = w.tilelist;
    f.tilecount = w.tilecount;
    f.list_cap = (int)tilemap_bytes(L);
    f.fp = fp;
    f.nt128 = (L.npad + fp + 127) / 128;
    return f;
}
int loglike_factor_finish(const Work& w, const Layout& L, int fp, int units, double* ltbuf, double* d_lnl, int* d_info,
                          hipStream_t s, sf_exec* ex) {
    const int64_t stride = (int64_t)L.npad * L.lda;
    int rc;
    {
        ProfScope ps(s, PS_POTRF);
        sf_gen_args gen;
        gen.Y = w.Y;
        gen.mpad = L.mpad;
        gen.ldy = L.npad;
        gen.tilemap = w.tilemap;
        gen.fp = fp;
        gen.nt128 = (L.npad + fp + 127) / 128;
        rc = sf_launch_potrf(w.C, L.npad, L.lda, stride, units, w.info_c, ltbuf, w.resid, L.npad, s, &gen, ex);
        if (rc) return rc;
    }
    {
        ProfScope ps(s, PS_SOLVE);
        rc = sf_launch_logdet_z(w.C, L.npad, L.lda, stride, units, w.resid, L.npad, w.logdet, w.sqmah, s);
        if (rc) return rc;
        rc = sf_launch_finish(units, w.logdet, w.sqmah, w.info_e, w.info_c, d_lnl, d_info, s);
        if (rc) return rc;
    }
    return SF_OK;
}

extern "C" int sf_loglike_batch(sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                                double* d_lnl, double* d_logdet, double* d_sqmah, double* d_resid,
                                double* d_log_scale, int* d_info, void* d_work, size_t work_bytes,
                                void* stream) {
    Work w;
    int rc = open_call(c, mdl, B, d_work, work_bytes, true, &w);
    if (rc) return rc;
    if (!d_lnl) {
        sf_set_error("sf_loglike_batch: d_lnl is required");
        return SF_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    prof_count_call();
    const Layout L = layout_of(c);
    {
        ProfScope ps(s, PS_TRANSFORM);
        rc = run_transforms(c, mdl, B, d_params, w, nullptr, nullptr, d_resid, d_log_scale, true, s);
        if (rc) return rc;
    }
    // (the tiles of the factorisation's frame: see sf_potrf_front_pad.  Evaluated ONCE per call and handed on to the fill
    // and the factorisation: it depends on the process-global persistent-kernel switch, which a recovery on another host
    // thread may flip between the two stages -- tile map and factorisation must agree on the frame)
    const int fp = sf_potrf_front_pad(c->npad, B);
    {
        ProfScope ps(s, PS_FILL);
        rc = sf_launch_fill(loglike_fill_args(c, mdl, d_params, w, L, fp), B, s);
        if (rc) return rc;
    }
    rc = loglike_factor_finish(w, L, fp, B, w.ltbuf, d_lnl, d_info, s, &c->exec);
    if (rc) return rc;
    return export_logdet_sqmah(d_logdet, d_sqmah, w, B, s);
}
