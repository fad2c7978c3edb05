// C-ABI host layer: multi-order batches.
// The units of several orders (the reference's multi-order spectra, Starfish/spectrum.py:96-115; orders are
// independent, docs/intro.rst:71-73) share ONE batched factorisation: every order runs its own transform chain
// and covariance fill into its slice of a common [units][npad][lda] array, padded (identity block) to the largest
// order of the group; the Cholesky, which is where the time goes, then sees sum(B_i) matrices in one launch
// sequence instead of nseg half-filled ones, and the host synchronises once.
// sf_loglike_multi_grad_batch_md is the same sequence with a gradient part (MultiGradCall): right-hand sides staged behind
// every order's chain, the factor applied to a whole chunk's staging area at once, and per segment the contractions of the
// two single-order gradient calls -- one factorisation per unit for the likelihood and its gradient.
// The calls on the band + Woodbury solver are in sf_multi_banded.cpp; sf_multi_grad_reduce and sf_multi_fisher_reduce (at the
// end) are the sums of the unit gradients and of the unit Fisher matrices over the orders.
#include <cstdio>
#include <string>

#include "sf_multi_pipeline.h"

int multi_layout(const sf_segment* segs, int nseg, const sf_model_desc* const* models, Layout* L, int* units, int* bmax,
                 sf_model_desc* uni) {
    if (!segs || nseg <= 0 || !models) {
        sf_set_error("multi-order call: bad segment list / model descriptor");
        return SF_EINVAL;
    }
    for (int i = 0; i < nseg; ++i) {
        if (!models[i]) {
            sf_set_error("multi-order call: segment %d has no model descriptor", i);
            return SF_EINVAL;
        }
    }
    const sf_ctx* c0 = segs[0].ctx;
    *uni = *models[0];
    long long U = 0;
    int bm = 0;
    for (int i = 0; i < nseg; ++i) {
        const sf_ctx* c = segs[i].ctx;
        if (!c || !c->n || segs[i].B <= 0 || !segs[i].d_params) {
            sf_set_error("multi-order call: segment %d has no order context / batch / parameters", i);
            return SF_EINVAL;
        }
        if (model_ok(c, models[i])) {
            const std::string why = sf_last_error();
            sf_set_error("multi-order call: segment %d: %s", i, why.c_str());
            return SF_EINVAL;
        }
        if (c->device != c0->device || c->m != c0->m || c->P != c0->P) {
            sf_set_error("multi-order call: segment %d differs from segment 0 in device, eigenspectra or grid dimensions", i);
            return SF_EINVAL;
        }
        if (models[i]->has_vsini) uni->has_vsini = 1;
        if (i == 0) *L = layout_of(c0);
        L->M = std::max(L->M, c->M);
        L->nf = std::max(L->nf, c->nf);
        L->npad = std::max(L->npad, c->npad);
        U += segs[i].B;
        bm = std::max(bm, (int)segs[i].B);
    }
    L->lda = L->npad + 16;
    if (U > 0x3fffffffLL) {
        sf_set_error("multi-order call: too many units");
        return SF_EINVAL;
    }
    *units = (int)U;
    *bmax = bm;
    return SF_OK;
}
// the most units a chunk of the pipeline (sf_multi_pipeline.h) can hold
static int multi_chunk_cap(int U, int bmax) { return std::min(U, std::max(U - multi_first_units(U), multi_first_units(U) + bmax)); }
// the workspace of U units in all, at most bmax of one order
static Work carve_multi(const Layout& L, const sf_model_desc& uni, int U, int bmax, void* p, size_t cap) {
    return carve(L, &uni, U, bmax, p, cap, true, multi_chunk_cap(U, bmax), SF_MULTI_LANES);
}
static size_t multi_workspace_bytes(const sf_segment* segs, int nseg, const sf_model_desc* const* models) {
    Layout L;
    sf_model_desc uni;
    int U = 0, bmax = 0;
    if (multi_layout(segs, nseg, models, &L, &U, &bmax, &uni)) return 0;
    return carve_multi(L, uni, U, bmax, nullptr, 0).bytes;
}
// the single-descriptor entry points: every segment described by `mdl`
static std::vector<const sf_model_desc*> same_desc(int nseg, const sf_model_desc* mdl) {
    return std::vector<const sf_model_desc*>(nseg > 0 ? nseg : 0, mdl);
}
extern "C" size_t sf_multi_workspace_bytes(const sf_segment* segs, int nseg, const sf_model_desc* mdl) {
    if (!mdl) return 0;
    return multi_workspace_bytes(segs, nseg, same_desc(nseg, mdl).data());
}
extern "C" size_t sf_multi_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models) {
    return multi_workspace_bytes(segs, nseg, models);
}
// ---- the gradient's part of a multi-order call (sf_loglike_multi_grad_batch_md)
#define MULTI_GRAD "sf_loglike_multi_grad_batch_md"
struct MultiGradCall {
    const sf_grad_request* reqs;
    double* d_grad;
    int grad_stride;
    MultiGradWork G;  // carved by loglike_multi behind the Work of the call
};
int multi_grad_requests_ok(const sf_segment* segs, int nseg, const sf_model_desc* const* models, const sf_grad_request* reqs,
                           int grad_stride, const char* call) {
    if (!reqs) {
        sf_set_error("%s: requests are required", call);
        return SF_EINVAL;
    }
    bool any = false;
    for (int i = 0; i < nseg; ++i) {
        const sf_grad_request& r = reqs[i];
        char who[96];
        snprintf(who, sizeof who, "%s: segment %d", call, i);
        int slots = 0;
        if (r.n_mean_slots != 0) {
            if (r.n_mean_slots < 0 || !r.h_mean_slots) {
                sf_set_error("%s: n_mean_slots=%d without columns", who, r.n_mean_slots);
                return SF_EINVAL;
            }
            SF_CHECK(mean_slots_ok(who, segs[i].ctx, models[i], r.h_mean_slots, r.n_mean_slots, grad_stride));
            slots += r.n_mean_slots;
        }
        if (r.want_cov) {
            const int cov = sf_cov_grad_slots(models[i]->has_global, models[i]->n_local);
            if (cov == 0) {
                sf_set_error("%s: nothing to differentiate (no global and no local kernel)", who);
                return SF_EINVAL;
            }
            slots += cov;
        }
        if (slots > grad_stride) {
            sf_set_error("%s: grad_stride=%d < %d slots", who, grad_stride, slots);
            return SF_EINVAL;
        }
        if (slots > 0 && segs[i].B > 65535) {  // (the staging and contraction launches take one grid plane per unit)
            sf_set_error("%s: B=%d must lie in 1 .. 65535", who, (int)segs[i].B);
            return SF_EINVAL;
        }
        any |= slots > 0;
    }
    if (!any) {
        sf_set_error("%s: nothing to differentiate (no segment requests a slot)", call);
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_multi_grad_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                   const sf_grad_request* reqs, int grad_stride) {
    Layout L;
    sf_model_desc uni;
    int U = 0, bmax = 0;
    if (multi_layout(segs, nseg, models, &L, &U, &bmax, &uni)) return 0;
    if (multi_grad_requests_ok(segs, nseg, models, reqs, grad_stride, MULTI_GRAD)) return 0;
    return carve_multi_grad(segs, nseg, models, reqs, L, U, nullptr, 0, carve_multi(L, uni, U, bmax, nullptr, 0).bytes).bytes;
}
// On segment i's lane, between its transform chain and its fill: the right-hand sides into the staging area.  The residual
// is read before the factorisation turns it into L^-1 r.
static int multi_grad_stage(const MultiGradCall& g, int i, const sf_ctx* c, int B, const Work& w, const Layout& L, hipStream_t sp) {
    const AppliedWork& aw = g.G.seg[i];
    if (g.reqs[i].n_mean_slots > 0) return sf_launch_mean_stage(w.resid, aw.xs, w.info_e, c->n, L.npad, c->m, B, aw.stage, sp);
    if (g.G.nrhs == 1) return sf_launch_apply_stage(nullptr, c->n, 0, w.resid, c->n, L.npad, 1, B, aw.stage, sp);
    // r alone among units of 1 + m rows: the residual's n data rows into row 0, zero everywhere else
    const size_t unit = sizeof(double) * (size_t)g.G.nrhs * L.npad;
    SF_HIP(hipMemsetAsync(aw.stage, 0, unit * (size_t)B, sp));
    SF_HIP(hipMemcpy2DAsync(aw.stage, unit, w.resid, sizeof(double) * (size_t)L.npad, sizeof(double) * (size_t)c->n, B,
                            hipMemcpyDeviceToDevice, sp));
    return SF_OK;
}
// On segment i's lane behind its own chain: the row tangents read the chain's transient buffers (broadened rows, multiplier
// table, FFT scratch), which the lane's next segment overwrites; they leave per-unit data only (dcoef, kdot, mudot, zdot)
static int multi_grad_tangents(const MultiGradCall& g, int i, sf_ctx* c, const sf_model_desc* mdl, int B, const double* d_params,
                               const Work& w, hipStream_t sp) {
    const sf_grad_request& r = g.reqs[i];
    if (r.n_mean_slots <= 0) return SF_OK;
    return sf_launch_mean_tangents(broaden_args(c, mdl, B, d_params, w), c->inv_band.as<double>(),
                                   emu_args(c, mdl, d_params, w, w.mu, nullptr, w.Lw, w.info_e),
                                   mean_grad_kernel_args(c, r.h_mean_slots, r.n_mean_slots, w, g.G.seg[i], nullptr, g.grad_stride), B, sp);
}
// Behind a chunk's factorisation and finish, on the caller's stream: alpha (and V) for the whole chunk in one launch, X = L^-1
// if a segment of the chunk wants covariance slots, then every segment's contractions.  seg_u0[i]: segment i's first unit
static int multi_grad_chunk(const MultiGradCall& g, const sf_segment* segs, const sf_model_desc* const* models, const Work& W,
                            const Layout& L, const int* seg_u0, int s0, int s1, int* d_info, hipStream_t s) {
    const int u0 = seg_u0[s0], units = seg_u0[s1 - 1] + segs[s1 - 1].B - u0;
    const int64_t stride = (int64_t)L.npad * L.lda, sstride = (int64_t)g.G.nrhs * L.npad;
    const Work wc = slice(W, u0);
    double* stage = g.G.seg[s0].stage;
    SF_CHECK(sf_launch_chol_apply(wc.C, L.npad, L.lda, stride, units, SF_APPLY_CINV, stage, g.G.nrhs, L.npad, sstride, stage, L.npad,
                                  sstride, s));
    bool cov = false;
    for (int i = s0; i < s1; ++i) cov |= g.reqs[i].want_cov != 0;
    // (the factor is applied first: the inverse's launch takes the strict upper triangle of the matrices as scratch)
    if (cov)
        SF_CHECK(sf_launch_chol_inverse_diag(wc.C, L.npad, L.lda, stride, units, g.G.seg[s0].winv, g.G.seg[s0].cinv_diag, L.npad, s));
    for (int i = s0; i < s1; ++i) {
        const sf_grad_request& r = g.reqs[i];
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B;
        AppliedWork aw = g.G.seg[i];
        aw.info = d_info + seg_u0[i];
        Work w = slice(W, seg_u0[i]);
        if (aw.coef) w.coef = aw.coef;
        double* grad = g.d_grad + (int64_t)seg_u0[i] * g.grad_stride;
        if (r.want_cov) {
            sf_fill_args f = fill_args(c, models[i], segs[i].d_params, w);
            f.C = w.C, f.lda = L.lda, f.stride = stride, f.lower_only = 1, f.add_jitter = 1;
            SF_CHECK(sf_launch_cov_grad(f, B, aw.winv, aw.stage, (int)sstride, aw.info, aw.part, grad + r.n_mean_slots, g.grad_stride, s));
        }
        if (r.n_mean_slots > 0)
            SF_CHECK(sf_launch_mean_grad(eval_args(c, models[i], segs[i].d_params, w),
                                         mean_grad_kernel_args(c, r.h_mean_slots, r.n_mean_slots, w, aw, grad, g.grad_stride), w.zs,
                                         c->m * c->M, B, s));
    }
    return SF_OK;
}

// g (gradient calls): what the segments are differentiated in; its workspace lies behind the likelihood's
static int loglike_multi(const char* who, const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                         double* d_lnl, double* d_logdet, double* d_sqmah, double* d_log_scale, int* d_info,
                         void* d_work, size_t work_bytes, void* stream, MultiGradCall* g = nullptr) {
    Layout L;
    sf_model_desc uni;
    int U = 0, bmax = 0;
    int rc = multi_layout(segs, nseg, models, &L, &U, &bmax, &uni);
    if (rc) return rc;
    if (g) SF_CHECK(multi_grad_requests_ok(segs, nseg, models, g->reqs, g->grad_stride, MULTI_GRAD));
    if (!d_lnl || !d_work || (g && (!d_info || !g->d_grad))) {
        sf_set_error(g ? "%s: d_lnl, d_info, d_grad and a workspace are required" : "%s: d_lnl and a workspace are required", who);
        return SF_EINVAL;
    }
    Work W = carve_multi(L, uni, U, bmax, d_work, work_bytes);
    if (g) g->G = carve_multi_grad(segs, nseg, models, g->reqs, L, U, d_work, work_bytes, W.bytes);
    rc = work_fits(work_bytes, g ? g->G.bytes : W.bytes);
    if (rc) return rc;
    sf_ctx* c0 = segs[0].ctx;
    if (use_device(c0)) return SF_EHIP;
    hipStream_t s = (hipStream_t)stream;
    prof_count_call();
    // (one frame for every chunk: the fills run before the chunk sizes are known; a chunk too small for the fused
    // sequences is factorised by them all the same -- sf_launch_potrf honours the frame of the tile map)
    const int fp = sf_potrf_front_pad(L.npad, 1 << 20);
    // Pipeline: the per-order transform chains and fills (many small launches, a few per cent of the step) run on
    // the lanes one chunk of orders ahead of the factorisation on the caller's stream, so all but the first chunk's
    // are hidden behind the Cholesky of the previous chunk (see multi_first_units).
    // (the factorisation has its own executor, exec_potrf: all four streams of c0->exec are free for the chains)
    MultiPipeline pipe;
    SF_CHECK(pipe.begin(&c0->exec, s, nseg, U));
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B;
        const MultiSegment at = pipe.start(i);
        hipStream_t sp = at.stream;
        const int u0 = at.u0;
        Work w = with_trans_set(slice(W, u0), at.lane);
        if (g && g->G.seg[i].coef) w.coef = g->G.seg[i].coef;  // (the contraction reads them behind the factorisation)
        {
            ProfScope ps(sp, PS_TRANSFORM);
            rc = run_transforms(c, models[i], B, segs[i].d_params, w, nullptr, g ? g->G.seg[i].xs : nullptr, nullptr,
                                d_log_scale ? d_log_scale + u0 : nullptr, true, sp);
            if (rc) return rc;
        }
        if (g) SF_CHECK(multi_grad_stage(*g, i, c, B, w, L, sp));
        {
            ProfScope ps(sp, PS_FILL);
            rc = sf_launch_fill(loglike_fill_args(c, models[i], segs[i].d_params, w, L, fp), B, sp);
            if (rc) return rc;
        }
        if (g) SF_CHECK(multi_grad_tangents(*g, i, c, models[i], B, segs[i].d_params, w, sp));
        SF_CHECK(pipe.done(i, B));
    }
    // (sf_launch_potrf rewinds the event pool of the executor it is given: the factorisation uses its own.
    // Two factorisations in flight on two streams, to hide one's under-filled last panels behind the other, were
    // measured slower: 306 vs 291 ms at cfg 3.)
    for (const MultiChunk& ch : pipe.chunks) {
        SF_CHECK(pipe.join(ch));
        rc = loglike_factor_finish(slice(W, ch.u0), L, fp, ch.units, W.ltbuf, d_lnl + ch.u0, d_info ? d_info + ch.u0 : nullptr, s,
                                   &c0->exec_potrf);
        if (rc) return rc;
        if (g) SF_CHECK(multi_grad_chunk(*g, segs, models, W, L, pipe.seg_u0.data(), ch.s0, ch.s1, d_info, s));
    }
    return export_logdet_sqmah(d_logdet, d_sqmah, W, U, s);
}
extern "C" int sf_loglike_multi_batch(const sf_segment* segs, int nseg, const sf_model_desc* mdl, double* d_lnl,
                                      double* d_logdet, double* d_sqmah, double* d_log_scale, int* d_info,
                                      void* d_work, size_t work_bytes, void* stream) {
    if (!mdl) {
        sf_set_error("multi-order call: bad segment list / model descriptor");
        return SF_EINVAL;
    }
    return loglike_multi("sf_loglike_multi_batch", segs, nseg, same_desc(nseg, mdl).data(), d_lnl, d_logdet, d_sqmah,
                         d_log_scale, d_info, d_work, work_bytes, stream);
}
extern "C" int sf_loglike_multi_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                         double* d_lnl, double* d_logdet, double* d_sqmah, double* d_log_scale,
                                         int* d_info, void* d_work, size_t work_bytes, void* stream) {
    return loglike_multi("sf_loglike_multi_batch_md", segs, nseg, models, d_lnl, d_logdet, d_sqmah, d_log_scale,
                         d_info, d_work, work_bytes, stream);
}
extern "C" int sf_loglike_multi_grad_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                              const sf_grad_request* reqs, double* d_lnl, double* d_log_scale, int* d_info,
                                              double* d_grad, int grad_stride, void* d_work, size_t work_bytes, void* stream) {
    MultiGradCall g{reqs, d_grad, grad_stride, {}};
    return loglike_multi(MULTI_GRAD, segs, nseg, models, d_lnl, nullptr, nullptr, d_log_scale, d_info, d_work, work_bytes, stream, &g);
}
extern "C" int sf_multi_grad_reduce(int nseg, int W, const double* d_unit_lnl, const int* d_unit_info, const double* d_unit_grad,
                                    int grad_stride, const int32_t* d_col_ptr, const int32_t* d_col_src, int ncols, double* d_lnl,
                                    double* d_grad, int out_stride, int* d_info, void* stream) {
    if (!d_unit_lnl || !d_unit_info || !d_unit_grad || !d_col_ptr || !d_lnl || !d_grad || !d_info || (!d_col_src && ncols > 0)) {
        sf_set_error("sf_multi_grad_reduce: the unit results, the column map and the outputs are required");
        return SF_EINVAL;
    }
    sf_multi_reduce_args a;
    a.unit_lnl = d_unit_lnl, a.unit_info = d_unit_info, a.unit_grad = d_unit_grad, a.col_ptr = d_col_ptr, a.col_src = d_col_src;
    a.nseg = nseg, a.W = W, a.grad_stride = grad_stride, a.ncols = ncols, a.out_stride = out_stride;
    a.lnl = d_lnl, a.grad = d_grad, a.info = d_info;
    return sf_launch_multi_grad_reduce(a, (hipStream_t)stream);
}

extern "C" int sf_multi_fisher_reduce(int nseg, int W, const double* d_unit_lnl, const int* d_unit_info, const double* d_unit_fisher,
                                      int fisher_ld, int fisher_stride, const int32_t* d_col_ptr, const int32_t* d_col_src, int ncols,
                                      double* d_lnl, double* d_fisher, int out_stride, int* d_info, void* stream) {
    if (!d_unit_lnl || !d_unit_info || !d_unit_fisher || !d_col_ptr || !d_lnl || !d_fisher || !d_info || (!d_col_src && ncols > 0)) {
        sf_set_error("sf_multi_fisher_reduce: the unit results, the column map and the outputs are required");
        return SF_EINVAL;
    }
    sf_multi_fisher_reduce_args a;
    a.unit_lnl = d_unit_lnl, a.unit_info = d_unit_info, a.unit_fisher = d_unit_fisher, a.col_ptr = d_col_ptr, a.col_src = d_col_src;
    a.nseg = nseg, a.W = W, a.fisher_ld = fisher_ld, a.ncols = ncols, a.fisher_stride = fisher_stride, a.out_stride = out_stride;
    a.lnl = d_lnl, a.fisher = d_fisher, a.info = d_info;
    return sf_launch_multi_fisher_reduce(a, (hipStream_t)stream);
}
