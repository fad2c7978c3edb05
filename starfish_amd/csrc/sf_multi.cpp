// C-ABI host layer: multi-order batches.
// The units of several orders (the reference's multi-order spectra, Starfish/spectrum.py:96-115; orders are
// independent, docs/intro.rst:71-73) share ONE batched factorisation: every order runs its own transform chain
// and covariance fill into its slice of a common [units][npad][lda] array, padded (identity block) to the largest
// order of the group; the Cholesky, which is where the time goes, then sees sum(B_i) matrices in one launch
// sequence instead of nseg half-filled ones, and the host synchronises once.
// sf_loglike_multi_grad_batch_md is the same sequence with a gradient part (MultiGradCall): right-hand sides staged behind
// every order's chain, the factor applied to a whole chunk's staging area at once, and per segment the contractions of the
// two single-order gradient calls -- one factorisation per unit for the likelihood and its gradient.
// sf_loglike_banded_multi_grad_batch_md (at the end) is that call on the band + Woodbury solver: no matrices, one launch of
// each band sweep over all units of a chunk.  sf_fisher_banded_multi_batch_md is its regrouping for the Fisher information of the
// mean-flux parameters (one plain sweep over [r; Y; J] per unit), sf_multi_fisher_reduce the sum of the unit matrices.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "sf_stages.h"

// models[i] describes the rows of segment i; *uni receives what the shared buffers are sized for (segment 0's
// descriptor with has_vsini set if ANY segment broadens: the transient buffers of the transform chains are shared)
static int multi_layout(const sf_segment* segs, int nseg, const sf_model_desc* const* models, Layout* L, int* units,
                        int* bmax, sf_model_desc* uni) {
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
// Chunks of a multi-order call (whole segments): a SMALL first chunk (at least 256 units: enough matrices to keep a
// factorisation's launches full) and the rest as the second -- only the first chunk's fills are exposed, the others
// run behind the first factorisation.  (Equal chunks: 1, 2, 3, 4 of them gave 283.1, 282.1, 282.7, 283.9 ms at cfg 3.)
// Orders whose transform chains + fills run side by side (own stream and own set of transient buffers each): a chain is
// ~14 small dependent launches, latency-bound -- alone it takes ~1 ms per order with the chip idle around it.
#define SF_MULTI_LANES 3  // (4, 6 and 8 lanes measured: no further gain)
static int multi_first_units(int U) { return std::min(U, 256); }
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
// every per-segment requirement of the two single-order gradient calls, for the segment that requests the part (behind
// multi_layout: contexts and models are good)
// call: the entry point the messages name
static int multi_grad_requests_ok(const sf_segment* segs, int nseg, const sf_model_desc* const* models, const sf_grad_request* reqs,
                                  int grad_stride, const char* call = MULTI_GRAD) {
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
    if (multi_grad_requests_ok(segs, nseg, models, reqs, grad_stride)) return 0;
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
    if (g) SF_CHECK(multi_grad_requests_ok(segs, nseg, models, g->reqs, g->grad_stride));
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
    // the context's auxiliary stream one chunk of orders ahead of the factorisation on the caller's stream, so all
    // but the first chunk's are hidden behind the Cholesky of the previous chunk (see multi_first_units).
    sf_exec* ex = &c0->exec;
    rc = sf_exec_prepare(ex);
    if (rc) return rc;
    // (the factorisation has its own executor, exec_potrf: all four streams of `ex` are free for the chains)
    // (no stream is created for the lanes: every additional ACTIVE stream costs dispatch latency on all of them --
    // one more for the wide sequence's A launches made a cfg-2 step 3 % slower)
    hipStream_t lane_stream[SF_MULTI_LANES] = {ex->aux, ex->side, ex->grp[0]};
    const int first_units = multi_first_units(U);
    SF_HIP(hipEventRecord(ex->fork, s));
    for (int l = 0; l < SF_MULTI_LANES; ++l) SF_HIP(hipStreamWaitEvent(lane_stream[l], ex->fork, 0));
    struct Chunk {
        int u0, units;
        hipEvent_t filled[SF_MULTI_LANES];
        int s0, s1;  // its segments [s0, s1)
    };
    std::vector<Chunk> chunks;
    std::vector<int> seg_u0(nseg);
    bool lane_used[SF_MULTI_LANES] = {};
    int u0 = 0, cu0 = 0, cs0 = 0;
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B;
        const int lane = i % SF_MULTI_LANES;
        hipStream_t sp = lane_stream[lane];
        lane_used[lane] = true;
        seg_u0[i] = u0;
        Work w = with_trans_set(slice(W, u0), lane);
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
        u0 += B;
        if ((chunks.empty() && u0 - cu0 >= first_units) || i == nseg - 1) {
            Chunk ch{cu0, u0 - cu0, {}, cs0, i + 1};
            cs0 = i + 1;
            for (int l = 0; l < SF_MULTI_LANES; ++l) {
                if (!lane_used[l]) continue;
                rc = sf_exec_event(ex, &ch.filled[l]);
                if (rc) return rc;
                SF_HIP(hipEventRecord(ch.filled[l], lane_stream[l]));
                lane_used[l] = false;
            }
            chunks.push_back(ch);
            cu0 = u0;
        }
    }
    // (sf_launch_potrf rewinds the event pool of the executor it is given: the factorisation uses its own.
    // Two factorisations in flight on two streams, to hide one's under-filled last panels behind the other, were
    // measured slower: 306 vs 291 ms at cfg 3.)
    for (const Chunk& ch : chunks) {
        for (int l = 0; l < SF_MULTI_LANES; ++l)
            if (ch.filled[l]) SF_HIP(hipStreamWaitEvent(s, ch.filled[l], 0));
        rc = loglike_factor_finish(slice(W, ch.u0), L, fp, ch.units, W.ltbuf, d_lnl + ch.u0, d_info ? d_info + ch.u0 : nullptr, s,
                                   &c0->exec_potrf);
        if (rc) return rc;
        if (g) SF_CHECK(multi_grad_chunk(*g, segs, models, W, L, seg_u0.data(), ch.s0, ch.s1, d_info, s));
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

// ----------------------------------------------------------------------------------- multi-order gradient on the band solver
// sf_loglike_banded_multi_grad_batch_md: the launch structure of banded_grad_call (sf_banded.cpp), regrouped as loglike_multi
// regroups the dense call.  Per segment on its lane: band fill, transform chain, row tangents, into the segment's slice of
// per-unit arrays with ONE frame (BandMultiFrame); per chunk on the caller's stream, over all its units at once: the keeping
// sweep, the capacitance step and lnl / info, the backward sweep, the mix and, with covariance slots, the selected inversion
// and Vs; then per segment the two contractions with the order's own n.
// The frame is taken from the whole call -- the largest n16, npad and half-width of its segments -- never from a chunk: a
// shorter order's rows n .. n16 are identity rows of the band (the fill's npad argument) with zero right-hand sides (the
// transform chain pads its rows to the layout's npad), which add 0 to the log-determinant and the Gram matrix and come out
// of the backward sweep as zeros; a wider window than a unit needs holds zeros of the band.  No device code of its own.
#define BANDED_MULTI_GRAD "sf_loglike_banded_multi_grad_batch_md"
struct BandMultiFrame {
    Layout L;
    sf_model_desc uni;
    int U, bmax, n16, halfwidth;
};
// who: the entry point the messages name; dense: the call they point to for what the window does not take
static int banded_multi_frame(const sf_segment* segs, int nseg, const sf_model_desc* const* models, const sf_grad_request* reqs,
                              const int* h_halfwidth, int grad_stride, BandMultiFrame* F, const char* who = BANDED_MULTI_GRAD,
                              const char* dense = MULTI_GRAD) {
    if (segs && nseg > 0 && models) {
        if (!h_halfwidth) {
            sf_set_error("%s: h_halfwidth (one half-width per segment) is required", who);
            return SF_EINVAL;
        }
        // (no context is needed to refuse what no window takes; with one, the limit is that of its 1 + m right-hand sides)
        for (int i = 0; i < nseg; ++i) {
            const sf_ctx* c = segs[i].ctx;
            const bool have = c && c->n;
            if (have && !c->monotonic) {
                sf_set_error("%s: segment %d: the banded solver needs a strictly increasing wavelength grid (use %s)", who, i, dense);
                return SF_EINVAL;
            }
            const int wmax = have ? sf_banded_window_halfwidth(c) : sf_band_max_halfwidth(1);
            if (h_halfwidth[i] < 0 || h_halfwidth[i] > wmax) {
                sf_set_error("%s: segment %d: half-width %d outside [0, %d], the LDS window (use %s)", who, i, h_halfwidth[i], wmax,
                             dense);
                return SF_EINVAL;
            }
        }
    }
    SF_CHECK(multi_layout(segs, nseg, models, &F->L, &F->U, &F->bmax, &F->uni));
    SF_CHECK(multi_grad_requests_ok(segs, nseg, models, reqs, grad_stride, who));
    F->n16 = 0, F->halfwidth = 0;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].B > 65535) {  // (the fill and the tangents take one grid plane per unit)
            sf_set_error("%s: segment %d: B=%d must lie in 1 .. 65535", who, i, (int)segs[i].B);
            return SF_EINVAL;
        }
        F->n16 = std::max(F->n16, (segs[i].ctx->n + 15) / 16 * 16);
        F->halfwidth = std::max(F->halfwidth, h_halfwidth[i]);
    }
    return SF_OK;
}
// the likelihood's workspace without matrices, then the band solver's
static Work carve_banded_multi(const BandMultiFrame& F, void* p, size_t cap) {
    return carve(F.L, &F.uni, F.U, F.bmax, p, cap, false, 0, SF_MULTI_LANES);
}
extern "C" size_t sf_banded_multi_grad_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                          const sf_grad_request* reqs, const int* h_halfwidth, int grad_stride) {
    BandMultiFrame F;
    if (banded_multi_frame(segs, nseg, models, reqs, h_halfwidth, grad_stride, &F)) return 0;
    return carve_band_multi_grad(segs, nseg, models, reqs, F.L, F.n16, F.halfwidth, F.U, nullptr, 0,
                                 carve_banded_multi(F, nullptr, 0).bytes).bytes;
}
// k_band_mix takes one grid plane per unit: the mix (and Vs) of `units` units in slices of at most 65535
static int banded_multi_mix(const BandMultiGradWork& G, const Work& wc, const Layout& L, int u0, int units, const int* info, bool vs,
                            hipStream_t s) {
    const size_t ng = (size_t)G.nrhs * G.nrhs, unit = (size_t)G.nrhs * L.npad;
    for (int lo = 0; lo < units; lo += 65535) {
        const int nb = std::min(units - lo, 65535);
        const size_t u = (size_t)u0 + lo;
        if (!vs)
            SF_CHECK(sf_launch_band_mix(G.gram + u * ng, wc.Lw + (size_t)lo * L.m * L.m, 1, L.m, L.m, info + lo, nullptr, G.T + u * unit, G.n16, L.npad, nb,
                                        G.M + u * ng, G.stage + u * unit, s));
        else
            SF_CHECK(sf_launch_band_vs(G.gram + u * ng, 1, L.m, 1, info + lo, G.T + u * unit, G.n16, L.npad, nb, G.M2 + u * ng,
                                       G.stage2 + u * unit, s));
    }
    return SF_OK;
}
extern "C" int sf_loglike_banded_multi_grad_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                     const sf_grad_request* reqs, const int* h_halfwidth, double* d_lnl,
                                                     double* d_log_scale, int* d_info, double* d_grad, int grad_stride, void* d_work,
                                                     size_t work_bytes, void* stream) {
    BandMultiFrame F;
    SF_CHECK(banded_multi_frame(segs, nseg, models, reqs, h_halfwidth, grad_stride, &F));
    if (!d_lnl || !d_info || !d_grad || !d_work) {
        sf_set_error(BANDED_MULTI_GRAD ": d_lnl, d_info, d_grad and a workspace are required");
        return SF_EINVAL;
    }
    const Layout& L = F.L;
    const Work W = carve_banded_multi(F, d_work, work_bytes);
    const BandMultiGradWork G = carve_band_multi_grad(segs, nseg, models, reqs, L, F.n16, F.halfwidth, F.U, d_work, work_bytes, W.bytes);
    SF_CHECK(work_fits(work_bytes, G.bytes));
    sf_ctx* c0 = segs[0].ctx;
    if (use_device(c0)) return SF_EHIP;
    hipStream_t s = (hipStream_t)stream;
    prof_count_call();
    sf_exec* ex = &c0->exec;
    SF_CHECK(sf_exec_prepare(ex));
    hipStream_t lane_stream[SF_MULTI_LANES] = {ex->aux, ex->side, ex->grp[0]};
    const int H = G.halfwidth, n16 = G.n16, nrhs = G.nrhs, first_units = multi_first_units(F.U);
    const int64_t sband = (int64_t)n16 * G.ldb, sstage = (int64_t)nrhs * L.npad;
    const size_t ng = (size_t)nrhs * nrhs;
    SF_HIP(hipEventRecord(ex->fork, s));
    for (int l = 0; l < SF_MULTI_LANES; ++l) SF_HIP(hipStreamWaitEvent(lane_stream[l], ex->fork, 0));
    struct Chunk {
        int u0, units;
        hipEvent_t filled[SF_MULTI_LANES];
        int s0, s1;  // its segments [s0, s1)
    };
    std::vector<Chunk> chunks;
    std::vector<int> seg_u0(nseg);
    bool lane_used[SF_MULTI_LANES] = {};
    int u0 = 0, cu0 = 0, cs0 = 0;
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B;
        const int lane = i % SF_MULTI_LANES;
        hipStream_t sp = lane_stream[lane];
        lane_used[lane] = true;
        seg_u0[i] = u0;
        Work w = with_trans_set(slice(W, u0), lane);
        if (G.seg[i].coef) w.coef = G.seg[i].coef;  // (the contraction reads them behind the sweeps)
        {
            ProfScope ps(sp, PS_FILL);
            SF_HIP(hipMemsetAsync(w.info_c, 0, sizeof(int) * (size_t)B, sp));
            sf_fill_args f = fill_args(c, models[i], segs[i].d_params, w);
            f.C = nullptr, f.lda = 0, f.stride = 0, f.lower_only = 1, f.add_jitter = 1;
            f.npad = n16;  // (identity rows up to the frame's row count)
            SF_CHECK(sf_launch_band_fill(f, B, G.band + (size_t)u0 * sband, H + 1, H, G.ldb, sband, w.info_c,
                                         G.gtab + (size_t)u0 * (G.ldb + 2), sp));
        }
        {
            ProfScope ps(sp, PS_TRANSFORM);
            SF_CHECK(run_transforms(c, models[i], B, segs[i].d_params, w, nullptr, G.seg[i].xs, nullptr,
                                    d_log_scale ? d_log_scale + u0 : nullptr, true, sp));
        }
        const sf_grad_request& r = reqs[i];
        if (r.n_mean_slots > 0)
            SF_CHECK(sf_launch_mean_tangents(broaden_args(c, models[i], B, segs[i].d_params, w), c->inv_band.as<double>(),
                                             emu_args(c, models[i], segs[i].d_params, w, w.mu, nullptr, w.Lw, w.info_e),
                                             mean_grad_kernel_args(c, r.h_mean_slots, r.n_mean_slots, w, G.seg[i], nullptr, grad_stride),
                                             B, sp));
        u0 += B;
        // (loglike_multi's chunks; a chunk every 256 units instead: 51.7 against 51.2 ms of device time at 25 x 3000 x 64)
        if ((chunks.empty() && u0 - cu0 >= first_units) || i == nseg - 1) {
            Chunk ch{cu0, u0 - cu0, {}, cs0, i + 1};
            cs0 = i + 1;
            for (int l = 0; l < SF_MULTI_LANES; ++l) {
                if (!lane_used[l]) continue;
                SF_CHECK(sf_exec_event(ex, &ch.filled[l]));
                SF_HIP(hipEventRecord(ch.filled[l], lane_stream[l]));
                lane_used[l] = false;
            }
            chunks.push_back(ch);
            cu0 = u0;
        }
    }
    for (const Chunk& ch : chunks) {
        for (int l = 0; l < SF_MULTI_LANES; ++l)
            if (ch.filled[l]) SF_HIP(hipStreamWaitEvent(s, ch.filled[l], 0));
        const Work wc = slice(W, ch.u0);
        const size_t u = (size_t)ch.u0;
        int* info = d_info + ch.u0;
        bool cov = false;
        for (int i = ch.s0; i < ch.s1; ++i) cov |= reqs[i].want_cov != 0;
        {
            ProfScope ps(s, PS_POTRF);
            sf_band_call k = {};
            k.band = G.band + u * sband, k.sband = sband, k.ldb = G.ldb, k.halfwidth = H;
            k.n = n16, k.batch = ch.units;
            k.r = sf_band_rhs{wc.Y, (int64_t)L.mpad * L.npad, L.npad, nrhs, wc.resid, L.npad};
            k.logdet = G.logdet_band + u, k.gram = G.gram + u * ng, k.info = wc.info_c;
            SF_CHECK(sf_launch_band_keep(k, G.fac + u * G.sfac, s));
        }
        {
            ProfScope ps(s, PS_SOLVE);
            SF_CHECK(sf_launch_woodbury(G.gram + u * ng, nrhs, ch.units, G.logdet_band + u, wc.logdet, wc.sqmah, wc.info_c, s));
            SF_CHECK(sf_launch_finish(ch.units, wc.logdet, wc.sqmah, wc.info_e, wc.info_c, d_lnl + ch.u0, info, s));
            // T = Bd^-1 [r, Y^T], then [alpha, V] = T M in the staging area
            SF_CHECK(sf_launch_band_back(G.fac + u * G.sfac, n16, H, ch.units, nrhs, info, G.T + u * sstage, L.npad, sstage, s));
            SF_CHECK(banded_multi_mix(G, wc, L, ch.u0, ch.units, info, false, s));
            if (cov) {
                SF_CHECK(sf_launch_band_selinv(G.fac + u * G.sfac, n16, H, ch.units, nrhs, info, G.sigma + u * sband, G.ldb, sband, s));
                SF_CHECK(banded_multi_mix(G, wc, L, ch.u0, ch.units, info, true, s));
            }
        }
        for (int i = ch.s0; i < ch.s1; ++i) {
            const sf_grad_request& r = reqs[i];
            sf_ctx* c = segs[i].ctx;
            const int B = segs[i].B;
            const size_t su = (size_t)seg_u0[i];
            AppliedWork aw = G.seg[i];
            aw.info = d_info + seg_u0[i];
            Work w = slice(W, seg_u0[i]);
            if (aw.coef) w.coef = aw.coef;
            double* grad = d_grad + (int64_t)seg_u0[i] * grad_stride;
            if (r.n_mean_slots > 0)
                SF_CHECK(sf_launch_mean_grad(eval_args(c, models[i], segs[i].d_params, w),
                                             mean_grad_kernel_args(c, r.h_mean_slots, r.n_mean_slots, w, aw, grad, grad_stride), w.zs,
                                             c->m * c->M, B, s));
            if (r.want_cov)
                SF_CHECK(sf_launch_band_cov_grad(fill_args(c, models[i], segs[i].d_params, w), B, G.sigma + su * sband, G.ldb, sband, H,
                                                 aw.stage, G.stage2 + su * sstage + L.npad, L.npad, sstage, c->m, aw.info, aw.part,
                                                 grad + r.n_mean_slots, grad_stride, s));
        }
    }
    return SF_OK;
}

// ----------------------------------------------------------------------------------- multi-order Fisher information on the band solver
// sf_fisher_banded_multi_batch_md: the launch structure above with the head of sf_fisher_banded_mean_batch (banded_head,
// sf_banded.cpp) in place of the gradient's.  Per segment on its lane: band fill, transform chain, row tangents, then the sweep's
// rows [r; Y; J] into the segment's slice of one per-unit row buffer; per chunk on the caller's stream, over all its units at
// once: ONE sweep -- the likelihood's, not a keeping one -- the capacitance step, lnl / info and F = G_JJ - U^T U.  The frame is
// BandMultiFrame's with the largest row count 1 + m + max p_i: an order with fewer columns carries zero rows behind its own.
#define BANDED_MULTI_FISHER "sf_fisher_banded_multi_batch_md"
struct BandMultiFisherFrame {
    BandMultiFrame F;
    int pmax;
};
// what the call refuses before anything is enqueued, and its frame
static int banded_multi_fisher_frame(const sf_segment* segs, int nseg, const sf_model_desc* const* models, const sf_grad_request* reqs,
                                     const int* h_halfwidth, BandMultiFisherFrame* X) {
    if (!reqs) {
        sf_set_error(BANDED_MULTI_FISHER ": requests are required");
        return SF_EINVAL;
    }
    X->pmax = 0;
    for (int i = 0; i < nseg; ++i) {
        if (reqs[i].want_cov) {
            sf_set_error(BANDED_MULTI_FISHER ": segment %d: want_cov must be 0 (the covariance block is not computed)", i);
            return SF_EINVAL;
        }
        if (reqs[i].n_mean_slots < 1) {
            sf_set_error(BANDED_MULTI_FISHER ": segment %d: no mean slot to take the Fisher information in", i);
            return SF_EINVAL;
        }
        X->pmax = std::max(X->pmax, (int)reqs[i].n_mean_slots);
    }
    SF_CHECK(banded_multi_frame(segs, nseg, models, reqs, h_halfwidth, SF_MEAN_GRAD_MAX_SLOTS, &X->F, BANDED_MULTI_FISHER,
                                "sf_fisher_mean_batch"));
    // the window's limit at the CALL's row count (fisher_window_ok's, sf_banded.cpp, for the frame)
    const int m = X->F.L.m, nin = 1 + m + X->pmax;
    if (m < 1 || m > 32 || sfb_admit(X->F.halfwidth, nin) != SFB_WINDOW) {
        sf_set_error(BANDED_MULTI_FISHER ": half-width %d with 1 + %d + %d rows lies outside the LDS window (at most %d at this row "
                     "count; use sf_fisher_mean_batch)", X->F.halfwidth, m, X->pmax, sf_band_max_halfwidth(nin));
        return SF_EINVAL;
    }
    return SF_OK;
}
extern "C" size_t sf_fisher_banded_multi_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                            const sf_grad_request* reqs, const int* h_halfwidth) {
    BandMultiFisherFrame X;
    if (banded_multi_fisher_frame(segs, nseg, models, reqs, h_halfwidth, &X)) return 0;
    const BandMultiFrame& F = X.F;
    return carve_band_multi_fisher(segs, nseg, models, reqs, F.L, F.n16, F.halfwidth, X.pmax, F.U, nullptr, 0,
                                   carve_banded_multi(F, nullptr, 0).bytes).bytes;
}
extern "C" int sf_fisher_banded_multi_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                               const sf_grad_request* reqs, const int* h_halfwidth, double* d_lnl, double* d_log_scale,
                                               int* d_info, double* d_fisher, int fisher_ld, int fisher_stride, void* d_work,
                                               size_t work_bytes, void* stream) {
    BandMultiFisherFrame X;
    SF_CHECK(banded_multi_fisher_frame(segs, nseg, models, reqs, h_halfwidth, &X));
    if (!d_lnl || !d_info || !d_fisher || !d_work) {
        sf_set_error(BANDED_MULTI_FISHER ": d_lnl, d_info, d_fisher and a workspace are required");
        return SF_EINVAL;
    }
    if (fisher_ld < X.pmax || (int64_t)fisher_stride < (int64_t)fisher_ld * fisher_ld) {
        sf_set_error(BANDED_MULTI_FISHER ": fisher_ld=%d < %d columns or fisher_stride=%d < fisher_ld^2", fisher_ld, X.pmax,
                     fisher_stride);
        return SF_EINVAL;
    }
    const BandMultiFrame& F = X.F;
    const Layout& L = F.L;
    const Work W = carve_banded_multi(F, d_work, work_bytes);
    const BandMultiFisherWork G = carve_band_multi_fisher(segs, nseg, models, reqs, L, F.n16, F.halfwidth, X.pmax, F.U, d_work,
                                                          work_bytes, W.bytes);
    SF_CHECK(work_fits(work_bytes, G.bytes));
    sf_ctx* c0 = segs[0].ctx;
    if (use_device(c0)) return SF_EHIP;
    hipStream_t s = (hipStream_t)stream;
    prof_count_call();
    sf_exec* ex = &c0->exec;
    SF_CHECK(sf_exec_prepare(ex));
    hipStream_t lane_stream[SF_MULTI_LANES] = {ex->aux, ex->side, ex->grp[0]};
    const int H = G.halfwidth, n16 = G.n16, nin = G.nin, pmax = G.pmax, m = L.m, first_units = multi_first_units(F.U);
    const int64_t sband = (int64_t)n16 * G.ldb, sbuf = (int64_t)nin * L.npad;
    const size_t ng = (size_t)nin * nin, nl = (size_t)(1 + m) * (1 + m);
    SF_HIP(hipEventRecord(ex->fork, s));
    for (int l = 0; l < SF_MULTI_LANES; ++l) SF_HIP(hipStreamWaitEvent(lane_stream[l], ex->fork, 0));
    struct Chunk {
        int u0, units;
        hipEvent_t filled[SF_MULTI_LANES];
    };
    std::vector<Chunk> chunks;
    bool lane_used[SF_MULTI_LANES] = {};
    int u0 = 0, cu0 = 0;
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B, p = reqs[i].n_mean_slots;
        const int lane = i % SF_MULTI_LANES;
        hipStream_t sp = lane_stream[lane];
        lane_used[lane] = true;
        const Work w = with_trans_set(slice(W, u0), lane);
        const AppliedWork& aw = G.seg[i];
        {
            ProfScope ps(sp, PS_FILL);
            SF_HIP(hipMemsetAsync(w.info_c, 0, sizeof(int) * (size_t)B, sp));
            sf_fill_args f = fill_args(c, models[i], segs[i].d_params, w);
            f.C = nullptr, f.lda = 0, f.stride = 0, f.lower_only = 1, f.add_jitter = 1;
            f.npad = n16;  // (identity rows up to the frame's row count)
            SF_CHECK(sf_launch_band_fill(f, B, G.band + (size_t)u0 * sband, H + 1, H, G.ldb, sband, w.info_c,
                                         G.gtab + (size_t)u0 * (G.ldb + 2), sp));
        }
        {
            ProfScope ps(sp, PS_TRANSFORM);
            SF_CHECK(run_transforms(c, models[i], B, segs[i].d_params, w, nullptr, aw.xs, nullptr, d_log_scale ? d_log_scale + u0 : nullptr,
                                    true, sp));
        }
        sf_mean_grad_args cols = mean_grad_kernel_args(c, reqs[i].h_mean_slots, p, w, aw, nullptr, 0);
        cols.info = w.info_e;  // (before the sweep: the transform chain's status)
        SF_CHECK(sf_launch_mean_tangents(broaden_args(c, models[i], B, segs[i].d_params, w), c->inv_band.as<double>(),
                                         emu_args(c, models[i], segs[i].d_params, w, w.mu, nullptr, w.Lw, w.info_e), cols, B, sp, false));
        // the unit's rows: [r; Y] (zero right-hand sides on a shorter order's padding), its p columns, zero rows up to the frame's
        SF_CHECK(sf_launch_fisher_rows(w.resid, w.Y, (int64_t)L.mpad * L.npad, c->n, L.npad, m, nin, B, aw.stage, sp));
        SF_CHECK(sf_launch_fisher_tangents(eval_args(c, models[i], segs[i].d_params, w), cols, aw.stage + (int64_t)(1 + m) * L.npad, sbuf, B,
                                           sp));
        if (p < pmax)
            SF_HIP(hipMemset2DAsync(aw.stage + (int64_t)(1 + m + p) * L.npad, sizeof(double) * (size_t)sbuf, 0,
                                    sizeof(double) * (size_t)(pmax - p) * L.npad, B, sp));
        u0 += B;
        if ((chunks.empty() && u0 - cu0 >= first_units) || i == nseg - 1) {  // (the gradient call's chunks)
            Chunk ch{cu0, u0 - cu0, {}};
            for (int l = 0; l < SF_MULTI_LANES; ++l) {
                if (!lane_used[l]) continue;
                SF_CHECK(sf_exec_event(ex, &ch.filled[l]));
                SF_HIP(hipEventRecord(ch.filled[l], lane_stream[l]));
                lane_used[l] = false;
            }
            chunks.push_back(ch);
            cu0 = u0;
        }
    }
    for (const Chunk& ch : chunks) {
        for (int l = 0; l < SF_MULTI_LANES; ++l)
            if (ch.filled[l]) SF_HIP(hipStreamWaitEvent(s, ch.filled[l], 0));
        const Work wc = slice(W, ch.u0);
        const size_t u = (size_t)ch.u0;
        int* info = d_info + ch.u0;
        {
            ProfScope ps(s, PS_POTRF);
            sf_band_call k = {};
            k.band = G.band + u * sband, k.sband = sband, k.ldb = G.ldb, k.halfwidth = H;
            k.n = n16, k.batch = ch.units;
            k.r = sf_band_rhs{G.buf + u * sbuf, sbuf, L.npad, nin, nullptr, 0};
            k.logdet = G.logdet_band + u, k.gram = G.gram + u * ng, k.info = wc.info_c;
            if (sf_band_twisted_applicable(n16, H, ch.units)) SF_CHECK(sf_launch_band_forms_twisted(k, G.twist, s));
            else SF_CHECK(sf_launch_band_forms(k, s));
        }
        {
            ProfScope ps(s, PS_SOLVE);
            SF_CHECK(sf_launch_fisher_lead(G.gram + u * ng, nin, m + 1, ch.units, G.lead + u * nl, s));
            SF_CHECK(sf_launch_woodbury(G.lead + u * nl, m + 1, ch.units, G.logdet_band + u, wc.logdet, wc.sqmah, wc.info_c, s));
            SF_CHECK(sf_launch_finish(ch.units, wc.logdet, wc.sqmah, wc.info_e, wc.info_c, d_lnl + ch.u0, info, s));
            // (k_fisher_band's leading dimension is its column count: compact pmax x pmax blocks, then the caller's layout)
            SF_CHECK(sf_launch_fisher_band(G.gram + u * ng, m, pmax, ch.units, info, G.fcomp + u * pmax * pmax, (int64_t)pmax * pmax, s));
            SF_CHECK(sf_launch_fisher_spread(G.fcomp + u * pmax * pmax, pmax, ch.units, d_fisher + (int64_t)ch.u0 * fisher_stride, fisher_ld,
                                             fisher_stride, s));
        }
    }
    return SF_OK;
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
