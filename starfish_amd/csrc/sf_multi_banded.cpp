// C-ABI host layer: multi-order batches on the band + Woodbury solver (the dense calls and what the regrouping is for:
// sf_multi.cpp).  sf_loglike_banded_multi_grad_batch_md is sf_loglike_multi_grad_batch_md without matrices: one launch of
// each band sweep over all units of a chunk.  sf_fisher_banded_multi_batch_md is its regrouping for the Fisher information of the
// mean-flux parameters (one plain sweep over [r; Y; J] per unit), sf_local_scan_banded_multi_batch_md the one for the score scan
// for new local kernels (the keeping sweep, alpha, the selected inversion and Vs, then every order's scan).
#include <algorithm>
#include <string>
#include <vector>

#include "sf_multi_pipeline.h"

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
                              const char* dense = "sf_loglike_multi_grad_batch_md") {
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
// ---- what the two calls share behind a good frame
// the outputs every unit needs (out: the name of the call's own)
static int banded_multi_outputs_ok(const char* who, const char* out, const void* d_lnl, const void* d_info, const void* d_out,
                                   const void* d_work) {
    if (d_lnl && d_info && d_out && d_work) return SF_OK;
    sf_set_error("%s: d_lnl, d_info, %s and a workspace are required", who, out);
    return SF_EINVAL;
}
// the workspace holds `need` bytes, segment 0's device is current and the lanes wait for the caller's stream
static int banded_multi_open(const sf_segment* segs, int nseg, int U, size_t work_bytes, size_t need, void* stream, MultiPipeline* pipe) {
    SF_CHECK(work_fits(work_bytes, need));
    sf_ctx* c0 = segs[0].ctx;
    if (use_device(c0)) return SF_EHIP;
    prof_count_call();
    return pipe->begin(&c0->exec, (hipStream_t)stream, nseg, U);
}
// On a segment's lane sp: its band into the call's frame, then its transform chain.  w: the segment's slice of the Work with the
// lane's transient buffers; u0: its first unit; xs: where the chain leaves the unscaled eigenspectra rows (may be NULL).  A work
// without G.gtab: every entry of the band from its own pixel pair, no table per diagonal (the diagnostics' fill, sf_banded.cpp)
static int banded_multi_segment(const BandMultiWork& G, const sf_segment& seg, const sf_model_desc* mdl, const Work& w, int u0,
                                double* xs, double* d_log_scale, hipStream_t sp) {
    const int64_t sband = (int64_t)G.n16 * G.ldb;
    {
        ProfScope ps(sp, PS_FILL);
        SF_HIP(hipMemsetAsync(w.info_c, 0, sizeof(int) * (size_t)seg.B, sp));
        sf_fill_args f = fill_args(seg.ctx, mdl, seg.d_params, w);
        f.C = nullptr, f.lda = 0, f.stride = 0, f.lower_only = 1, f.add_jitter = 1;
        f.npad = G.n16;  // (identity rows up to the frame's row count)
        SF_CHECK(sf_launch_band_fill(f, seg.B, G.band + (size_t)u0 * sband, G.halfwidth + 1, G.halfwidth, G.ldb, sband, w.info_c,
                                     G.gtab ? G.gtab + (size_t)u0 * (G.ldb + 2) : nullptr, sp));
    }
    ProfScope ps(sp, PS_TRANSFORM);
    return run_transforms(seg.ctx, mdl, seg.B, seg.d_params, w, nullptr, xs, nullptr, d_log_scale ? d_log_scale + u0 : nullptr, true, sp);
}
// the band solver's call for a chunk's units: their bands, the right-hand sides r, the Gram matrices of r.nrhs rows
static sf_band_call banded_multi_sweep(const BandMultiWork& G, const MultiChunk& ch, const Work& wc, const sf_band_rhs& r) {
    const size_t u = (size_t)ch.u0;
    sf_band_call k = {};
    k.sband = (int64_t)G.n16 * G.ldb;
    k.band = G.band + u * k.sband, k.ldb = G.ldb, k.halfwidth = G.halfwidth;
    k.n = G.n16, k.batch = ch.units;
    k.r = r;
    k.logdet = G.logdet_band + u, k.gram = G.gram + u * r.nrhs * r.nrhs, k.info = wc.info_c;
    return k;
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
    SF_CHECK(banded_multi_outputs_ok(BANDED_MULTI_GRAD, "d_grad", d_lnl, d_info, d_grad, d_work));
    const Layout& L = F.L;
    const Work W = carve_banded_multi(F, d_work, work_bytes);
    const BandMultiGradWork G = carve_band_multi_grad(segs, nseg, models, reqs, L, F.n16, F.halfwidth, F.U, d_work, work_bytes, W.bytes);
    MultiPipeline pipe;
    SF_CHECK(banded_multi_open(segs, nseg, F.U, work_bytes, G.bytes, stream, &pipe));
    hipStream_t s = pipe.s;
    const int H = G.halfwidth, n16 = G.n16, nrhs = G.nrhs;
    const int64_t sband = (int64_t)n16 * G.ldb, sstage = (int64_t)nrhs * L.npad;
    const size_t ng = (size_t)nrhs * nrhs;
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B;
        const MultiSegment at = pipe.start(i);
        hipStream_t sp = at.stream;
        Work w = with_trans_set(slice(W, at.u0), at.lane);
        if (G.seg[i].coef) w.coef = G.seg[i].coef;  // (the contraction reads them behind the sweeps)
        SF_CHECK(banded_multi_segment(G, segs[i], models[i], w, at.u0, G.seg[i].xs, d_log_scale, sp));
        const sf_grad_request& r = reqs[i];
        if (r.n_mean_slots > 0)
            SF_CHECK(sf_launch_mean_tangents(broaden_args(c, models[i], B, segs[i].d_params, w), c->inv_band.as<double>(),
                                             emu_args(c, models[i], segs[i].d_params, w, w.mu, nullptr, w.Lw, w.info_e),
                                             mean_grad_kernel_args(c, r.h_mean_slots, r.n_mean_slots, w, G.seg[i], nullptr, grad_stride),
                                             B, sp));
        SF_CHECK(pipe.done(i, B));
    }
    for (const MultiChunk& ch : pipe.chunks) {
        SF_CHECK(pipe.join(ch));
        const Work wc = slice(W, ch.u0);
        const size_t u = (size_t)ch.u0;
        int* info = d_info + ch.u0;
        bool cov = false;
        for (int i = ch.s0; i < ch.s1; ++i) cov |= reqs[i].want_cov != 0;
        {
            ProfScope ps(s, PS_POTRF);
            const sf_band_call k = banded_multi_sweep(G, ch, wc, sf_band_rhs{wc.Y, (int64_t)L.mpad * L.npad, L.npad, nrhs, wc.resid, L.npad});
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
            const size_t su = (size_t)pipe.seg_u0[i];
            AppliedWork aw = G.seg[i];
            aw.info = d_info + pipe.seg_u0[i];
            Work w = slice(W, pipe.seg_u0[i]);
            if (aw.coef) w.coef = aw.coef;
            double* grad = d_grad + (int64_t)pipe.seg_u0[i] * grad_stride;
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
    SF_CHECK(banded_multi_outputs_ok(BANDED_MULTI_FISHER, "d_fisher", d_lnl, d_info, d_fisher, d_work));
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
    MultiPipeline pipe;
    SF_CHECK(banded_multi_open(segs, nseg, F.U, work_bytes, G.bytes, stream, &pipe));
    hipStream_t s = pipe.s;
    const int n16 = G.n16, nin = G.nin, pmax = G.pmax, m = L.m;
    const int64_t sbuf = (int64_t)nin * L.npad;
    const size_t ng = (size_t)nin * nin, nl = (size_t)(1 + m) * (1 + m);
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B, p = reqs[i].n_mean_slots;
        const MultiSegment at = pipe.start(i);
        hipStream_t sp = at.stream;
        const Work w = with_trans_set(slice(W, at.u0), at.lane);
        const AppliedWork& aw = G.seg[i];
        SF_CHECK(banded_multi_segment(G, segs[i], models[i], w, at.u0, aw.xs, d_log_scale, sp));
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
        SF_CHECK(pipe.done(i, B));
    }
    for (const MultiChunk& ch : pipe.chunks) {
        SF_CHECK(pipe.join(ch));
        const Work wc = slice(W, ch.u0);
        const size_t u = (size_t)ch.u0;
        int* info = d_info + ch.u0;
        {
            ProfScope ps(s, PS_POTRF);
            const sf_band_call k = banded_multi_sweep(G, ch, wc, sf_band_rhs{G.buf + u * sbuf, sbuf, L.npad, nin, nullptr, 0});
            if (sf_band_twisted_applicable(n16, G.halfwidth, ch.units)) SF_CHECK(sf_launch_band_forms_twisted(k, G.twist, s));
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

// ----------------------------------------------------------------------------------- multi-order score scan on the band solver
// sf_local_scan_banded_multi_batch_md: the launch structure of the gradient call above with the head that
// sf_local_scan_banded_batch runs (banded_diag_head, sf_banded.cpp, for the walker's own residual with the selected inversion).
// Per segment on its lane: the band fill, entry by entry, and the transform chain; per chunk on the caller's stream, over all
// its units in one launch each: keeping sweep, capacitance step, lnl / info, backward sweep and mix (alpha: one staging row per
// unit), selected inversion and Vs (the m columns alone); then per segment sf_launch_local_scan_banded as it is, with the order's
// own n, grid and slice of the candidates, Sigma / Vs / alpha addressed with the frame's strides.  The frame is BandMultiFrame's
// at the half-width wmax -- the LDS window's widest for 1 + m rows, the single-order call's rule -- whatever the orders' own
// support is: there is no h_halfwidth.  No device code of its own.
#define BANDED_MULTI_SCAN "sf_local_scan_banded_multi_batch_md"
// what the call refuses on its segments before anything is enqueued, and its frame.  *no_band (may be NULL): the refusal is that
// the band solver does not take the orders (a grid that is not strictly increasing, no window), which the patch query answers 0
static int banded_multi_scan_frame(const sf_segment* segs, int nseg, const sf_model_desc* const* models, BandMultiFrame* F,
                                   bool* no_band = nullptr) {
    if (no_band) *no_band = false;
    if (multi_layout(segs, nseg, models, &F->L, &F->U, &F->bmax, &F->uni)) {
        const std::string why = sf_last_error();
        sf_set_error("%s: %s", BANDED_MULTI_SCAN, why.c_str());
        return SF_EINVAL;
    }
    F->n16 = 0;
    for (int i = 0; i < nseg; ++i) {
        const sf_ctx* c = segs[i].ctx;
        if (segs[i].B > 65535) {  // (the fill and the candidates take one grid plane per unit)
            sf_set_error("%s: segment %d: B=%d must lie in 1 .. 65535", BANDED_MULTI_SCAN, i, (int)segs[i].B);
            return SF_EINVAL;
        }
        if (!c->monotonic) {
            if (no_band) *no_band = true;
            sf_set_error("%s: segment %d: the wavelength grid is not monotonic (the band solver needs a strictly increasing one, and a "
                         "candidate's pixels are no contiguous patch)", BANDED_MULTI_SCAN, i);
            return SF_EINVAL;
        }
        F->n16 = std::max(F->n16, (c->n + 15) / 16 * 16);
    }
    const int m = F->L.m;
    F->halfwidth = m < 1 || m > 32 ? -1 : sf_band_max_halfwidth(1 + m);
    if (F->halfwidth < 0) {
        if (no_band) *no_band = true;
        sf_set_error("%s: segment 0: 1 + %d rows exceed the LDS window at every half-width (use sf_local_scan_batch per order)",
                     BANDED_MULTI_SCAN, m);
        return SF_EINVAL;
    }
    return SF_OK;
}
// the candidate lists: nseg + 1 ascending ints on the host, 1 .. 65535 candidates per segment
static int banded_multi_scan_cands_ok(int nseg, const int* h_cand_ptr) {
    if (!h_cand_ptr) {
        sf_set_error("%s: h_cand_ptr (nseg + 1 ascending ints on the host) is required", BANDED_MULTI_SCAN);
        return SF_EINVAL;
    }
    if (h_cand_ptr[0] < 0) {
        sf_set_error("%s: segment 0: h_cand_ptr starts at %d, a negative index", BANDED_MULTI_SCAN, h_cand_ptr[0]);
        return SF_EINVAL;
    }
    for (int i = 0; i < nseg; ++i) {
        const long long count = (long long)h_cand_ptr[i + 1] - h_cand_ptr[i];
        if (count < 1 || count > 65535) {
            sf_set_error("%s: segment %d: %lld candidates (h_cand_ptr %d .. %d) must lie in 1 .. 65535", BANDED_MULTI_SCAN, i, count,
                         h_cand_ptr[i], h_cand_ptr[i + 1]);
            return SF_EINVAL;
        }
    }
    return SF_OK;
}
extern "C" int sf_local_scan_banded_multi_max_patch(const sf_segment* segs, int nseg, const sf_model_desc* const* models) {
    BandMultiFrame F;
    bool no_band = false;
    if (banded_multi_scan_frame(segs, nseg, models, &F, &no_band)) return no_band ? 0 : SF_EINVAL;
    return F.halfwidth + 1;
}
extern "C" size_t sf_local_scan_banded_multi_workspace_bytes_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                                const int* h_cand_ptr) {
    BandMultiFrame F;
    if (banded_multi_scan_frame(segs, nseg, models, &F) || banded_multi_scan_cands_ok(nseg, h_cand_ptr)) return 0;
    return carve_band_multi_scan(segs, nseg, h_cand_ptr, F.L, F.n16, F.halfwidth, F.U, nullptr, 0, carve_banded_multi(F, nullptr, 0).bytes)
        .bytes;
}
extern "C" int sf_local_scan_banded_multi_batch_md(const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                                                   const double* d_cand, const int* h_cand_ptr, double* d_out, double* d_lnl,
                                                   double* d_log_scale, int* d_info, void* d_work, size_t work_bytes, void* stream) {
    BandMultiFrame F;
    SF_CHECK(banded_multi_scan_frame(segs, nseg, models, &F));
    SF_CHECK(banded_multi_scan_cands_ok(nseg, h_cand_ptr));
    if (!d_cand || !d_out || !d_lnl || !d_info || !d_work) {
        sf_set_error("%s: d_cand, d_out, d_lnl, d_info and a workspace are required", BANDED_MULTI_SCAN);
        return SF_EINVAL;
    }
    const Layout& L = F.L;
    const Work W = carve_banded_multi(F, d_work, work_bytes);
    const BandMultiScanWork G = carve_band_multi_scan(segs, nseg, h_cand_ptr, L, F.n16, F.halfwidth, F.U, d_work, work_bytes, W.bytes);
    if (work_bytes < G.bytes) {  // (said here, so that the message names the call)
        sf_set_error("%s: workspace too small: have %zu, need %zu", BANDED_MULTI_SCAN, work_bytes, G.bytes);
        return SF_ENOMEM;
    }
    MultiPipeline pipe;
    SF_CHECK(banded_multi_open(segs, nseg, F.U, work_bytes, G.bytes, stream, &pipe));
    hipStream_t s = pipe.s;
    const int H = G.halfwidth, n16 = G.n16, nrhs = G.nrhs, m = L.m;
    const int64_t sband = (int64_t)n16 * G.ldb, sT = (int64_t)nrhs * L.npad, svs = (int64_t)m * L.npad;
    const size_t ng = (size_t)nrhs * nrhs;
    std::vector<int64_t> out0(nseg);  // where a segment's triples start
    int64_t triples = 0;
    for (int i = 0; i < nseg; ++i) {
        out0[i] = 3 * triples;
        triples += (int64_t)segs[i].B * (h_cand_ptr[i + 1] - h_cand_ptr[i]);
    }
    for (int i = 0; i < nseg; ++i) {
        const MultiSegment at = pipe.start(i);
        const Work w = with_trans_set(slice(W, at.u0), at.lane);
        SF_CHECK(banded_multi_segment(G, segs[i], models[i], w, at.u0, nullptr, d_log_scale, at.stream));
        SF_CHECK(pipe.done(i, segs[i].B));
    }
    for (const MultiChunk& ch : pipe.chunks) {
        SF_CHECK(pipe.join(ch));
        const Work wc = slice(W, ch.u0);
        const size_t u = (size_t)ch.u0;
        int* info = d_info + ch.u0;
        {
            ProfScope ps(s, PS_POTRF);
            const sf_band_call k = banded_multi_sweep(G, ch, wc, sf_band_rhs{wc.Y, (int64_t)L.mpad * L.npad, L.npad, nrhs, wc.resid, L.npad});
            SF_CHECK(sf_launch_band_keep(k, G.fac + u * G.sfac, s));
        }
        {
            ProfScope ps(s, PS_SOLVE);
            SF_CHECK(sf_launch_woodbury(G.gram + u * ng, nrhs, ch.units, G.logdet_band + u, wc.logdet, wc.sqmah, wc.info_c, s));
            SF_CHECK(sf_launch_finish(ch.units, wc.logdet, wc.sqmah, wc.info_e, wc.info_c, d_lnl + ch.u0, info, s));
            // T = Bd^-1 [r, Y^T], alpha = T M in the staging row; the band of Sigma = Bd^-1 and Vs of C^-1 = Sigma - Vs Vs^T
            // (k_band_mix takes one grid plane per unit: slices of at most 65535)
            SF_CHECK(sf_launch_band_back(G.fac + u * G.sfac, n16, H, ch.units, nrhs, info, G.T + u * sT, L.npad, sT, s));
            for (int lo = 0; lo < ch.units; lo += 65535) {
                const int nb = std::min(ch.units - lo, 65535);
                const size_t v = u + lo;
                SF_CHECK(sf_launch_band_mix(G.gram + v * ng, wc.Lw + (size_t)lo * m * m, 1, m, 0, info + lo, nullptr, G.T + v * sT, n16, L.npad,
                                            nb, G.M + v * nrhs, G.stage + v * L.npad, s));
            }
            SF_CHECK(sf_launch_band_selinv(G.fac + u * G.sfac, n16, H, ch.units, nrhs, info, G.sigma + u * sband, G.ldb, sband, s));
            for (int lo = 0; lo < ch.units; lo += 65535) {
                const int nb = std::min(ch.units - lo, 65535);
                const size_t v = u + lo;
                SF_CHECK(sf_launch_band_vs(G.gram + v * ng, 1, m, 0, info + lo, G.T + v * sT, n16, L.npad, nb, G.M2 + v * nrhs * m,
                                           G.vs + v * svs, s));
            }
        }
        for (int i = ch.s0; i < ch.s1; ++i) {
            sf_ctx* c = segs[i].ctx;
            const size_t su = (size_t)pipe.seg_u0[i];
            const Work w = slice(W, pipe.seg_u0[i]);
            SF_CHECK(sf_launch_local_scan_banded(fill_args(c, models[i], segs[i].d_params, w), segs[i].B, G.sigma + su * sband, G.ldb, sband,
                                                 H, G.vs + su * svs, L.npad, svs, m, G.stage + su * L.npad, L.npad, d_info + su,
                                                 d_cand + 2 * (int64_t)h_cand_ptr[i], h_cand_ptr[i + 1] - h_cand_ptr[i], G.patch, G.wband,
                                                 d_out + out0[i], s));
        }
    }
    return SF_OK;
}
// the averaged proposal of one segment's slice (sf_local_scan_multi.h)
extern "C" int sf_local_scan_mean(int B, int ncand, const double* d_out, const int* d_info, double* d_mean, int* d_count, void* stream) {
    return sf_launch_local_scan_mean(B, ncand, d_out, d_info, d_mean, d_count, (hipStream_t)stream);
}
