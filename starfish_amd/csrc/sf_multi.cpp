// C-ABI host layer: multi-order batches.
// The units of several orders (the reference's multi-order spectra, Starfish/spectrum.py:96-115; orders are
// independent, docs/intro.rst:71-73) share ONE batched factorisation: every order runs its own transform chain
// and covariance fill into its slice of a common [units][npad][lda] array, padded (identity block) to the largest
// order of the group; the Cholesky, which is where the time goes, then sees sum(B_i) matrices in one launch
// sequence instead of nseg half-filled ones, and the host synchronises once.
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
static int loglike_multi(const char* who, const sf_segment* segs, int nseg, const sf_model_desc* const* models,
                         double* d_lnl, double* d_logdet, double* d_sqmah, double* d_log_scale, int* d_info,
                         void* d_work, size_t work_bytes, void* stream) {
    Layout L;
    sf_model_desc uni;
    int U = 0, bmax = 0;
    int rc = multi_layout(segs, nseg, models, &L, &U, &bmax, &uni);
    if (rc) return rc;
    if (!d_lnl || !d_work) {
        sf_set_error("%s: d_lnl and a workspace are required", who);
        return SF_EINVAL;
    }
    Work W = carve_multi(L, uni, U, bmax, d_work, work_bytes);
    rc = work_fits(work_bytes, W.bytes);
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
    };
    std::vector<Chunk> chunks;
    bool lane_used[SF_MULTI_LANES] = {};
    int u0 = 0, cu0 = 0;
    for (int i = 0; i < nseg; ++i) {
        sf_ctx* c = segs[i].ctx;
        const int B = segs[i].B;
        const int lane = i % SF_MULTI_LANES;
        hipStream_t sp = lane_stream[lane];
        lane_used[lane] = true;
        Work w = with_trans_set(slice(W, u0), lane);
        {
            ProfScope ps(sp, PS_TRANSFORM);
            rc = run_transforms(c, models[i], B, segs[i].d_params, w, nullptr, nullptr, nullptr,
                                d_log_scale ? d_log_scale + u0 : nullptr, true, sp);
            if (rc) return rc;
        }
        {
            ProfScope ps(sp, PS_FILL);
            rc = sf_launch_fill(loglike_fill_args(c, models[i], segs[i].d_params, w, L, fp), B, sp);
            if (rc) return rc;
        }
        u0 += B;
        if ((chunks.empty() && u0 - cu0 >= first_units) || i == nseg - 1) {
            Chunk ch{cu0, u0 - cu0, {}};
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
